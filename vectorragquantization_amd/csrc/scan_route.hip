// scan_route.hip -- the Phase-I route (host only): the one place that decides which scan runs for a call
// shape, plans it and says where its lists land.  vrq_hamming_topk, vrq_search3* / vrq_search3_dim*,
// vrq_search2* and the vrq_scan_* introspection (select_rescore.hip) all go through it.
#include "vrq_scan.h"

namespace vrq {

int phase1_route(int64_t n, int cb, int nq, int K, int flags, Phase1Route* r) {
  if (n < 1 || nq < 1 || K < 1) return VRQ_EINVAL;
  r->mfma = cb == 128 ? mfma_use(n, nq, K, flags) : mfma_dim_use(n, cb, nq, K, flags);
  if (r->mfma) {
    const int rc = cb == 128 ? mfma_plan(n, nq, K, &r->mp) : mfma_dim_plan(n, cb, nq, K, &r->mp);
    if (rc != VRQ_OK) return rc;
    // the matrix-core scans leave one sorted K-list per query (their suffix stage)
    r->bytes = r->mp.bytes;
    r->off_lists = r->mp.off_suffix;
    r->nl = 1;
    r->sorted = true;
    return VRQ_OK;
  }
  const int rc = scan_plan(n, cb, nq, K, &r->sp);
  if (rc != VRQ_OK) return rc;
  if (r->sp.nchunks > MAX_LISTS) return VRQ_EUNSUPPORTED;
  r->bytes = r->sp.list_bytes;
  r->off_lists = 0;
  r->nl = r->sp.nchunks;
  r->sorted = false;
  return VRQ_OK;
}

int phase1_launch(const Phase1Route& r, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                  void* ws, hipStream_t s, int flags) {
  if (!r.mfma) return scan_launch(r.sp, codes, n, cb, q, nq, K, (uint64_t*)ws, s);
  return cb == 128 ? mfma_scan_launch(r.mp, codes, n, q, nq, K, (uint8_t*)ws, s, flags)
                   : mfma_dim_scan_launch(r.mp, codes, n, cb, q, nq, K, (uint8_t*)ws, s, flags);
}

size_t phase1_workspace_bytes(int64_t n, int cb, int nq, int K) {
  // the wavefront scan serves every shape that has a route; the matrix-core scan, forced, is chosen
  // wherever any flags choose it.  Sized for both, whatever the flags of the call will be.
  Phase1Route v, m;
  if (phase1_route(n, cb, nq, K, VRQ_SEARCH_SCAN_VALU, &v) != VRQ_OK) return 0;
  if (phase1_route(n, cb, nq, K, VRQ_SEARCH_SCAN_MFMA, &m) != VRQ_OK) return v.bytes;
  return m.bytes > v.bytes ? m.bytes : v.bytes;
}

}  // namespace vrq
