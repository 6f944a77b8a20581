// count_route.hip -- the counting-scan route (host only): the plan of K1h (hamming_count.hip) and of K1hm
// (hamming_count_mfma.hip), the choice between the two engines, the workspace a call needs, and the one loop
// over passes and stages that runs either.  The vrq_*_large, vrq_*_filtered, vrq_*_batch and sharded *_large
// entry points and the vrq_scan_*_plan introspection (select_rescore.hip) all go through it.  The measured
// tables (large_qg_of / large_waves_of, large_mfma_min_queries / _mb_of / _qreal_of) stay with their kernels.
#include "vrq_scan.h"

namespace vrq {

static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// rows per chunk (a multiple of 64) for about `want` chunks: at least kMinChunkRows rows; at most kLargeMaxChunks
// chunks and kLargeHistBytes of histograms per pass of qb queries, but chunks of at most 2^30 rows
static int64_t large_chunk_rows(int64_t n, int64_t want, int qb, int64_t bins) {
  if (want < 1) want = 1;
  int64_t rows = (n + want - 1) / want;
  if (rows < kMinChunkRows) rows = kMinChunkRows;
  int64_t maxc = kLargeHistBytes / (qb * bins * 4);
  if (maxc > kLargeMaxChunks) maxc = kLargeMaxChunks;
  const int64_t minc = (n + (int64_t(1) << 30) - 1) >> 30;
  if (maxc < minc) maxc = minc;
  if (maxc < 1) maxc = 1;
  if (rows < (n + maxc - 1) / maxc) rows = (n + maxc - 1) / maxc;
  return (rows + 63) & ~int64_t(63);
}

// the chunks and the workspace layout of a plan whose chunk_rows is set (the same for both engines)
static void large_layout(CountPlan* p, int64_t n, int nq, int qb, int K, int64_t bins) {
  p->nchunks = (int)((n + p->chunk_rows - 1) / p->chunk_rows);
  size_t off = 0;
  p->off_hist = off;
  off = align256(off + (size_t)qb * p->nchunks * bins * 4);
  p->off_prefix = off;
  off = align256(off + (size_t)nq * p->nchunks * 4 * sizeof(int32_t));
  p->off_tc = off;
  off = align256(off + (size_t)nq * 2 * sizeof(int32_t));
  p->off_lists = off;
  off = align256(off + (size_t)nq * K * sizeof(uint64_t));
  p->off_s2 = off;
  off = align256(off + (size_t)nq * K * sizeof(double));
  p->off_s3 = off;
  off = align256(off + (size_t)nq * K * sizeof(double));
  p->off_ord = off;
  off = align256(off + (size_t)nq * K * sizeof(int32_t));
  p->off_kp = off;
  off = align256(off + (size_t)nq * sizeof(int32_t));
  p->bytes = p->need = off;
}

// the plan of one engine for a shape count_route accepted: the engines differ in the queries of a count
// workgroup and in the number of workgroups their chunking aims at
static void large_plan(int64_t n, int cb, int nq, int K, int engine, CountPlan* p) {
  const bool mfma = engine == VRQ_LARGE_ENGINE_MFMA;
  const int64_t bins = (int64_t)cb * 8 + 1;
  const int qb = nq < kLargeQueryBatch ? nq : kLargeQueryBatch;  // queries of one pass
  p->engine = engine;
  p->mb = mfma ? large_mfma_mb_of(cb, qb) : 0;
  p->qpw = mfma ? large_mfma_qreal_of(cb) * p->mb : large_qg_of(cb);
  p->nqb = (qb + p->qpw - 1) / p->qpw;
  p->passes = (nq + kLargeQueryBatch - 1) / kLargeQueryBatch;
  // K1h: query groups x chunks near kTargetWaves / nw workgroups.  K1hm: chunks x query blocks near
  // kTargetWaves / 4 count workgroups (one per CU at a time: the bins fill its LDS)
  p->chunk_rows = large_chunk_rows(n, kTargetWaves / (mfma ? 4 : large_waves_of(cb)) / p->nqb, qb, bins);
  large_layout(p, n, nq, qb, K, bins);
  p->flush_rows = mfma && p->chunk_rows > large_mfma_flush_rows() ? large_mfma_flush_rows() : 0;
}

int count_route(int64_t n, int cb, int nq, int K, int engine, bool either, CountPlan* p) {
  if (engine < VRQ_LARGE_ENGINE_AUTO || engine > VRQ_LARGE_ENGINE_MFMA) return VRQ_EINVAL;
  if (n < 1 || nq < 1 || K < 1) return VRQ_EINVAL;
  if (!(cb == 128 || dim_code_bytes_supported(cb)) || K > VRQ_K_LARGE_MAX || n >= (int64_t(1) << 32))
    return VRQ_EUNSUPPORTED;
  if (engine == VRQ_LARGE_ENGINE_AUTO)
    engine = nq >= large_mfma_min_queries(cb) ? VRQ_LARGE_ENGINE_MFMA : VRQ_LARGE_ENGINE_VALU;
  large_plan(n, cb, nq, K, engine, p);
  if (either) {  // the workspace covers either engine
    CountPlan other;
    large_plan(n, cb, nq, K, VRQ_LARGE_ENGINE_VALU + VRQ_LARGE_ENGINE_MFMA - engine, &other);
    if (other.bytes > p->need) p->need = other.bytes;
  }
  return VRQ_OK;
}

int count_route_launch(const CountPlan& p, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                       uint8_t* ws, hipStream_t s, int stages, const RowFilter& filter) {
  const bool mfma = p.engine == VRQ_LARGE_ENGINE_MFMA;
  // not a plan of this engine
  if ((!mfma && p.engine != VRQ_LARGE_ENGINE_VALU) || p.nchunks < 1 || p.nchunks > kLargeMaxChunks) return VRQ_EINVAL;
  if (mfma && (p.mb < 1 || p.chunk_rows % 64 != 0)) return VRQ_EINVAL;
  if (!(stages & kLargeStageAll)) stages |= kLargeStageAll;
  const int bins = cb * 8 + 1;
  const int want = (int64_t)K < n ? K : (int)n;
  for (int b0 = 0; b0 < nq; b0 += kLargeQueryBatch) {
    CountPassArgs a;
    a.codes = codes;
    a.n = n;
    a.q = q + (int64_t)b0 * cb;
    a.nq = nq - b0 < kLargeQueryBatch ? nq - b0 : kLargeQueryBatch;
    a.K = K;
    a.chunk_rows = p.chunk_rows;
    a.nchunks = p.nchunks;
    a.mb = p.mb;
    a.filter = filter;
    if (filter.query_set) a.filter.query_set = filter.query_set + b0;  // the pass's queries' sets
    a.hist = (uint32_t*)(ws + p.off_hist);
    a.prefix = (int32_t*)(ws + p.off_prefix) + (int64_t)b0 * p.nchunks * 4;
    a.tc = (int32_t*)(ws + p.off_tc) + (int64_t)b0 * 2;
    a.lists = (uint64_t*)(ws + p.off_lists) + (int64_t)b0 * K;
    int rc;
    if (stages & kLargeStageCount) {
      rc = mfma ? large_mfma_count_launch(cb, a, s) : large_count_launch(cb, a, s);
      if (rc != VRQ_OK) return rc;
    }
    if (stages & kLargeStageThreshold) {
      rc = large_threshold_launch(a.hist, a.nq, p.nchunks, bins, want, K, filter.allow != nullptr, a.tc, a.prefix, a.lists, s);
      if (rc != VRQ_OK) return rc;
    }
    if (stages & kLargeStageEmit) {
      rc = mfma ? large_mfma_emit_launch(cb, a, s) : large_emit_launch(cb, a, s);
      if (rc != VRQ_OK) return rc;
    }
  }
  return VRQ_OK;
}

}  // namespace vrq
