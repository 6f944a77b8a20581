// vrq_scan.h -- host-side plan of the Phase-I scan (K1) shared by the C ABI entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/vrq.h"

namespace vrq {

// Waves the scan aims to launch (256 CUs x 16): enough to fill every SIMD several
// times over.  A constant (not a device query) so workspace sizes are pure
// functions of the call shape.
constexpr int64_t kTargetWaves = 4096;
// A chunk emits K candidate keys; >= 4096 rows keeps that output < 0.2 % of the
// bytes the chunk scans (K = 100, 128-byte codes).
constexpr int64_t kMinChunkRows = 4096;

struct ScanPlan {
  int cap;             // per-query LDS candidate capacity (pow2 >= K + 64)
  int qg;              // queries per wave (resident in SGPRs)
  int wpg;             // waves per workgroup (share one LDS tile ring)
  int nqg;             // query groups
  int64_t chunk_rows;  // rows per wave (multiple of 64, <= 2^20)
  int nchunks;
  size_t list_bytes;   // nq * nchunks * K * 8
};

int scan_plan(int64_t n, int cb, int nq, int K, ScanPlan* p);
int scan_launch(const ScanPlan& p, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                uint64_t* lists, hipStream_t s);

// ---- K1d: the wavefront scan for the other code sizes (search_dim.hip); scan_plan / scan_launch
// dispatch to it for cb != 128 (one wave per workgroup: wpg = 1, qg fixed per code size) ----
bool dim_code_bytes_supported(int cb);   // 32, 48, 64, 96, 192, 256
int dim_scan_queries_per_wave(int cb);
int dim_scan_launch(const ScanPlan& p, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                    uint64_t* lists, hipStream_t s);

// ---- K1m: matrix-core scan for large query batches (hamming_mfma.hip) ----
constexpr int kMfmaMaxK = 128;           // K bound of the path
// the minimum dense sample (VRQ_MIN_SAMPLE: A/B builds).  Round 6: 65 536 rows; with the round-6 suffix and
// finish a looser tau_s costs less than the sample rows it saves (config 2: step 0.459-0.468 -> 0.445-0.450 ms,
// sample pass 0.075 -> 0.048 ms, matrix pass +0.007 ms; profiles/r6_c2_min_sample_ab.jsonl)
#ifndef VRQ_MIN_SAMPLE
#define VRQ_MIN_SAMPLE 65536
#endif
constexpr int64_t kMfmaMinSample = VRQ_MIN_SAMPLE;
constexpr int64_t kMfmaMaxSample = 1 << 20;   // dense-sample cap (1M rows: ~0.3 ms of MFMA at nq = 1024)
constexpr int64_t kMfmaMinRows = 65536;  // below this the wavefront scan is used
constexpr int kMfmaMinQueries = 1;       // auto-selection threshold on the batch size (K1r below 129)
// dense threshold sample = n / kMfmaSampleDiv rows (clamped above).  Per-step time at nq = 1024
// (profiles/r3_c4_shard_sample_div.txt): 12.5M rows (one rank of 8) div 16 / 32 / 64 / 128 = 4.31 /
// 4.22 / 4.23 / 4.32 ms, 25M rows 8.00 / 7.96 / 7.90 / 8.11 ms; 100M and 1M rows are at the clamps
constexpr int64_t kMfmaSampleDiv = 32;

struct MfmaPlan {
  int64_t sample;            // dense sample rows (sample_chunks * sample_chunk_rows)
  int64_t dvcols;            // dv columns per query: 32 lane minima per sample chunk
  int64_t sample_chunk_rows;
  int64_t sample_stride;     // sample chunk c starts at row c * sample_stride
  int64_t sample_tile_stride;  // rows between consecutive sample tiles (>= 64)
  int sample_chunks;
  int j;                     // sampled threshold order (tau_s = d_(j) + 1); K = tau_p only
  int capc;                  // candidate capacity per (query, chunk) list
  int rows;                  // 1: the row-split small-batch kernel K1r (nq <= 128, nqb = 1)
  int swap;                  // the large-batch pass runs K1s (row sets resident) instead of K1m (MB = 4):
                             // 1 = K1s<2, 8> (two waves per SIMD), 2 = K1s<4, 4> (one wave per SIMD)
  int rows_sample;           // 1: K1r also runs the dense sample pass (MB <= 2, nq <= 64)
  int mb;                    // M-blocks (32 queries) per wave of the matrix kernel: 4 or 2 (K1r: 1, 2 (lean), 4)
  int qpb;                   // queries per workgroup (128 * mb)
  int nqb;                   // query blocks of the thresholded pass
  int nqb_s;                 // query blocks of the dense sample pass (always the MB = 2 kernel)
  int64_t chunk_rows;        // rows per workgroup of the thresholded pass (multiple of 64)
  int nchunks;
  size_t off_suffix, off_cand, off_cnt, off_tau, bytes;
};

int mfma_plan(int64_t n, int nq, int K, MfmaPlan* p);
bool mfma_use(int64_t n, int nq, int K, int flags);
int mfma_scan_launch(const MfmaPlan& p, const uint8_t* codes, int64_t n, const uint8_t* q, int nq, int K,
                     uint8_t* ws, hipStream_t s, int flags);

// ---- what the matrix-core scans of every code size share (mfma_threshold.hip): the tail of a plan, the
// view of its workspace, and the launches of the threshold, recheck and suffix stages (cb: code bytes) ----
int mfma_sample_order(double lam, int K);  // the sampled order j an iid corpus proves with probability 1 - 1e-6
// capc, j, the workspace offsets and bytes, from the chunk_rows, nchunks, nqb, sample and dvcols already filled in
void mfma_plan_lists(MfmaPlan* p, int64_t n, int nq, int K);
struct MfmaWorkspace {  // the arrays of a plan's workspace
  uint16_t* dv;         // [nq][dvcols] lane minima of the dense sample pass
  uint64_t *suffix, *cand;  // sorted K-lists [nq][K]; candidate lists [nq][nchunks][capc]
  int32_t *ccnt, *tau_s, *tau_p, *rerun, *qbflag;  // list lengths [nq][nchunks]; [nq] each; [nqb]
  MfmaWorkspace(const MfmaPlan& p, uint8_t* ws, int nq) {
    const size_t qa = ((size_t)nq * sizeof(int32_t) + 255) & ~size_t(255);
    dv = (uint16_t*)ws;
    suffix = (uint64_t*)(ws + p.off_suffix);
    cand = (uint64_t*)(ws + p.off_cand);
    ccnt = (int32_t*)(ws + p.off_cnt);
    tau_s = (int32_t*)(ws + p.off_tau);
    tau_p = (int32_t*)(ws + p.off_tau + qa);
    rerun = (int32_t*)(ws + p.off_tau + 2 * qa);
    qbflag = (int32_t*)(ws + p.off_tau + 3 * qa);
  }
};
int mfma_sample_select_launch(const MfmaPlan& p, const MfmaWorkspace& w, const uint8_t* q, int cb, int nq, int K,
                              hipStream_t s);
int mfma_sample_check_launch(const MfmaPlan& p, const MfmaWorkspace& w, int nq, int K, hipStream_t s);
int mfma_suffix_launch(const MfmaPlan& p, const MfmaWorkspace& w, const uint8_t* codes, int64_t n, int cb,
                       const uint8_t* q, int nq, int K, hipStream_t s);

// ---- K1rd: the row-split matrix-core scan for the other code sizes (hamming_mfma_dim.hip): cb = 32, 48,
// 64, 96, 192, 256.  Same four stages, same workspace layout and the same constants as the 1024-bit scan;
// an MfmaPlan with rows = rows_sample = 1, mb M-blocks per wave and nqb = ceil(nq / (32 mb)) query blocks
// (the dense sample pass runs min(mb, 2) M-blocks per wave in nqb_s blocks).  Keys carry
// (dist - tau + dim + 1) << 40 | row, the u16 lane minima dist - pc(q) + dim. ----
constexpr int kMfmaKindRowsDim = 3;      // info[0] of vrq_scan_plan
int mfma_dim_min_queries(int cb);        // the measured default threshold (INT32_MAX: forced only)
int mfma_dim_plan(int64_t n, int cb, int nq, int K, MfmaPlan* p);
bool mfma_dim_use(int64_t n, int cb, int nq, int K, int flags);
int mfma_dim_scan_launch(const MfmaPlan& p, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                         uint8_t* ws, hipStream_t s, int flags);

// ---- the Phase-I route (scan_route.hip): which of the scans above runs for a call shape, its plan, the
// workspace it needs and where it leaves its lists.  Every search entry point takes its scan from here;
// nothing else calls mfma_use / mfma_dim_use or the three planners. ----
constexpr int KMAX = 1024;          // max K (binary_k) handled per query
constexpr int MAX_LISTS = 4096;     // max chunk lists merged per query (select_rescore.hip)

struct Phase1Route {
  bool mfma;         // a matrix-core scan (K1m / K1s / K1r at 128 code bytes, K1rd otherwise)
  ScanPlan sp;       // valid when !mfma
  MfmaPlan mp;       // valid when mfma
  size_t bytes;      // workspace this route needs
  size_t off_lists;  // where the finish finds the lists [nq][nl][K] in the workspace (0, or mp.off_suffix)
  int nl;            // lists per query (sp.nchunks, or 1)
  bool sorted;       // the single list is already the exact top-K in (dist, row) order, KEY_NONE padded
};
// VRQ_EINVAL for an empty shape, VRQ_EUNSUPPORTED where no scan serves it (code size, K, more than
// MAX_LISTS chunk lists).  flags: VRQ_SEARCH_SCAN_VALU / VRQ_SEARCH_SCAN_MFMA force a scan, the rest is ignored.
int phase1_route(int64_t n, int cb, int nq, int K, int flags, Phase1Route* r);
// runs the route's scan (flags: the VRQ_SCAN_STAGE_* bits of a matrix-core scan)
int phase1_launch(const Phase1Route& r, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                  void* ws, hipStream_t s, int flags);
// the largest `bytes` of the routes any flags can select (a pure function of the shape); 0: no route
size_t phase1_workspace_bytes(int64_t n, int cb, int nq, int K);

// ---- K1h: the counting scan for K up to VRQ_K_LARGE_MAX (hamming_count.hip).  Distances are integers in
// [0, dim]: per-(query, chunk) histograms -> per-query threshold T and c_lt = count(dist < T) -> a second
// pass that writes every row below T and the first K - c_lt rows at T, in row order, at positions that
// the chunk prefixes fix.  K1hm (hamming_count_mfma.hip) is the count and the emit stage again on the matrix
// cores; the threshold stage is shared.  The plan, the choice of the engine and the loop over passes and
// stages are the counting-scan route's (below); an engine file exports the count and the emit stage of one
// pass, and the measured tables the plan reads. ----
constexpr int kLargeMaxChunks = 1024;          // chunk prefixes of the threshold stage live in LDS
constexpr int64_t kLargeHistBytes = 64 << 20;  // cap of the per-chunk histograms of one query batch
constexpr int kLargeQueryBatch = 512;          // queries per pass of the scan (bounds the histograms)

// cb -> f(std::integral_constant<int, cb>) for the code sizes the counting scan has instances of
template <class F>
int count_code_bytes(int cb, F&& f) {
  switch (cb) {
    case 32: return f(std::integral_constant<int, 32>{});
    case 48: return f(std::integral_constant<int, 48>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 96: return f(std::integral_constant<int, 96>{});
    case 128: return f(std::integral_constant<int, 128>{});
    case 192: return f(std::integral_constant<int, 192>{});
    case 256: return f(std::integral_constant<int, 256>{});
    default: return VRQ_EUNSUPPORTED;
  }
}

// The row filter of a counting scan.  allow == null: none.  query_set == null: the one bitmap `allow`, u64
// [ceil(n / 64)], bit r & 63 of word r >> 6: row r takes part (nsets and set_words are not read).  Otherwise
// `allow` holds nsets such bitmaps, bitmap s at allow + s * set_words (set_words >= ceil(n / 64)), and query q
// is filtered by bitmap query_set[q] (device i32 [nq]): -1 allows every row, any other value outside
// [0, nsets) allows none.
struct RowFilter {
  const uint64_t* allow = nullptr;
  int nsets = 0;
  int64_t set_words = 0;
  const int32_t* query_set = nullptr;
};
// filter -> f(std::integral_constant<int, FILTER_*>) (row_filter.h: 0 off, 1 one bitmap, 2 per-query sets)
template <class F>
int filter_kind(const RowFilter& r, F&& f) {
  if (!r.allow) return f(std::integral_constant<int, 0>{});
  if (!r.query_set) return f(std::integral_constant<int, 1>{});
  return f(std::integral_constant<int, 2>{});
}

// one pass (at most kLargeQueryBatch queries) of either engine: the pointers are the pass's own slices
struct CountPassArgs {
  const uint8_t* codes;
  int64_t n;
  const uint8_t* q;
  int nq, K;
  int64_t chunk_rows;
  int nchunks;
  int mb;                 // K1hm: M-blocks per wave
  RowFilter filter;       // query_set is the pass's own slice
  uint32_t* hist;
  int32_t* tc;
  int32_t* prefix;
  uint64_t* lists;
};
// K1h: queries and waves per workgroup of the count kernel, and its two stages
int large_qg_of(int cb);
int large_waves_of(int cb);
int large_count_launch(int cb, const CountPassArgs& a, hipStream_t s);
int large_emit_launch(int cb, const CountPassArgs& a, hipStream_t s);
// the threshold stage of a pass, shared by K1h and K1hm
int large_threshold_launch(const uint32_t* hist, int nq, int nchunks, int bins, int want, int K, bool filtered,
                           int32_t* tc, int32_t* prefix, uint64_t* lists, hipStream_t s);
// K1hm: the measured AUTO threshold (INT32_MAX: forced only; one entry per code size, valid with and without a
// bitmap), M-blocks per wave for a pass of qb queries, real queries of an M-block, the rows a count workgroup
// scans between two flushes of its u16 bins, and its two stages
int large_mfma_min_queries(int cb);
int large_mfma_mb_of(int cb, int qb);
int large_mfma_qreal_of(int cb);
int64_t large_mfma_flush_rows();
int large_mfma_count_launch(int cb, const CountPassArgs& a, hipStream_t s);
int large_mfma_emit_launch(int cb, const CountPassArgs& a, hipStream_t s);

// ---- the counting-scan route (count_route.hip): the plan of either engine, the choice between them, the
// workspace a call needs and the one loop over passes and stages.  The vrq_*_large, vrq_*_filtered, vrq_*_batch
// and sharded *_large entry points (select_rescore.hip) all take their scan from here. ----
struct CountPlan {
  int engine;           // VRQ_LARGE_ENGINE_VALU (K1h) or VRQ_LARGE_ENGINE_MFMA (K1hm): the one that runs
  int qpw;              // queries per workgroup of the count kernel (K1hm: per wave: 32 mb, 16 at 256 code bytes)
  int mb;               // K1hm: M-blocks per wave (K1h: 0)
  int nqb;              // query blocks of a full pass of the count kernel
  int passes;           // passes of at most kLargeQueryBatch queries
  int64_t chunk_rows;   // multiple of 64, <= 2^30
  int nchunks;
  int64_t flush_rows;   // K1hm: rows between two flushes of a count workgroup's bins; 0: it never flushes
  // workspace: histograms u32 [qb][chunks][dim + 1] and chunk prefixes i32 [nq][nchunks][4] (the counts
  // region), T / c_lt pairs i32 [nq][2], K-lists u64 [nq][K], then the
  // finish's scratch: s2 f64 [nq][K], s3 f64 [nq][K], Phase-II order i32 [nq][K], candidates i32 [nq]
  size_t off_hist, off_prefix, off_tc, off_lists, off_s2, off_s3, off_ord, off_kp, bytes;
  size_t need;          // bytes the call's workspace must hold: `bytes`, or the larger of the two engines'
};
// engine: VRQ_LARGE_ENGINE_*; AUTO is resolved.  either: the workspace must cover either engine (a *_batch
// call); a *_large / *_filtered call is engine VALU with K1h's own bytes.  VRQ_EINVAL for an engine outside
// them or an empty shape, VRQ_EUNSUPPORTED for a code size or K outside the path or n >= 2^32
int count_route(int64_t n, int cb, int nq, int K, int engine, bool either, CountPlan* p);
// the whole scan (count, threshold, emit): leaves the K-lists at off_lists, KEY_NONE padded, the
// dist < T part and the dist == T part each in row order.  stages: a mask of kLargeStage* (none = all).
// filter: the row filter (above); the lists of a query then hold its min(K, allowed) smallest allowed rows.
constexpr int kLargeStageCount = VRQ_LARGE_STAGE_COUNT, kLargeStageThreshold = VRQ_LARGE_STAGE_THRESHOLD,
              kLargeStageEmit = VRQ_LARGE_STAGE_EMIT,
              kLargeStageAll = kLargeStageCount | kLargeStageThreshold | kLargeStageEmit;
int count_route_launch(const CountPlan& p, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                       uint8_t* ws, hipStream_t s, int stages, const RowFilter& filter);

}  // namespace vrq
