/*
 * vrq.h -- C ABI of libvrq.so, the MI355X (gfx950) hot path of
 * aitrailblazer/VectorRAGQuantization re-built as hand-written HIP kernels.
 *
 * The reference reaches its compute through two un-vendored native
 * dependencies (FAISS C++ for Phase I, NumPy for Phases II/III and the
 * encoders).  Each entry point below replaces one of those call sites; the
 * reference location is cited per function (paths relative to the reference
 * checkout).  The Python host layer (vectorragquantization_amd) binds these
 * symbols with ctypes; the cgo / JNI / ctypes stubs a maintainer would add on
 * the reference side are in INTEGRATION.md.
 *
 * Conventions (all functions):
 *   - every pointer is a DEVICE pointer owned by the caller (allocated e.g. by
 *     torch); the library never allocates, frees or synchronises;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*, NULL =
 *     the null stream) and is stream-ordered; no host threads, no global
 *     mutable state, so concurrent calls on different streams are safe;
 *   - return VRQ_OK (0) or a negative VRQ_E* code; never abort, never throw;
 *     vrq_strerror() maps a code to text.
 *   - row indices are int64; "rows" are internal (insertion-order) indices of
 *     the caller's shard, reported as row_offset + local row (global row).
 */
#ifndef VRQ_H_
#define VRQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRQ_ABI_VERSION 1

#define VRQ_OK 0
#define VRQ_EINVAL (-1)       /* bad argument (null pointer, negative size, ...) */
#define VRQ_EHIP (-2)         /* a HIP runtime call or kernel launch failed */
#define VRQ_EUNSUPPORTED (-3) /* shape outside what the kernels implement */
#define VRQ_EWORKSPACE (-4)   /* workspace smaller than *_workspace_size() */

/* flags for vrq_search3 */
#define VRQ_SEARCH_PHASE1_ONLY 1 /* stop after Phase I (FAISS IndexBinaryFlat::search) */
#define VRQ_SEARCH_SHARD 2       /* sharded mode: return all K Phase-I candidates in
                                    (dist,row) order with Phase-II AND Phase-III
                                    scores, no Phase II/III sort (merged later by
                                    vrq_merge_shards) */
#define VRQ_SEARCH_SCAN_VALU 4   /* Phase-I scan: force the wavefront popcount scan */
#define VRQ_SEARCH_SCAN_MFMA 8   /* Phase-I scan: force the matrix-core scan wherever it is
                                    supported (K <= 128, n >= 65536); by default it is used for
                                    nq >= 128.  Both scans give identical results. */
/* vrq_search3_scan only, matrix-core scan only: run a subset of its four stages (none set =
 * all), so a caller can bracket each stage with events; issuing PREFIX, MATRIX, RECHECK,
 * SUFFIX in that order on one stream is exactly the full scan. */
#define VRQ_SCAN_STAGE_PREFIX 16 /* dense matrix-core pass over a spread row sample -> per-query
                                    thresholds (sampled d_(j), guaranteed d_(K)) */
#define VRQ_SCAN_STAGE_MATRIX 32 /* thresholded matrix-core pass over all rows */
#define VRQ_SCAN_STAGE_RECHECK 128 /* per-query proof that the sampled threshold admitted >= K rows
                                      and exact re-run of the rare failed query blocks */
#define VRQ_SCAN_STAGE_SUFFIX 64 /* candidates -> one sorted K-list per query (exact rescan on
                                    list overflow) */

/* encoder modes for vrq_encode.  Inputs must be finite: the reference's NumPy encoders give NaN
 * min/max, NaN means and platform-defined integer casts for a NaN element, so no NaN behaviour is
 * pinned; the d = 1024 kernels fold min/max with v_med3 (a NaN element yields min = -inf, i.e. an
 * all-zero local code) and the generic kernel with fminf/fmaxf (NaN elements ignored). */
#define VRQ_ENC_INT8_GLOBAL 0  /* VectorDBInt8Global._quantize_to_int8 + _to_binary */
#define VRQ_ENC_INT16_GLOBAL 1 /* VectorDBInt16Global._quantize_to_int16 + _to_binary */
#define VRQ_ENC_INT4_GLOBAL 2  /* VectorDBInt4Global._quantize_to_int4 (limit ignored) + _to_binary */
#define VRQ_ENC_INT8_LOCAL 3   /* VectorDBInt8._quantize_to_int8 (+min/max) + _to_binary */
#define VRQ_ENC_INT4_LOCAL 4   /* VectorDBInt4._quantize_to_int4 (+min/max) + _to_binary */
#define VRQ_ENC_BIN_INT16 5    /* VectorDBInt16._to_binary on int16 input */
#define VRQ_ENC_COHERE 6       /* synthetic Cohere provider: int8 (global limit) + ubinary = packbits(x > 0) */
#define VRQ_ENC_SIGNED_BINARY 7 /* CohereVectorDBBinary._to_signed_binary + _pack_signed_binary
                                   (CohereVectorDBBinary.py:133-150): codes = packbits(x >= mean(x)) -- the
                                   only mode that keeps the elements equal to the float32 mean (a constant
                                   row encodes to all ones); codes only: q, minmax and limit are unused */
/* vrq_rescore_dequant only: the compare_float32 branch of the VectorDB* searches
 * (VectorDBInt8Global.py:239-240, VectorDBInt8.py:231-232, VectorDBInt4.py:262-263,
 * VectorDBInt16Global.py:240-241, VectorDBInt4Global.py:257-258): q = f32[n, dim] float rows */
#define VRQ_RESCORE_F32 16
/* vrq_rescore_dequant / vrq_search2 only: CohereVectorDBBinary._unpack_signed_binary
 * (CohereVectorDBBinary.py:152-159, rescoring at :231-232): q = u8[n, dim/8] packed sign codes, row
 * element i = +1.0f if bit i (MSB-first) is set, else -1.0f; minmax and limit ignored; dim % 128 == 0 */
#define VRQ_RESCORE_SIGNED_BINARY 17

int vrq_abi_version(void);
const char* vrq_strerror(int code);

/* ---------------------------------------------------------------------------
 * Phase I -- exhaustive Hamming k-NN over packed codes.
 * Replaces faiss.IndexBinaryFlat::search (hammings_knn_hc) reached from
 *   CohereEnhancedVectorDB.py:267-268 (and VectorDBInt8Global.py:224-225,
 *   VectorDBInt16.py, VectorDBInt4*.py, VectorDBInt16Global.py search()).
 * codes      u8[n, code_bytes]    (code_bytes = d/8; 128 for d = 1024)
 * queries    u8[nq, code_bytes]
 * out_dist   i32[nq, k]  ascending (dist, row) -- FAISS order; missing = INT32_MAX
 * out_rows   i64[nq, k]  row_offset + row; missing = -1
 * Supported: code_bytes in {32, 48, 64, 96, 128, 192, 256} (d = 256, 384, 512, 768, 1024, 1536,
 * 2048), 1 <= k <= 1024, n <= 2^32.  Every code size has a matrix-core scan (k <= 128, n >= 65536); it is
 * chosen by shape, see vrq_scan_kind.
 * ------------------------------------------------------------------------- */
size_t vrq_hamming_topk_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k);
int vrq_hamming_topk(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                     const uint8_t* queries, int32_t nq, int32_t k, int32_t* out_dist,
                     int64_t* out_rows, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Fused three-phase search -- replaces CohereEnhancedVectorDB.search
 *   (CohereEnhancedVectorDB.py:247-322) for a batch of nq queries:
 *   Phase I   top-K by Hamming (K = binary_k = min(k*binary_oversample, ntotal), :267-275)
 *   Phase II  s2 = q . (2*unpackbits(code)-1) in float64 (:283-293); stable sort desc (:296)
 *   Phase III s3 = float(q . int8 [f32]) / ||int8||_2 [f64], -inf if 0 (:302-318);
 *             over the first K3 = k*int8_oversample (:297); stable sort desc; first k (:321-322)
 * x8     int8[n, dim]   (the RocksDict "int8" value, :221)
 * norms  f64[n]         ||x8 row||_2 (vrq_int8_row_norms), as np.linalg.norm (:308)
 * rescore_row  i64[n] or NULL: row whose code/int8 Phases II/III use for Phase-I row r.
 *        IndexBinaryIDMap2::reconstruct(id) returns the row of the LAST add of an id
 *        (rev_map, :286) and the doc store keeps the last value (:221,303); when an id
 *        occurs on several rows pass rev_map[id_map[r]], else NULL (identity).
 * qf     f32[nq, dim], qb u8[nq, dim/8]
 * outputs [nq, kout] where kout = k (or K with VRQ_SEARCH_SHARD):
 *   out_count i32[nq]; out_rows i64; out_dist i32; out_binary f64; out_cosine f64
 * dim must be 1024 (code_bytes 128) in this ABI version.
 *
 * Score accuracy, every entry point of this header.  The products q_i * w_i (w = +-1, int8 or float32)
 * are exact in float64 and are summed in float64; the ORDER of the sum differs between entry points (one
 * wave per row and a butterfly in vrq_rescore_*, the *_large calls, vrq_gemm_topk and the exhaustive scan;
 * nibble tables, one row per lane, in the fused finish of vrq_search3 / _dim / vrq_shard_search3; one row
 * per lane in K5d).  Hence:
 *   - When all non-zero |q_i| are multiples of some 2^g and wmax * sum|q_i| < 2^(g+53) (wmax = 1 for Phase
 *     II, 128 for Phase III; at dim 1024 any float32 query whose non-zero coordinates lie within about 2^20
 *     of each other in magnitude, 2^12 for Phase III), every partial sum is exact: s2 is THE exact dot, the float32 dot of Phase III / flat IP
 *     its one correct rounding, and all entry points return identical bits.  "bit-identical" / "bit for
 *     bit" statements about scores below are made under this condition.
 *   - Otherwise each float64 sum is within gamma_(dim-1) * sum|q_i w_i| of the exact dot (gamma_m =
 *     m u / (1 - m u), u = 2^-53), in whatever order: entry points with different orders may differ in the
 *     last bits of s2 (and a Phase-II cut or a tie order may then fall differently), and the float32 dot is
 *     one of the at most two float32 neighbours of the exact dot within that bound.  Entry points that
 *     share an order stay bit-identical: the shard form and the fused finish; the *_large calls and
 *     vrq_rescore_*_dim; the _dim forwarders and the ABI-1 calls at 1024.
 *   tests/test_gpu_exact_scores.py checks both against exact rational arithmetic.
 * ------------------------------------------------------------------------- */
size_t vrq_search3_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search3(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq, int32_t k,
                int32_t K, int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows,
                int32_t* out_dist, double* out_binary, double* out_cosine, void* workspace,
                size_t workspace_bytes, void* stream);

/* The two launches vrq_search3 is made of, for callers that time or overlap them:
 * vrq_search3_scan   -- K1, the Phase-I scan: per-chunk exact top-K lists into `workspace`
 * vrq_search3_finish -- K2, exact merge of those lists + Phases II/III + the sorts
 * (same arguments as vrq_search3, the same flags to both; the workspace carries the lists
 * between them). */
int vrq_search3_scan(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq,
                     int32_t K, int32_t flags, void* workspace, size_t workspace_bytes, void* stream);
int vrq_search3_finish(const uint8_t* codes, const int8_t* x8, const double* norms,
                       const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset,
                       const float* qf, int32_t nq, int32_t k, int32_t K, int32_t K3, int32_t flags,
                       int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_binary,
                       double* out_cosine, const void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The same search at the other embedding dims (additive to ABI version 1; the functions above keep
 * their "dim must be 1024" contract).
 * vrq_dim_supported: 1 for dim in {256, 384, 512, 768, 1024, 1536, 2048}, else 0 (host-only; the
 *   source of truth for the functions below, which return VRQ_EUNSUPPORTED for every other dim).
 * vrq_search3_dim / vrq_search3_dim_workspace_size: the arguments and semantics of vrq_search3 /
 *   vrq_search3_workspace_size.  At dim == 1024 they forward to them (identical results and
 *   workspace size, every flag).  At the other dims: flags 0 and VRQ_SEARCH_PHASE1_ONLY; the Phase-I
 *   scan is chosen by shape (vrq_scan_kind tells which) and VRQ_SEARCH_SCAN_VALU forces the wavefront
 *   scan (identical results); VRQ_SEARCH_SCAN_MFMA, VRQ_SCAN_STAGE_* and VRQ_SEARCH_SHARD return
 *   VRQ_EUNSUPPORTED here: forcing and staging the matrix-core scan go through the pair below.
 * vrq_search3_dim_scan / vrq_search3_dim_finish: the two launches vrq_search3_dim is made of, with the
 *   arguments of vrq_search3_scan / vrq_search3_finish (the same flags to both).  At dim == 1024 they
 *   forward.  At the other dims they accept VRQ_SEARCH_PHASE1_ONLY, VRQ_SEARCH_SCAN_VALU,
 *   VRQ_SEARCH_SCAN_MFMA (the row-split matrix-core scan K1rd, for K <= 128 and n >= 65536) and
 *   VRQ_SCAN_STAGE_*; VRQ_SEARCH_SHARD returns VRQ_EUNSUPPORTED.  The workspace size of
 *   vrq_search3_dim_workspace_size covers either scan.
 * vrq_rescore_binary_dim / vrq_rescore_int8_cosine_dim: the arguments of vrq_rescore_binary /
 *   vrq_rescore_int8_cosine; at 1024 they forward to them (bit-identical).
 * ------------------------------------------------------------------------- */
int vrq_dim_supported(int32_t dim);
size_t vrq_search3_dim_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search3_dim(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                    int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                    int32_t k, int32_t K, int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows,
                    int32_t* out_dist, double* out_binary, double* out_cosine, void* workspace,
                    size_t workspace_bytes, void* stream);
int vrq_search3_dim_scan(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq,
                         int32_t K, int32_t flags, void* workspace, size_t workspace_bytes, void* stream);
int vrq_search3_dim_finish(const uint8_t* codes, const int8_t* x8, const double* norms,
                           const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset,
                           const float* qf, int32_t nq, int32_t k, int32_t K, int32_t K3, int32_t flags,
                           int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_binary,
                           double* out_cosine, const void* workspace, size_t workspace_bytes, void* stream);
int vrq_rescore_binary_dim(const float* qf, int32_t nq, int32_t dim, const uint8_t* codes, int64_t n,
                           const int64_t* cand_rows, int32_t ncand, double* out, void* stream);
int vrq_rescore_int8_cosine_dim(const float* qf, int32_t nq, int32_t dim, const int8_t* x8,
                                const double* norms, int64_t n, const int64_t* cand_rows,
                                int32_t ncand, double* out, void* stream);

/* Which Phase-I scan vrq_search3 / vrq_search3_scan / vrq_hamming_topk (and the _dim entry points,
 * for every dim of vrq_dim_supported) would run for this shape and flags: VRQ_SCAN_KIND_VALU (wavefront popcount) or VRQ_SCAN_KIND_MFMA (matrix
 * core; *prefix_rows, if non-NULL, receives the rows scanned outside the thresholded
 * matrix-core pass: 0, or n for the wavefront scan), or a
 * negative VRQ_E* code for an unsupported shape.  Host-only, no device work. */
#define VRQ_SCAN_KIND_VALU 0
#define VRQ_SCAN_KIND_MFMA 1
int vrq_scan_kind(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t flags, int64_t* prefix_rows);
/* Host-only planning introspection of the matrix-core scan (no reference counterpart; tests and
 * tools): info i64[12] = row-split kernel K1r (1), shared-tile kernel K1m (0) or row-set kernel K1s (2,
 * large batches of short passes), M-blocks (32 queries) per wave (K1s: 4, its 512-query blocks), chunk rows, chunks, per-(query, chunk) list capacity, workspace offsets of
 * the candidate lists (u64 keys (v + 1025) << 40 | row, v = dist - tau), of the list lengths (i32
 * [nq][chunks]) and of tau_s / tau_p / rerun (i32 [nq] each, 256-B aligned), sample rows, sampled
 * order j, offset of the sorted K-lists, workspace bytes.  VRQ_EUNSUPPORTED when the shape takes the
 * wavefront scan.  At the other dims of vrq_dim_supported the fields keep their meaning: info[0] = 3, the
 * row-split kernel of the other code sizes (K1rd), info[1] its M-blocks per wave (the grid holds
 * ceil(nq / (32 info[1])) query blocks per chunk group); the key bias is dim + 1 (keys
 * (v + dim + 1) << 40 | row) where it is 1025 at 1024. */
int vrq_scan_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t flags, int64_t* info);
/* Host-only introspection of the matrix-core scan's dense sample pass (tests and tools): info i64[6]
 * = the row-split kernel runs it (1) or K1m's MB = 2 instance (0), sample chunks, rows per sample
 * chunk, rows between consecutive sample chunks, rows between consecutive 64-row sample tiles, and
 * the u16 lane-minimum columns per query at workspace offset 0 (32 per sample chunk: column
 * chunk * 32 + r = min over the chunk's tiles and both 32-row halves of tile row r of
 * dist - popcount(query), + 1024; + dim at the other dims, where info[0] is 1).  VRQ_EUNSUPPORTED when
 * the shape takes the wavefront scan. */
int vrq_scan_sample_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t flags, int64_t* info);

/* ---------------------------------------------------------------------------
 * Merge of per-shard candidate tuples after the RCCL all-gather (multi-GPU
 * row sharding; the reference is single-process, so this reproduces the
 * single-index semantics of CohereEnhancedVectorDB.py:267-322 exactly):
 *   global top-K by (dist, global row) -> stable sort by s2 desc -> first K3
 *   -> stable sort by s3 desc -> first k.
 * Inputs are the VRQ_SEARCH_SHARD / vrq_shard_search3 outputs of S shards stacked
 * [S, nq, K] (counts i32[S, nq]); shard s must own a contiguous global row range
 * below shard s+1's.  out_src (nullable) i32[nq, k] receives s*K + p, the position
 * of each result in the stacked inputs (to fetch per-candidate payloads such as
 * external ids).
 * The merge takes no dim and serves every dim of vrq_dim_supported: it orders
 * candidates by their (dist, row) keys, and every distance up to 2048 is covered.
 * Limits: K <= 1024, nshards <= 4096.
 * ------------------------------------------------------------------------- */
int vrq_merge_shards(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts,
                     const int64_t* rows, const int32_t* dist, const double* s2,
                     const double* s3, int32_t k, int32_t K3, int32_t* out_count,
                     int64_t* out_rows, int32_t* out_dist, double* out_binary,
                     double* out_cosine, int32_t* out_src, void* stream);

/* ---------------------------------------------------------------------------
 * Row-sharded search at every embedding dim and for the two-phase classes (additive to ABI version 1;
 * VRQ_SEARCH_SHARD keeps its "1024 only" contract on vrq_search3* and is still refused by vrq_search2*).
 * One process per GPU owns a contiguous global row range [row_offset, row_offset + n); each runs the
 * per-shard call with the GLOBAL K (the global top-K may sit in one shard), the outputs are all-gathered
 * and every rank runs the merge.
 * Both per-shard calls: outputs [nq, K] = the shard's exact Phase-I top-K in FAISS (dist, row) order, rows
 *   as row_offset + local row, every candidate with its score(s) and no sort by score;
 *   out_count i32[nq] = min(K, n); missing slots -1 / INT32_MAX / NaN.  flags: 0, VRQ_SEARCH_SCAN_VALU or
 *   VRQ_SEARCH_SCAN_MFMA as vrq_search3_dim_scan takes them (identical results on every scan); any other
 *   bit returns VRQ_EUNSUPPORTED.  Supported: every dim of vrq_dim_supported, K <= 1024.  Workspace:
 *   vrq_shard_search{3,2}_workspace_size = vrq_search3_dim_workspace_size.  n, K or nq = 0 behave as in
 *   vrq_search3_dim_finish with kout = K.  Every argument is checked before anything is launched.
 * vrq_shard_search3: the arguments of vrq_search3_dim without k and K3; out_binary = s2 and out_cosine = s3
 *   of all K candidates (the scores vrq_search3_dim gives the same rows, bit for bit).  At dim == 1024 it
 *   forwards to vrq_search3 with VRQ_SEARCH_SHARD (bit-identical); at the other dims it runs the scan
 *   vrq_search3_dim_scan runs for the shape and flags, then the shard mode of the runtime-dim finish.
 *   Merged by vrq_merge_shards.
 * vrq_shard_search2: the arguments of vrq_search2 without k; out_score = the vrq_rescore_dequant score of
 *   `mode` (every mode vrq_search2 accepts, VRQ_RESCORE_F32 and VRQ_RESCORE_SIGNED_BINARY included) of all
 *   K candidates, bit-identical to vrq_search2's.  Merged by vrq_merge_shards2.
 * vrq_merge_shards2: the merge of the stacked vrq_shard_search2 outputs [S, nq, K] (counts i32[S, nq];
 *   shard s owns a contiguous global row range below shard s+1's): global top-K by (dist, global row) ->
 *   stable sort by score descending over that order (-0.0 ties +0.0) -> first k, which is exactly the
 *   single-index semantics of CohereVectorDBBinary.py:215-239 / VectorDBInt8Global.py:224-252, so the
 *   result equals vrq_search2 over the whole corpus.  Outputs [nq, k]; out_count = min(k, candidates);
 *   out_src (nullable) i32[nq, k] = s*K + p as in vrq_merge_shards (missing -1).  Limits as there.
 * Not sharded: VRQ_ENC_BIN_INT16 (VectorDBInt16 ranks by Phase I alone); a rescore_row that points into
 *   another shard (an id added twice must live in one shard).
 * ------------------------------------------------------------------------- */
size_t vrq_shard_search3_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_shard_search3(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                      int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb,
                      int32_t nq, int32_t K, int32_t flags, int32_t* out_count, int64_t* out_rows,
                      int32_t* out_dist, double* out_binary, double* out_cosine,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t vrq_shard_search2_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_shard_search2(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                      const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                      const uint8_t* qb, int32_t nq, int32_t K, int32_t flags, int32_t* out_count,
                      int64_t* out_rows, int32_t* out_dist, double* out_score,
                      void* workspace, size_t workspace_bytes, void* stream);
int vrq_merge_shards2(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts, const int64_t* rows,
                      const int32_t* dist, const double* score, int32_t k, int32_t* out_count,
                      int64_t* out_rows, int32_t* out_dist, double* out_score, int32_t* out_src, void* stream);

/* ---------------------------------------------------------------------------
 * Stand-alone Phase II / Phase III candidate rescoring (the per-candidate
 * loops of CohereEnhancedVectorDB.py:283-293 and :302-318).
 * cand_rows i64[nq, ncand] local rows (negative = skip, output NaN).
 * ------------------------------------------------------------------------- */
int vrq_rescore_binary(const float* qf, int32_t nq, int32_t dim, const uint8_t* codes, int64_t n,
                       const int64_t* cand_rows, int32_t ncand, double* out, void* stream);
int vrq_rescore_int8_cosine(const float* qf, int32_t nq, int32_t dim, const int8_t* x8,
                            const double* norms, int64_t n, const int64_t* cand_rows,
                            int32_t ncand, double* out, void* stream);

/* ---------------------------------------------------------------------------
 * Encoders -- the VectorDBInt{4,8,16}{,Global} quantize + _to_binary path:
 *   VectorDBInt8Global.py:130-142,154-160   VectorDBInt16Global.py:130-142,154-160
 *   VectorDBInt4Global.py:129-164,190-196   VectorDBInt8.py:114-126,140-146
 *   VectorDBInt4.py:116-154,186-192          VectorDBInt16.py:148-157
 * x       f32[n, dim] (i16[n, dim] for VRQ_ENC_BIN_INT16)
 * codes   u8[n, dim/8]           packbits(x > mean(x)) MSB-first (x > 0 for COHERE, x >= mean(x) for
 *                                SIGNED_BINARY)
 * q       i8[n, dim] | i16[n, dim] | i8[n, (dim+1)/2] (int4 nibbles) | unused (BIN_INT16 and
 *         SIGNED_BINARY: may be NULL)
 * minmax  f64[n, 2] (local modes only; may be NULL otherwise)
 * limit   global clip limit (Global modes / COHERE), as passed by the caller
 * dim must be a multiple of 8 and <= 8192.
 * ------------------------------------------------------------------------- */
int vrq_encode(int32_t mode, const void* x, int64_t n, int32_t dim, double limit, uint8_t* codes,
               void* q, double* minmax, void* stream);

/* ---------------------------------------------------------------------------
 * Search side of the VectorDB* classes: dequantisation and the
 * dequantised-dot rescoring of Phase-I candidates.  mode is the VRQ_ENC_* mode that produced the
 * codes (INT8_GLOBAL, INT16_GLOBAL, INT4_GLOBAL, INT8_LOCAL, INT4_LOCAL):
 *   VectorDBInt8Global._dequantize_int8   VectorDBInt8Global.py:144-152
 *   VectorDBInt16Global._dequantize_int16 VectorDBInt16Global.py:144-152
 *   VectorDBInt4Global._dequantize_int4   VectorDBInt4Global.py:166-188
 *   VectorDBInt8._dequantize_int8         VectorDBInt8.py:129-138
 *   VectorDBInt4._dequantize_int4         VectorDBInt4.py:157-184
 * bit-identical to the reference (NumPy 2 scalar rules).  q is the code array (int8 / int16 /
 * packed int4 bytes), minmax f64[n, 2] for the local modes (NULL otherwise), limit for the global
 * ones.  vrq_dequantize writes f32[n, dim]; vrq_rescore_dequant writes, per (query, candidate), the
 * reference score float(np.dot(query_float, dequantised row)) (VectorDBInt8Global.py:232-238 and the
 * same loop in the other classes) as the correctly rounded float32 dot (NaN for negative rows).
 * vrq_rescore_dequant also takes mode VRQ_RESCORE_F32 (q = the f32 float rows, compare_float32) and
 * VRQ_RESCORE_SIGNED_BINARY (q = the packed sign codes; dim a multiple of 128, else VRQ_EUNSUPPORTED).
 * ------------------------------------------------------------------------- */
int vrq_dequantize(int32_t mode, const void* q, const double* minmax, int64_t n, int32_t dim, double limit,
                   float* out, void* stream);
int vrq_rescore_dequant(int32_t mode, const float* qf, int32_t nq, int32_t dim, const void* q,
                        const double* minmax, double limit, int64_t n, const int64_t* cand_rows,
                        int32_t ncand, double* out, void* stream);
/* ---------------------------------------------------------------------------
 * Fused two-phase search -- CohereVectorDBBinary.search (CohereVectorDBBinary.py:215-239) and the
 * identical loops of the VectorDBInt* classes (e.g. VectorDBInt8Global.py:224-252) for a batch of nq
 * queries, in two launches (scan + finish) instead of vrq_hamming_topk, a gather, vrq_rescore_dequant,
 * a sort and three more gathers:
 *   Phase I   top-K by Hamming over `codes` in FAISS (dist, row) order (K = min(k*binary_oversample,
 *             ntotal)): exactly the scan vrq_search3_dim_scan runs for the shape and flags
 *   Phase II  every candidate row r gets the vrq_rescore_dequant score of `mode` (any mode it accepts;
 *             q / minmax / limit as there) taken from row rescore_row[r] (r itself if NULL: see
 *             vrq_search3).  For VRQ_RESCORE_SIGNED_BINARY the caller normally passes q = codes.
 *   then      a stable sort by score descending over the Phase-I order (-0.0 ties +0.0), first k
 * outputs [nq, k]: out_rows i64 = row_offset + r (missing -1), out_dist i32 (missing INT32_MAX),
 *   out_score f64 (missing NaN); out_count i32[nq] = min(k, K, n).  Inputs must be finite.
 * Supported: every dim of vrq_dim_supported, 1 <= K <= 1024; n, K, k or nq = 0 behave as in
 * vrq_search3_dim_finish.  flags: 0, VRQ_SEARCH_SCAN_VALU, VRQ_SEARCH_SCAN_MFMA (as vrq_search3_dim_scan;
 * identical results); any other bit returns VRQ_EUNSUPPORTED.
 * vrq_search2 = vrq_search3_dim_scan + vrq_search2_finish with the same flags and workspace (size:
 * vrq_search2_workspace_size = vrq_search3_dim_workspace_size); the finish reads the lists the scan left
 * and needs no other scratch.
 * ------------------------------------------------------------------------- */
size_t vrq_search2_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search2(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, int32_t* out_count,
                int64_t* out_rows, int32_t* out_dist, double* out_score, void* workspace,
                size_t workspace_bytes, void* stream);
int vrq_search2_finish(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                       const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                       int32_t nq, int32_t k, int32_t K, int32_t flags, int32_t* out_count, int64_t* out_rows,
                       int32_t* out_dist, double* out_score, const void* workspace, size_t workspace_bytes,
                       void* stream);
/* np.linalg.norm(int8 row) in float64 (CohereEnhancedVectorDB.py:308), computed once at add time */
int vrq_int8_row_norms(const int8_t* x8, int64_t n, int32_t dim, double* out, void* stream);
/* ---------------------------------------------------------------------------
 * Exhaustive batched Phase-II / Phase-III scoring on the matrix cores (BASELINE config 5):
 * the per-candidate scores of CohereEnhancedVectorDB.py:283-293 (VRQ_GEMM_BINARY) or :302-318
 * (VRQ_GEMM_INT8_COSINE) evaluated against EVERY row, top-k fused (no nq x n score matrix):
 *   VRQ_GEMM_BINARY       s = float(q . (2*unpackbits(code)-1)) in float64      (codes)
 *   VRQ_GEMM_INT8_COSINE  s = float32(q . int8) / ||int8||_2, -inf if the norm is 0 (x8, norms)
 * out_rows i64[nq, k] / out_scores f64[nq, k]: the k rows with the largest s ordered (s desc,
 * row asc) -- the reference's stable sorted(..., reverse=True) (:296, :321) over rows in index
 * order -- as row_offset + row, with their exact scores (vrq_search3's: see "Score accuracy" above);
 * out_count i32[nq] = min(k, n); unused slots -1 / NaN.  Queries must be finite.
 * Exact for every input: int8-quantised queries on v_mfma_i32_32x32x32_i8 give scores within a
 * proven per-query bound, a sampled threshold keeps every row that can reach the top-k, and the
 * survivors are rescored exactly (heavy-tie inputs fall back to an exact scan of every row).
 * flags: 0, or a subset of the VRQ_GEMM_STAGE_* (issued in order SAMPLE, MAIN, FINISH on one
 * workspace = the full call; FINISH consumes the thresholds SAMPLE wrote, so every MAIN + FINISH
 * pair needs its own SAMPLE before it), optionally | VRQ_GEMM_NO_FALLBACK: queries the matrix
 * path could not serve (heavy exact ties) are left with out_count = -1 and unwritten rows instead
 * of taking the exact per-query scan of every row (callers that must bound latency; tests prove
 * with it that the matrix path alone served a batch).
 * Supported: dim = 1024, 1 <= k <= 1024, 1 <= n < 2^32.
 * ------------------------------------------------------------------------- */
#define VRQ_GEMM_BINARY 2
#define VRQ_GEMM_INT8_COSINE 3
#define VRQ_GEMM_STAGE_SAMPLE 16 /* query split + dense sample pass + per-query thresholds */
#define VRQ_GEMM_STAGE_MAIN 32   /* thresholded pass over every row -> candidate lists */
#define VRQ_GEMM_STAGE_FINISH 64 /* exact rescoring + sort of the candidates (+ exact fallback) */
#define VRQ_GEMM_NO_FALLBACK 128 /* skip the exact fallback: unserved queries get out_count = -1 */
size_t vrq_gemm_topk_workspace_size(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k);
/* int8 pieces per query of this build's matrix pass (1: q ~ S*a, 2: q ~ S*(a + b/256)); the
 * algorithmic ops of a pass are 2*nq*n*dim either way (for roofline reporting) */
int vrq_gemm_topk_pieces(void);
/* Host-only planning introspection (no reference counterpart; for tests and tools): the matrix
 * passes' plan of a vrq_gemm_topk / vrq_flat_ip_topk call shape.  info i64[8] = chunk rows, chunks,
 * per-(query, chunk) list capacity, query blocks, sample chunks, rows per sample chunk, workspace
 * bytes, queries per block.  VRQ_EUNSUPPORTED for shapes the path does not serve. */
int vrq_gemm_topk_plan(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info);
/* Host-only introspection of the workspace layout (tests checking the candidate lists a MAIN stage
 * leaves): info i64[8] = padded queries nq_pad; byte offsets of the per-query thresholds (f32
 * [nq_pad], u units), the list lengths (i32 [nq][chunks]), the lists (u32 rows [nq][chunks][capc]) and
 * the sample maxima (f32 [nq][cols]); sample columns per query, rows between sample chunks, rows per
 * sample chunk.  The int8 query pieces a (q/S = a + rho) sit at offset 0 as i8 [nq_pad][1024]: natural
 * dim order for VRQ_GEMM_INT8_COSINE, and within each 32-dim step the Phase-II k-permutation for
 * VRQ_GEMM_BINARY.  Hit rule of the MAIN pass: binary u = <a, bits> >= ceil(thr); cosine u =
 * f32(<a, x>) * (1 / f32(norm)) >= thr. */
int vrq_gemm_topk_layout(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info);
/* The rest of that layout (additive; tests checking what the SAMPLE stage's query split leaves): info
 * i64[4] = byte offsets of the per-query error bounds Delta (f64 [nq_pad], u units: |u - s'| <= Delta for
 * every row), of alpha and of beta (f64 [nq_pad] each: a reference score s is s' = alpha s + beta in u
 * units), and of the per-query flags the FINISH stage writes (i32 [nq]: 0 served, 2 retried, 1 left to
 * the exact fallback).  Delta in u units, with rho = q/S - a, S = max|q| / 127 and eps = 2^-20:
 *   VRQ_GEMM_BINARY       max(sum rho+, sum rho-) (1 + eps) + eps ||q/S||_1
 *   VRQ_GEMM_INT8_COSINE  ||rho||_2 (1 + eps) + eps ||q/S||_2
 *   VRQ_GEMM_FLOAT_IP     (||rho||_2 B0 + ||q/S||_2 B1) (1 + eps) + eps (||q/S||_2 + ||rho||_2) B0,
 *                         (B0, B1) = the corpus bounds of vrq_flat_ip_prepare
 * The SAMPLE stage sets thr = U - 2 Delta rounded down to f32, U = the k-th largest sample maximum. */
int vrq_gemm_topk_prep_layout(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info);
int vrq_gemm_topk(int32_t mode, const uint8_t* codes, const int8_t* x8, const double* norms, int64_t n,
                  int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t flags,
                  int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace,
                  size_t workspace_bytes, void* stream);
/* ---------------------------------------------------------------------------
 * Exact float inner-product top-k: CohereVectorDBFloat's faiss.IndexIDMap(faiss.IndexFlatIP(d))
 * (CohereVectorDBFloat.py:55-64) searched at :156, for a batch of queries, on the matrix cores.
 *   s = q . x in float32 (the exact products summed in float64, rounded once to float32)
 * out_* as vrq_gemm_topk: the k rows with the largest s ordered (s desc, row asc) -- FAISS's
 * IndexFlatIP result order, re-sorted stably by score at :170 -- as row_offset + row, scores f64
 * holding the float32 values.
 * vrq_flat_ip_prepare (once per added batch, rows [0, n) of the given pointers) derives the
 * matrix pass's operands from the float32 rows xf: x8 int8[n, dim] (per-row scaled), inv_scale
 * f64[n] and the running corpus bounds f64[2], which it max-accumulates (zero them before the first
 * batch; after removals the old bounds stay valid upper bounds).  vrq_flat_ip_topk: exact for every
 * input -- int8 queries x int8 rows on v_mfma_i32_32x32x32_i8 within a proven per-query bound, a
 * sampled threshold, exact rescoring of the survivors from xf (exact fallback on heavy ties).
 * Workspace: vrq_gemm_topk_workspace_size(VRQ_GEMM_FLOAT_IP, ...).  Supported: dim = 1024,
 * 1 <= k <= 1024, 1 <= n < 2^32, finite inputs.
 * ------------------------------------------------------------------------- */
#define VRQ_GEMM_FLOAT_IP 4
int vrq_flat_ip_prepare(const float* xf, int64_t n, int32_t dim, int8_t* x8, double* inv_scale, double* bounds,
                        void* stream);
int vrq_flat_ip_topk(const float* xf, const int8_t* x8, const double* inv_scale, const double* bounds, int64_t n,
                     int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t flags,
                     int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Exhaustive top-k and the exact float inner product at every supported embedding dim (additive to
 * ABI version 1; the functions above keep their "dim = 1024" contract).  The arguments, outputs and
 * result order of vrq_gemm_topk / vrq_flat_ip_topk / vrq_gemm_topk_workspace_size.
 * At dim == 1024 without VRQ_GEMM_SCAN_EXACT they forward to those functions (identical results,
 * workspace size and flags).  At the other dims of vrq_dim_supported, and at 1024 with
 * VRQ_GEMM_SCAN_EXACT, they run K5d, an exact scan that scores every (query, row) pair once in f64:
 * no matrix-core pass, no sampled threshold and no fallback, so no query is ever left unserved.
 * There: flags 0, VRQ_GEMM_SCAN_EXACT and VRQ_GEMM_NO_FALLBACK (a no-op); VRQ_GEMM_STAGE_* returns
 * VRQ_EUNSUPPORTED; vrq_flat_ip_topk_dim ignores x8, inv_scale and bounds (may be NULL; there is no
 * prepare step off 1024); mode VRQ_GEMM_FLOAT_IP passed to vrq_gemm_topk_dim returns VRQ_EINVAL.
 * Workspace: vrq_gemm_topk_dim_workspace_size; at 1024 that is the forwarded path's size, and a
 * caller that sets VRQ_GEMM_SCAN_EXACT there sizes the workspace as the maximum of it and the bytes
 * vrq_gemm_topk_dim_plan reports.  Supported: 1 <= k <= 1024, 1 <= n < 2^32, finite inputs.
 * vrq_gemm_topk_dim_plan (host-only; tests and tools): K5d's plan, info i64[6] = rows per tile, rows
 * per chunk, chunks, queries per workgroup, list capacity per (query, chunk), workspace bytes;
 * VRQ_EUNSUPPORTED for shapes K5d does not serve.
 * ------------------------------------------------------------------------- */
#define VRQ_GEMM_SCAN_EXACT 256 /* _dim entry points only: run the exact exhaustive scan (K5d) at
                                   dim == 1024 too, instead of forwarding */
size_t vrq_gemm_topk_dim_workspace_size(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k);
int vrq_gemm_topk_dim_plan(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info);
int vrq_gemm_topk_dim(int32_t mode, const uint8_t* codes, const int8_t* x8, const double* norms, int64_t n,
                      int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t flags,
                      int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace,
                      size_t workspace_bytes, void* stream);
int vrq_flat_ip_topk_dim(const float* xf, const int8_t* x8, const double* inv_scale, const double* bounds, int64_t n,
                         int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t flags,
                         int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Search with more than 1024 Phase-I candidates (additive to ABI version 1; every function above keeps
 * its K <= 1024 contract and its VRQ_EUNSUPPORTED beyond it).  FAISS IndexBinaryFlat::search takes any k,
 * and K = min(k * binary_oversample, ntotal) passes 1024 at k = 103 with the default oversample of 10.
 * vrq_hamming_topk_large / vrq_search3_large / vrq_search2_large: the arguments, outputs and semantics of
 *   vrq_hamming_topk / vrq_search3_dim / vrq_search2 -- Phase I = the K smallest rows by (dist, row), missing
 *   slots INT32_MAX / -1 / NaN; scores from rescore_row[r] when given; Phase II a stable sort by score
 *   descending over the Phase-I order (-0.0 ties +0.0); the three-phase call then takes the first
 *   min(K3, candidates), scores Phase III, sorts stably by it descending and keeps the first k; out_count =
 *   min(k, K, n), or min(K, n) with VRQ_SEARCH_PHASE1_ONLY -- with scores bit-identical to
 *   vrq_rescore_binary_dim / vrq_rescore_int8_cosine_dim / vrq_rescore_dequant for the same (query, row)
 *   (the same scorers: for every input).
 *   Supported: every dim of vrq_dim_supported, 1 <= K <= VRQ_K_LARGE_MAX, 0 <= k <= VRQ_K_LARGE_MAX, any
 *   K3 >= 0, 1 <= n < 2^32.  K <= 1024 is accepted on purpose: there every output equals the call above's,
 *   bit for bit, under the condition of "Score accuracy" (vrq_search3_dim sums Phase II by nibble tables:
 *   otherwise s2 may differ in its last bits, within the bound stated there; distances, Phase III scores of
 *   the same row and the two-phase scores are equal for every input).  flags: vrq_search3_large 0 or VRQ_SEARCH_PHASE1_ONLY, vrq_search2_large 0; any other bit
 *   returns VRQ_EUNSUPPORTED.  n, nq, K or k = 0 behave as in vrq_search3_dim_finish / vrq_search2 (counts 0,
 *   padding written, nothing scanned).  Every argument and the workspace size are checked before anything
 *   is launched.  Sharded through the vrq_shard_search*_large / vrq_merge_shards*_large calls below.
 * Phase I is the counting scan K1h: a Hamming distance is an integer in [0, dim], so per-(query, chunk)
 *   histograms give the threshold distance T with count(dist < T) < K <= count(dist <= T), and a second
 *   pass writes every row below T and the first K - count(dist < T) rows at T, in row order.  The finish
 *   sorts the K keys and the (score, rank) pairs in LDS; 8192 pairs take 96 KiB, hence VRQ_K_LARGE_MAX.
 * vrq_scan_large_plan (host-only; tests and tools): info i64[8] = rows per chunk (a multiple of 64), chunks,
 *   queries per workgroup of the count kernel, rows of the bounding prefix (always 0: the count adds every
 *   distance; a bound from a row prefix was measured and bought nothing), workspace offset of the
 *   per-(query, chunk) counts (histograms u32 [min(nq, 512)][chunks][dim + 1], then the chunk prefixes), of the per-query T / count(dist < T) pairs (i32 [nq][2]), of the K-lists (u64 dist << 40 | row,
 *   [nq][K], all-ones padded), and the workspace bytes = the three *_large_workspace_size (pure functions of
 *   the shape; 0 for an unsupported one).  VRQ_EINVAL for an empty shape or a null info, VRQ_EUNSUPPORTED as
 *   the search calls.
 * ------------------------------------------------------------------------- */
#define VRQ_K_LARGE_MAX 8192
/* vrq_scan_large: the Phase-I scan the three calls above start with, alone or a subset of its stages (for
 * callers that time them): `stages` = 0 (all) or a mask of VRQ_LARGE_STAGE_*; issuing COUNT, THRESHOLD, EMIT
 * in that order on one stream and workspace is exactly the full scan.  Leaves the K-lists at the plan's
 * offset (row order within the dist < T part and within the dist == T part, all-ones padded).  Shapes,
 * return codes and the workspace as the search calls; any other bit returns VRQ_EUNSUPPORTED; n, nq or
 * K = 0 returns VRQ_OK and does nothing. */
#define VRQ_LARGE_STAGE_COUNT 1      /* histograms of the distances per (query, chunk) over every row */
#define VRQ_LARGE_STAGE_THRESHOLD 2  /* per query: T, count(dist < T), the chunk prefixes, the list padding */
#define VRQ_LARGE_STAGE_EMIT 4       /* second pass: the rows of the K-lists at their final positions */
int vrq_scan_large(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                   int32_t stages, void* workspace, size_t workspace_bytes, void* stream);
size_t vrq_hamming_topk_large_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k);
int vrq_hamming_topk_large(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                           const uint8_t* queries, int32_t nq, int32_t k, int32_t* out_dist,
                           int64_t* out_rows, void* workspace, size_t workspace_bytes, void* stream);
size_t vrq_search3_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search3_large(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                      int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                      int32_t k, int32_t K, int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows,
                      int32_t* out_dist, double* out_binary, double* out_cosine, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t vrq_search2_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search2_large(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                      const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                      const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, int32_t* out_count,
                      int64_t* out_rows, int32_t* out_dist, double* out_score, void* workspace,
                      size_t workspace_bytes, void* stream);
int vrq_scan_large_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int64_t* info);

/* ---------------------------------------------------------------------------
 * Filtered search: a row allow-bitmap (additive to ABI version 1).  The nearest rows among a caller-chosen
 * subset of the index -- a tenant, a date range, a permission set, the hits of a keyword pre-filter -- without
 * copying that subset into an index of its own (FAISS: SearchParameters::sel = IDSelectorBitmap).
 * vrq_hamming_topk_filtered / vrq_search3_filtered / vrq_search2_filtered / vrq_scan_filtered: the arguments
 *   of vrq_hamming_topk_large / vrq_search3_large / vrq_search2_large / vrq_scan_large plus
 *   allow  device pointer to ceil(n / 64) little-endian u64 words, 8-byte aligned: row r takes part iff bit
 *          r & 63 of word r >> 6 is set (the bytes of FAISS's IDSelectorBitmap and of numpy's
 *          packbits(mask, bitorder="little")).  Bits at positions >= n of the last word are ignored.  One
 *          bitmap per call, shared by its queries; it is only read.
 *   Every output equals, bit for bit, that of the *_large call on the corpus with the disallowed rows removed
 *   in row order (the corpus remove_ids would leave), row numbers mapped back: Phase I = the min(K, allowed)
 *   smallest allowed rows by (dist, row), padding INT32_MAX / -1 / NaN; out_count = min(k, K, allowed), or
 *   min(K, allowed) with VRQ_SEARCH_PHASE1_ONLY.  rescore_row[r] keeps its meaning: the filter decides whether
 *   row r is a Phase-I candidate, its scores come from row rescore_row[r] whether or not that row is allowed.
 *   An all-ones bitmap gives the *_large outputs; with an all-zero one every count is 0 and every output
 *   padding.  Shapes, flags, return codes and the workspace (= the *_large one: the bitmap is the caller's)
 *   are those of the *_large calls -- any 1 <= K <= VRQ_K_LARGE_MAX at every dim of vrq_dim_supported,
 *   n < 2^32; n, nq, K or k = 0 behave as there (and read no bitmap).  A null or misaligned allow of a
 *   non-empty call returns VRQ_EINVAL; every argument is checked before anything is launched.
 * Only the counting scan K1h reads the bitmap (one word per 64-row tile, a scalar load): it serves every K,
 *   and is a VALU scan meant for small and medium batches (for big ones: the vrq_*_batch calls below).  A
 *   bitmap per query: the vrq_*_perquery calls further below.  There is no filtered sharded call.
 * ------------------------------------------------------------------------- */
size_t vrq_scan_filtered_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_scan_filtered(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                      int32_t stages, const uint64_t* allow, void* workspace, size_t workspace_bytes,
                      void* stream);
size_t vrq_hamming_topk_filtered_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k);
int vrq_hamming_topk_filtered(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                              const uint8_t* queries, int32_t nq, int32_t k, const uint64_t* allow,
                              int32_t* out_dist, int64_t* out_rows, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t vrq_search3_filtered_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search3_filtered(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                         int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                         int32_t k, int32_t K, int32_t K3, int32_t flags, const uint64_t* allow, int32_t* out_count,
                         int64_t* out_rows, int32_t* out_dist, double* out_binary, double* out_cosine,
                         void* workspace, size_t workspace_bytes, void* stream);
size_t vrq_search2_filtered_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search2_filtered(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                         const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                         const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, const uint64_t* allow,
                         int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_score,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The counting scan on the matrix cores: large-K and filtered search for big batches (additive to ABI
 * version 1).  K1hm (hamming_count_mfma.hip) runs the count and the emit stage of the counting scan on
 * v_mfma_f32_32x32x64_f8f6f4, at every dim of vrq_dim_supported, with and without the row bitmap; the
 * threshold stage and the finish are K1h's.  The *_large and *_filtered calls above keep running K1h.
 * vrq_hamming_topk_batch / vrq_search3_batch / vrq_search2_batch / vrq_scan_batch: the arguments of the
 *   *_filtered call plus
 *   engine  VRQ_LARGE_ENGINE_AUTO (the engine vrq_large_engine names), _VALU (K1h: exactly the *_large /
 *           *_filtered call) or _MFMA (K1hm, for any non-empty shape the *_large calls accept); any other
 *           value returns VRQ_EINVAL.
 *   allow   may be null here: an unfiltered search.  A misaligned non-null allow returns VRQ_EINVAL.
 *   For every input, every output is bit-identical, whichever engine runs, to the *_large call (allow null)
 *   or the *_filtered call with the same arguments; after vrq_scan_batch the T / count(dist < T) pairs and the
 *   K-lists in the workspace are bit-identical between the engines too (the dist < T part and the dist == T part
 *   each in row order, all-ones padded), each at its own plan's offset, and so are the histograms summed over
 *   the chunks: an engine's plan fixes its chunks, so the per-chunk arrays agree only where the plans do.  Shapes, flags (0 / VRQ_SEARCH_PHASE1_ONLY as in
 *   the *_large calls), stage masks, empty shapes and return codes are those of the *_filtered calls; the
 *   workspace (vrq_*_batch_workspace_size: a pure function of the shape, 0 for an unsupported one) covers
 *   either engine.  Every argument is checked before anything is launched.
 * vrq_large_engine (host-only): the engine AUTO takes for a shape, VRQ_LARGE_ENGINE_VALU or _MFMA, from a
 *   measured minimum batch per code size (tools/batch_bench.py); VRQ_EINVAL / VRQ_EUNSUPPORTED as
 *   vrq_scan_large_plan.
 * vrq_scan_batch_plan (host-only; tests and tools): info i64[10] = the engine that will run, rows per chunk
 *   (a multiple of 64), chunks, queries per wave of the count kernel (K1h: per workgroup), query blocks of a
 *   pass, rows a count workgroup scans between two flushes of its 16-bit bins (0: it never flushes), the
 *   workspace offsets of the histograms (u32 [min(nq, 512)][chunks][dim + 1]), of the T / count(dist < T) pairs
 *   and of the K-lists, and the workspace bytes.  With VRQ_LARGE_ENGINE_VALU the chunks and offsets are
 *   vrq_scan_large_plan's.
 * ------------------------------------------------------------------------- */
#define VRQ_LARGE_ENGINE_AUTO 0
#define VRQ_LARGE_ENGINE_VALU 1 /* K1h: exactly the *_large / *_filtered call */
#define VRQ_LARGE_ENGINE_MFMA 2 /* K1hm, any non-empty shape the *_large calls accept */
int vrq_large_engine(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t filtered);
int vrq_scan_batch_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t engine, int64_t* info);
size_t vrq_scan_batch_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_scan_batch(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                   int32_t stages, const uint64_t* allow, void* workspace, size_t workspace_bytes, void* stream,
                   int32_t engine);
size_t vrq_hamming_topk_batch_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k);
int vrq_hamming_topk_batch(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                           const uint8_t* queries, int32_t nq, int32_t k, const uint64_t* allow, int32_t* out_dist,
                           int64_t* out_rows, void* workspace, size_t workspace_bytes, void* stream,
                           int32_t engine);
size_t vrq_search3_batch_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search3_batch(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                      int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                      int32_t k, int32_t K, int32_t K3, int32_t flags, const uint64_t* allow, int32_t* out_count,
                      int64_t* out_rows, int32_t* out_dist, double* out_binary, double* out_cosine,
                      void* workspace, size_t workspace_bytes, void* stream, int32_t engine);
size_t vrq_search2_batch_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_search2_batch(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                      const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                      const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, const uint64_t* allow,
                      int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_score,
                      void* workspace, size_t workspace_bytes, void* stream, int32_t engine);

/* ---------------------------------------------------------------------------
 * Filtered search with a row bitmap per query (additive to ABI version 1; every call above keeps its
 * contract).  A serving batch mixes queries of different tenants, permission sets or date ranges: these calls
 * take a set of bitmaps and, per query, which of them filters it, on either engine of the counting scan.
 * vrq_scan_perquery / vrq_hamming_topk_perquery / vrq_search3_perquery / vrq_search2_perquery: the arguments
 *   of the *_batch call, `engine` included, followed by
 *   nsets      number of bitmaps `allow` holds, >= 1.
 *   set_words  u64 words from one bitmap to the next, >= ceil(n / 64) (bitmaps may be sized for capacity).
 *   query_set  device i32 [nq], 4-byte aligned: query q is filtered by bitmap query_set[q].  -1: every row is
 *              allowed (an unfiltered query).  Any other value outside [0, nsets): no row is allowed -- count 0,
 *              every output padding; no address is ever formed from such an id.
 *   allow      device u64, 8-byte aligned: bitmap s is the ceil(n / 64) words at allow + s * set_words, in the
 *              format of the *_filtered calls.  Words past ceil(n / 64) of a set are never read, bits past n
 *              are ignored; all index arithmetic is 64-bit.
 *   For every query q and every input, row q of every output array equals, bit for bit, the *_batch call of the
 *   same engine run on that query alone with allow + query_set[q] * set_words (a null allow for -1); hence the
 *   result does not depend on the engine, and after vrq_scan_perquery the T / count(dist < T) pairs and the
 *   K-lists in the workspace are bit-identical between the engines, as after vrq_scan_batch.  Shapes, flags,
 *   stage masks, engines, empty shapes (n, nq, K or k = 0 read neither array) and return codes are those of
 *   the *_batch calls; the workspace is vrq_*_batch_workspace_size (the bitmaps are the caller's and nothing
 *   else is staged in global memory).  A non-empty call returns VRQ_EINVAL for a null allow or query_set, an
 *   allow not 8-byte aligned, a query_set not 4-byte aligned, nsets < 1 or set_words < ceil(n / 64); every
 *   argument and the workspace size are checked before anything is launched.  vrq_large_engine(...,
 *   filtered = 1) and vrq_scan_batch_plan describe these calls unchanged: the plan, the chunks and the
 *   workspace layout do not depend on the filter's shape.
 * Both engines read a word per (64-row tile, resident query) as a scalar load; when every query of a count
 *   workgroup (K1h) or wave (K1hm) names the same set they run the single-bitmap loop body, inside an instance
 *   with a higher register use: measured at 1M rows, a batch in one set costs 1.05-1.18 times the *_batch call
 *   with that bitmap, and mixed sets cost K1h 1.1-1.3 times and K1hm up to 6.5 times that call
 *   (tools/perquery_bench.py, DESIGN section 5 "Per-query filters").  Not built: a filter on the sharded calls or on the
 *   exhaustive (gemm_topk) path, and skipping the loads of tiles no query may see.
 * ------------------------------------------------------------------------- */
int vrq_scan_perquery(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                      int32_t stages, const uint64_t* allow, void* workspace, size_t workspace_bytes, void* stream,
                      int32_t engine, int32_t nsets, int64_t set_words, const int32_t* query_set);
int vrq_hamming_topk_perquery(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                              const uint8_t* queries, int32_t nq, int32_t k, const uint64_t* allow,
                              int32_t* out_dist, int64_t* out_rows, void* workspace, size_t workspace_bytes,
                              void* stream, int32_t engine, int32_t nsets, int64_t set_words,
                              const int32_t* query_set);
int vrq_search3_perquery(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                         int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                         int32_t k, int32_t K, int32_t K3, int32_t flags, const uint64_t* allow, int32_t* out_count,
                         int64_t* out_rows, int32_t* out_dist, double* out_binary, double* out_cosine,
                         void* workspace, size_t workspace_bytes, void* stream, int32_t engine, int32_t nsets,
                         int64_t set_words, const int32_t* query_set);
int vrq_search2_perquery(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                         const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                         const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, const uint64_t* allow,
                         int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_score,
                         void* workspace, size_t workspace_bytes, void* stream, int32_t engine, int32_t nsets,
                         int64_t set_words, const int32_t* query_set);

/* ---------------------------------------------------------------------------
 * Row-sharded search with more than 1024 Phase-I candidates (additive to ABI version 1; vrq_shard_search3,
 * vrq_shard_search2, vrq_merge_shards and vrq_merge_shards2 keep their K <= 1024 contract).
 * vrq_shard_search3_large / vrq_shard_search2_large: the arguments and outputs of vrq_shard_search3 /
 *   vrq_shard_search2.  Outputs [nq, K]: the shard's exact Phase-I top-K in FAISS (dist, row) order, rows as
 *   row_offset + local row, every candidate with its score(s) -- s2 and s3 for the three-phase call, the
 *   vrq_rescore_dequant score of `mode` (every mode vrq_search2_large accepts) for the two-phase call -- taken
 *   from rescore_row[r] when given; no sort by score; out_count = min(K, n); missing slots -1 / INT32_MAX / NaN.
 *   Scores are bit-identical to vrq_rescore_binary_dim / vrq_rescore_int8_cosine_dim / vrq_rescore_dequant for
 *   the same (query, row), hence to the single-index *_large calls.  Supported: every dim of
 *   vrq_dim_supported, 1 <= K <= VRQ_K_LARGE_MAX, 1 <= n < 2^32; flags must be 0 (the counting scan takes no
 *   scan flags): any bit returns VRQ_EUNSUPPORTED.  n, nq or K = 0 behave as in the *_large search calls.
 *   Every argument and the workspace size (= vrq_search3_large_workspace_size) are checked before anything is
 *   launched.  Route: K1h, the sort of the K keys, one scoring launch per score kind over all K positions.
 * vrq_merge_shards_large / vrq_merge_shards2_large: the arguments, outputs and semantics of vrq_merge_shards /
 *   vrq_merge_shards2 plus a workspace of vrq_merge_shards_large_workspace_size(nshards, nq, K) bytes (one
 *   pure function for both; 0 for an unsupported shape).  Inputs: the stacked per-shard outputs [S, nq, K]
 *   with counts i32[S, nq]; each shard's list ascending in (dist, row) and shard s owning a contiguous global
 *   row range below shard s + 1's, as the per-shard calls leave them.  Three-phase: global top-K by (dist,
 *   global row) -> stable sort by s2 descending -> first min(K3, candidates) -> stable sort by s3 descending ->
 *   first k.  Two-phase: global top-K -> stable sort by score descending (-0.0 ties +0.0) -> first k.
 *   out_src (nullable) i32[nq, k] = s * K + p of each result in the stacked inputs, -1 for missing.
 *   Supported: 1 <= K <= VRQ_K_LARGE_MAX, 0 <= k <= VRQ_K_LARGE_MAX, any K3 >= 0, nshards <= 4096 (s * K + p
 *   < 2^25), distances in [0, 2048]; K <= 1024 is accepted on purpose and equals the merges above bit for bit.
 *   VRQ_EINVAL for null pointers or negative sizes, VRQ_EUNSUPPORTED past the limits, VRQ_EWORKSPACE for a
 *   short workspace, all before any launch.  The result equals vrq_search3_large / vrq_search2_large over the
 *   whole corpus, bit for bit.
 *   The global (dist, row) order of such inputs is their (dist, shard, position) order, so nothing is sorted:
 *   a histogram of the distances gives every distance's first global rank, and shard after shard each entry's
 *   rank is that plus its offset in its shard's run of equal distances; ranks below K are the result.
 * ------------------------------------------------------------------------- */
size_t vrq_shard_search3_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_shard_search3_large(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                            int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb,
                            int32_t nq, int32_t K, int32_t flags, int32_t* out_count, int64_t* out_rows,
                            int32_t* out_dist, double* out_binary, double* out_cosine, void* workspace,
                            size_t workspace_bytes, void* stream);
size_t vrq_shard_search2_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K);
int vrq_shard_search2_large(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                            const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                            const uint8_t* qb, int32_t nq, int32_t K, int32_t flags, int32_t* out_count,
                            int64_t* out_rows, int32_t* out_dist, double* out_score, void* workspace,
                            size_t workspace_bytes, void* stream);
size_t vrq_merge_shards_large_workspace_size(int32_t nshards, int32_t nq, int32_t K);
int vrq_merge_shards_large(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts, const int64_t* rows,
                           const int32_t* dist, const double* s2, const double* s3, int32_t k, int32_t K3,
                           int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_binary,
                           double* out_cosine, int32_t* out_src, void* workspace, size_t workspace_bytes,
                           void* stream);
int vrq_merge_shards2_large(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts, const int64_t* rows,
                            const int32_t* dist, const double* score, int32_t k, int32_t* out_count,
                            int64_t* out_rows, int32_t* out_dist, double* out_score, int32_t* out_src,
                            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VRQ_H_ */
