// select_rescore.hip -- K2: exact merge of the per-chunk Phase-I lists + fused
// Phase II / Phase III rescoring and the reference's stable sorts, one
// 256-thread workgroup per query.  Also the shard merge used after the RCCL
// all-gather (vrq_merge_shards) and the stand-alone rescoring entry points.
//
// Reference semantics (CohereEnhancedVectorDB.py):
//   :267-275  K = binary_k Phase-I hits in FAISS (dist asc, row asc) order
//   :283-293  s2 = float(qf . (2*unpackbits(code)-1))   float32.int32 -> float64
//   :296-297  stable sort by s2 desc, keep K3 = k*int8_oversample
//   :302-318  s3 = float(qf . int8) / np.linalg.norm(int8); -inf if norm == 0
//   :321-322  stable sort by s3 desc, first k
// Numerics: Phase II is accumulated in float64 -- every product is +-q_i
// (exact); when the non-zero |q_i| are multiples of some 2^g with
// sum|q_i| < 2^(g+53) (coordinates within ~2^20 of each other at dim 1024) the
// partial sums fit in 53 bits, so the sum is exact in any order and equals
// NumPy's ddot bit for bit; otherwise it is within gamma_(dim-1) * sum|q_i| of
// the exact dot and its last bits depend on the order (exact_scores.h).
// Phase III: the f32 x int8 products are exact in float64 and, under the same
// condition with 128 * sum|q_i|, so is their sum; rounding it once to float32
// gives the correctly rounded float32 dot (NumPy's sdot rounds per BLAS
// summation order, <= a few ulp away: the 1e-5 tolerance of the north star).
// The norm is sqrt of an exact integer sum (correctly rounded, equal
// to np.linalg.norm) and the division is IEEE double, as in the reference.
#include "dequant_dot.h"
#include "exact_scores.h"
#include "vrq_internal.h"
#include "vrq_scan.h"

namespace vrq {

constexpr int SEL_THREADS = 256;
constexpr int NBINS = 1025 + 3;     // dist in [0, 1024] for 1024-bit codes
constexpr uint64_t ROW_MASK = (1ull << KEY_ROW_BITS) - 1;

// Per-query LDS state, sized for at most KM candidates (binary_k) and ML lists.  The general
// instance (KMAX, MAX_LISTS) takes ~89 KiB, one workgroup per CU; the common shape (K <= 128,
// <= 64 lists) runs the small instance (~11 KiB) so 8 workgroups share a CU.
// (NB = histogram bins of the selection: every distance the code size allows, + padding)
template <int KM, int ML, int NB>
struct SelState {
  static constexpr int kKM = KM, kML = ML, kBins = NB;
  uint32_t hist[NB];
  int32_t ltcnt[ML];
  int32_t eqend[ML];
  uint64_t sel[KM];         // Phase-I keys (dist << 40 | row), FAISS order after select
  int32_t pay[KM];          // payload index (list * K + pos) of each selected key
  uint64_t skey[KM];        // sort keys (descending score image)
  int32_t sidx[KM];         // sort payload (Phase-I rank)
  double s2[KM];
  double s3[KM];
  int32_t ord2[KM];         // Phase-I ranks in Phase-II order (first K3)
  double s3o[KM];           // Phase-III scores in Phase-II order
  int32_t scan[SEL_THREADS / WAVE + 1];
  int32_t misc[8];
};
template <int KM, int ML>
struct SelShared : SelState<KM, ML, NBINS> {};
constexpr int KSMALL = 128, LSMALL = 64;
typedef SelShared<KMAX, MAX_LISTS> SelBig;
typedef SelShared<KSMALL, LSMALL> SelSmall;
// the instances of the other embedding dims (vrq_search3_dim): dist in [0, 2048]
constexpr int NBINS_DIM = 2049 + 3;
template <int KM, int ML>
struct SelSharedDim : SelState<KM, ML, NBINS_DIM> {};
typedef SelSharedDim<KMAX, MAX_LISTS> SelDimBig;
typedef SelSharedDim<KSMALL, LSMALL> SelDimSmall;
// Per-query LDS state of the two-phase finish (vrq_search2): what select_topk and stable_desc_order use,
// one score array, every distance up to 2048 (all dims of vrq_dim_supported, 1024 included).
template <int KM, int ML>
struct Sel2State {
  static constexpr int kKM = KM, kML = ML, kBins = NBINS_DIM;
  uint32_t hist[NBINS_DIM];
  int32_t ltcnt[ML];
  int32_t eqend[ML];
  uint64_t sel[KM];
  int32_t pay[KM];
  uint64_t skey[KM];
  int32_t sidx[KM];
  double s2[KM];
  int32_t scan[SEL_THREADS / WAVE + 1];
  int32_t misc[8];
};
typedef Sel2State<KMAX, MAX_LISTS> Sel2Big;
typedef Sel2State<KSMALL, LSMALL> Sel2Small;

// Block-wide exclusive scan of one int per thread; returns exclusive prefix, total in *tot.
__device__ inline int block_excl_scan(int v, int* tot, int32_t* scratch) {
  const int l = lane_id(), w = threadIdx.x / WAVE;
  int x = v;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int y = __shfl_up(x, o, WAVE);
    if (l >= o) x += y;
  }
  __syncthreads();
  if (l == WAVE - 1) scratch[w] = x;
  __syncthreads();
  int base = 0, all = 0;
  for (int i = 0; i < SEL_THREADS / WAVE; ++i) {
    const int s = scratch[i];
    if (i < w) base += s;
    all += s;
  }
  __syncthreads();
  *tot = all;
  return base + x - v;
}

// Exact top-Kp (Kp = min(K, #valid)) of the union of nl sorted lists of K keys each,
// whose row ranges are disjoint and increasing with the list index.  Result: sh.sel[0..Kp)
// ascending by key (= FAISS (dist, row) order) with sh.pay = list*K + pos.  Returns Kp.
template <class KeyAt, class SH>
__device__ int select_topk(const KeyAt& L, int nl, int K, SH& sh) {
  constexpr int NBINS = SH::kBins;  // (keys with dist >= NBINS would be dropped: the instance covers its dims)
  const int tid = threadIdx.x;
  const int total = nl * K;
  for (int i = tid; i < NBINS; i += SEL_THREADS) sh.hist[i] = 0;
  for (int i = tid; i < nl; i += SEL_THREADS) {
    sh.ltcnt[i] = 0;
    sh.eqend[i] = 0;
  }
  __syncthreads();
  for (int i = tid; i < total; i += SEL_THREADS) {
    const uint64_t key = L[i];
    const uint32_t d = (uint32_t)(key >> KEY_ROW_BITS);
    if (key != KEY_NONE && d < (uint32_t)NBINS) atomicAdd(&sh.hist[d], 1u);
  }
  __syncthreads();
  // threshold T: smallest d with cum(d) >= Kp
  constexpr int BPT = (NBINS + SEL_THREADS - 1) / SEL_THREADS;
  int local = 0;
  for (int b = 0; b < BPT; ++b) {
    const int i = tid * BPT + b;
    if (i < NBINS) local += (int)sh.hist[i];
  }
  int valid = 0;
  int pre = block_excl_scan(local, &valid, sh.scan);
  const int Kp = K < valid ? K : valid;
  if (tid == 0) {
    sh.misc[0] = 0x7fffffff;
    sh.misc[1] = 0;
  }
  __syncthreads();
  if (Kp == 0) return 0;
  {
    int cum = pre;
    for (int b = 0; b < BPT; ++b) {
      const int i = tid * BPT + b;
      if (i >= NBINS) break;
      const int h = (int)sh.hist[i];
      if (cum < Kp && cum + h >= Kp) {
        sh.misc[0] = i;    // T
        sh.misc[1] = cum;  // c_lt = #entries with dist < T
      }
      cum += h;
    }
  }
  __syncthreads();
  const uint32_t T = (uint32_t)sh.misc[0];
  const int c_lt = sh.misc[1];
  const int R = Kp - c_lt;  // entries with dist == T to take, in row order
  // per-list lt / eq run ends (each list is sorted by (dist,row))
  for (int i = tid; i < total; i += SEL_THREADS) {
    const int c = i / K, p = i - c * K;
    const uint32_t d = (uint32_t)(L[i] >> KEY_ROW_BITS);
    const uint32_t dn = (p + 1 < K) ? (uint32_t)(L[i + 1] >> KEY_ROW_BITS) : 0xffffffffu;
    if (d < T && dn >= T) sh.ltcnt[c] = p + 1;
    if (d == T && dn != T) sh.eqend[c] = p + 1;
  }
  __syncthreads();
  // exclusive scans over lists of lt counts and eq counts (LPT lists per thread)
  const int LPT = (nl + SEL_THREADS - 1) / SEL_THREADS;
  int sl = 0, se = 0;
  for (int b = 0; b < LPT; ++b) {
    const int c = tid * LPT + b;
    if (c < nl) {
      const int lt = sh.ltcnt[c];
      const int eq = sh.eqend[c] > lt ? sh.eqend[c] - lt : 0;
      sl += lt;
      se += eq;
    }
  }
  int tl, te;
  int pl = block_excl_scan(sl, &tl, sh.scan);
  int pe = block_excl_scan(se, &te, sh.scan);
  // convert ltcnt/eqend into (lt prefix, eq prefix - lt) in place, per thread range
  for (int b = 0; b < LPT; ++b) {
    const int c = tid * LPT + b;
    if (c < nl) {
      const int lt = sh.ltcnt[c];
      const int eq = sh.eqend[c] > lt ? sh.eqend[c] - lt : 0;
      sh.ltcnt[c] = pl;       // output base of this list's dist<T run
      sh.eqend[c] = pe - lt;  // rank of entry p (dist==T) = eqend[c] + p
      pl += lt;
      pe += eq;
    }
  }
  __syncthreads();
  for (int i = tid; i < total; i += SEL_THREADS) {
    const uint64_t key = L[i];
    const uint32_t d = (uint32_t)(key >> KEY_ROW_BITS);
    if (d > T) continue;
    const int c = i / K, p = i - c * K;
    if (d < T) {
      const int o = sh.ltcnt[c] + p;
      sh.sel[o] = key;
      sh.pay[o] = i;
    } else {
      const int r = sh.eqend[c] + p;
      if (r < R) {
        sh.sel[c_lt + r] = key;
        sh.pay[c_lt + r] = i;
      }
    }
  }
  __syncthreads();
  // sort the dist<T group (the dist==T group is already in row order)
  if (c_lt > 1) {
    const int np2 = next_pow2(c_lt);
    for (int i = c_lt + tid; i < np2; i += SEL_THREADS) {
      sh.skey[i] = KEY_NONE;
    }
    for (int i = tid; i < c_lt; i += SEL_THREADS) {
      sh.skey[i] = sh.sel[i];
      sh.sidx[i] = sh.pay[i];
    }
    block_bitonic_sort_kv(sh.skey, sh.sidx, np2);
    for (int i = tid; i < c_lt; i += SEL_THREADS) {
      sh.sel[i] = sh.skey[i];
      sh.pay[i] = sh.sidx[i];
    }
  }
  __syncthreads();
  return Kp;
}

// Stable descending sort of scores sc[0..m) keeping the original positions:
// (desc image of score, position) lexicographic -- Python's list.sort(reverse=True)
// on a key is stable, so equal scores keep their previous order (:296, :321).
template <class SH>
__device__ void stable_desc_order(const double* sc, int m, SH& sh) {
  if (m <= SEL_THREADS) {
    // one element per thread: its rank = #{j : (key_j, j) < (key_i, i)} over the m keys (broadcast LDS
    // reads), then one scatter -- 3 barriers instead of a bitonic network's log^2 rounds of them
    const int i = threadIdx.x;
    const uint64_t ki = i < m ? desc_key_f64(sc[i]) : KEY_NONE;
    if (i < m) sh.skey[i] = ki;
    __syncthreads();
    int rank = 0;
    if (i < m)
      for (int j = 0; j < m; ++j) {
        const uint64_t kj = sh.skey[j];
        rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
      }
    __syncthreads();
    if (i < m) {
      sh.skey[rank] = ki;
      sh.sidx[rank] = i;
    }
    __syncthreads();
    return;
  }
  const int np2 = next_pow2(m > 1 ? m : 1);
  for (int i = threadIdx.x; i < np2; i += SEL_THREADS) {
    sh.skey[i] = i < m ? desc_key_f64(sc[i]) : KEY_NONE;
    sh.sidx[i] = i < m ? i : 0x7fffffff;
  }
  // bitonic on (skey, sidx) lexicographic
  for (int size = 2; size <= np2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < (np2 >> 1); i += SEL_THREADS) {
        const int lo = ((i / stride) * stride * 2) + (i % stride);
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t ka = sh.skey[lo], kb = sh.skey[hi];
        const int ia = sh.sidx[lo], ib = sh.sidx[hi];
        const bool gt = (ka > kb) || (ka == kb && ia > ib);
        if (gt == up) {
          sh.skey[lo] = kb;
          sh.skey[hi] = ka;
          sh.sidx[lo] = ib;
          sh.sidx[hi] = ia;
        }
      }
    }
  }
  __syncthreads();
}

// Finish one query from Phase-I candidates sh.sel[0..Kp) with s2 (and s3 where needed)
// already in sh.s2/sh.s3 by Phase-I rank: stable sort by s2, cut K3, stable sort by
// s3, cut k, write outputs.  have_s3: s3 valid for all Kp (shard merge); otherwise
// it is computed here for the K3 survivors.
struct FinishArgs {
  const float* q;
  const int8_t* x8;
  const double* norms;
  const int64_t* remap;  // rescore row of each Phase-I row (IDMap2 rev_map[id_map[r]]), or null
  int64_t row_offset;  // added to local rows for output
  int k, K3;
  int32_t* out_count;
  int64_t* out_rows;
  int32_t* out_dist;
  double* out_s2;
  double* out_s3;
  int32_t* out_src;  // shard merge only: payload index (shard * K + pos) of each output, or null
  int kout;
};

template <class SH>
__device__ void finish_query(int Kp, bool have_s3, const FinishArgs& a, int qi, SH& sh) {
  const int tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  stable_desc_order(sh.s2, Kp, sh);  // sh.sidx[0..Kp) = Phase-I ranks in Phase-II order
  const int K3p = a.K3 < Kp ? a.K3 : Kp;
  // stash the Phase-II order (sidx is reused by the next sort)
  int32_t* ord2 = sh.ord2;
  for (int i = tid; i < K3p; i += SEL_THREADS) ord2[i] = sh.sidx[i];
  __syncthreads();
  if (!have_s3) {
    float qv[DPL];
    load_q(qv, a.q);
    // CB3 survivors per wave in flight: every row's load issued before the first score.  The loads are
    // unconditional (indices past K3p re-read the last survivor): a load under a divergent branch gets
    // its own vmcnt(0) at the branch join, which serialises the gathers (round 6: 59 -> ? us at config 2)
    constexpr int NW = SEL_THREADS / WAVE, CB3 = 8;
    for (int j0 = w; j0 < K3p; j0 += NW * CB3) {
      int64_t rowv[CB3];
#pragma unroll
      for (int i = 0; i < CB3; ++i) {
        const int j = j0 + NW * i;
        rowv[i] = (int64_t)(sh.sel[ord2[j < K3p ? j : K3p - 1]] & ROW_MASK);
      }
      if (a.remap)
#pragma unroll
        for (int i = 0; i < CB3; ++i) rowv[i] = a.remap[rowv[i]];
      int4 raw[CB3];
      double nrm[CB3];
#pragma unroll
      for (int i = 0; i < CB3; ++i) {
        raw[i] = phase3_load(a.x8 + rowv[i] * DIM);
        nrm[i] = a.norms[rowv[i]];
      }
#pragma unroll
      for (int i = 0; i < CB3; ++i) {
        const int j = j0 + NW * i;
        const double c = phase3_from(qv, raw[i], nrm[i]);
        if (j < K3p && l == 0) sh.s3[ord2[j]] = c;
      }
    }
  }
  __syncthreads();
  // gather s3 in Phase-II order, stable sort desc
  double* s3o = sh.s3o;
  for (int i = tid; i < K3p; i += SEL_THREADS) s3o[i] = sh.s3[ord2[i]];
  __syncthreads();
  stable_desc_order(s3o, K3p, sh);
  const int m = a.k < K3p ? a.k : K3p;
  for (int i = tid; i < a.kout; i += SEL_THREADS) {
    const int64_t o = (int64_t)qi * a.kout + i;
    if (i < m) {
      const int r = ord2[sh.sidx[i]];
      const uint64_t key = sh.sel[r];
      a.out_rows[o] = (int64_t)(key & ROW_MASK) + a.row_offset;
      a.out_dist[o] = (int32_t)(key >> KEY_ROW_BITS);
      a.out_s2[o] = sh.s2[r];
      a.out_s3[o] = sh.s3[r];
      if (a.out_src) a.out_src[o] = sh.pay[r];
    } else {
      a.out_rows[o] = -1;
      a.out_dist[o] = DIST_NONE;
      a.out_s2[o] = __builtin_nan("");
      a.out_s3[o] = __builtin_nan("");
      if (a.out_src) a.out_src[o] = -1;
    }
  }
  if (tid == 0) a.out_count[qi] = m;
}

// The lists a scan left for one query, [nl][K]: the chunk lists of the wavefront scans (K1 / K1d), or the
// single sorted list of a matrix-core scan.
struct ChunkKeys {
  const uint64_t* lists;
  __device__ uint64_t operator[](int i) const { return lists[i]; }
};

// Outputs in Phase-I order (VRQ_SEARCH_PHASE1_ONLY, and VRQ_SEARCH_SHARD with the two scores): the Kp
// selected candidates sh.sel[0..Kp), padded to a.kout.
template <class SH>
__device__ void write_phase1_order(int Kp, bool with_scores, const FinishArgs& a, int qi, const SH& sh) {
  for (int i = threadIdx.x; i < a.kout; i += SEL_THREADS) {
    const int64_t o = (int64_t)qi * a.kout + i;
    if (i < Kp) {
      a.out_rows[o] = (int64_t)(sh.sel[i] & ROW_MASK) + a.row_offset;
      a.out_dist[o] = (int32_t)(sh.sel[i] >> KEY_ROW_BITS);
      if (with_scores) {
        a.out_s2[o] = sh.s2[i];
        a.out_s3[o] = sh.s3[i];
      }
    } else {
      a.out_rows[o] = -1;
      a.out_dist[o] = DIST_NONE;
      if (with_scores) {
        a.out_s2[o] = __builtin_nan("");
        a.out_s3[o] = __builtin_nan("");
      }
    }
  }
  if (threadIdx.x == 0 && a.out_count) a.out_count[qi] = Kp;
}

// Phase II (:283-293) of the Kp candidates sh.sel[0..Kp) -> sh.s2, one candidate per lane.  The score is
// a sum of 256 nibble terms: for nibble p of the packed code (dims 4p..4p+3, MSB first) and its value v,
// T[p][v] = sum_b (bit b of v ? q[4p+b] : -q[4p+b]) in float64, and s2 = sum_p T[p][v_p] in nibble order.
// Under the condition of exact_scores.h (all |q_i| multiples of 2^g, sum|q_i| < 2^(g+53)) every partial sum is
// exact and s2 is the value of the wave-wide ddot of phase2_dot, bit for bit; otherwise the two orders agree
// within gamma_1023 * sum|q_i|, not in the last bits -- with 256 LDS lookups per candidate instead of 1024 products spread over a wave.
// The tables cover QT_NIB nibbles at a time (16 KiB of LDS: four workgroups of the small instance per CU).
constexpr int QT_NIB = 128;
template <class SH>
__device__ void phase2_nibble_tables(const float* __restrict__ q, const uint8_t* __restrict__ codes,
                                     const int64_t* __restrict__ remap, int Kp, SH& sh, double* qtab) {
  constexpr int NW = SEL_THREADS / WAVE;
  const int tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  for (int jb = 0; jb < Kp; jb += SEL_THREADS) {  // candidates jb + 4 l + w (all of them when Kp <= 256)
    const int j = jb + NW * l + w;
    const bool live = j < Kp;
    int64_t row = (int64_t)(sh.sel[live ? j : 0] & ROW_MASK);
    if (remap) row = remap[row];
    double acc = 0.0;
    for (int half = 0; half < 256 / QT_NIB; ++half) {
      // this half's code bytes of the lane's row (bytes 64 half .. +63), loaded before the table build
      uint4 cw[4];
      const uint4* src = reinterpret_cast<const uint4*>(codes + row * (DIM / 8) + half * (QT_NIB / 2));
#pragma unroll
      for (int i = 0; i < 4; ++i) cw[i] = src[i];
      __syncthreads();  // (the previous half's lookups are done)
      for (int e = tid; e < QT_NIB * 16; e += SEL_THREADS) {
        const int p = e >> 4, v = e & 15, d0 = 4 * (half * QT_NIB + p);
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double x = (double)q[d0 + b];
          t += ((v >> (3 - b)) & 1) ? x : -x;
        }
        qtab[e] = t;
      }
      __syncthreads();
      if (live) {
        const uint32_t wd[16] = {cw[0].x, cw[0].y, cw[0].z, cw[0].w, cw[1].x, cw[1].y, cw[1].z, cw[1].w,
                                 cw[2].x, cw[2].y, cw[2].z, cw[2].w, cw[3].x, cw[3].y, cw[3].z, cw[3].w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {  // byte 4k + c (little-endian in the dword): nibbles 2(4k+c), +1
            const uint32_t byte = (wd[k] >> (8 * c)) & 0xffu;
            const int pb = 2 * (4 * k + c);
            acc += qtab[pb * 16 + (byte >> 4)];
            acc += qtab[(pb + 1) * 16 + (byte & 15)];
          }
        }
      }
    }
    if (live) sh.s2[j] = acc;
  }
  __syncthreads();
}

// mode: 0 = full 3-phase; 1 = Phase I only; 2 = shard (all Kp candidates, s2 + s3, Phase-I order)
template <class SH>
// (the small instance at 4 waves per SIMD: every query of a 1024-query batch resident at once)
__global__ __launch_bounds__(SEL_THREADS, SH::kKM <= KSMALL ? 4 : 1) void select_rescore_kernel(
    const uint64_t* __restrict__ lists, int nl, bool sorted, int K, const uint8_t* __restrict__ codes,
    const int8_t* __restrict__ x8, const double* __restrict__ norms, const float* __restrict__ qf, int mode,
    FinishArgs fa) {
  __shared__ SH sh;
  const int qi = blockIdx.x;
  const int tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  const uint64_t* sq = lists + (int64_t)qi * nl * K;
  int Kp;
  if (sorted) {
    // the matrix-core scan's suffix stage left one list, already the exact top-K in FAISS (dist, row)
    // order with KEY_NONE padding after its valid prefix: taken as is
    if (tid == 0) sh.misc[0] = 0;
    __syncthreads();
    int valid = 0;
    for (int i = tid; i < K; i += SEL_THREADS) {
      const uint64_t key = sq[i];
      sh.sel[i] = key;
      sh.pay[i] = i;
      valid += key != KEY_NONE ? 1 : 0;
    }
    if (valid) atomicAdd(&sh.misc[0], valid);
    __syncthreads();
    Kp = sh.misc[0];
  } else {
    Kp = select_topk(ChunkKeys{sq}, nl, K, sh);
  }
  if (mode == 1) {
    write_phase1_order(Kp, false, fa, qi, sh);
    return;
  }
  // Phase II for all Kp candidates (float64, :283-293)
  const float* q = qf + (int64_t)qi * DIM;
  __shared__ double qtab[QT_NIB * 16];
  phase2_nibble_tables(q, codes, fa.remap, Kp, sh, qtab);
  if (mode == 2) {
    float qv[DPL];
    load_q(qv, q);
    for (int j = w; j < Kp; j += SEL_THREADS / WAVE) {
      uint64_t row = sh.sel[j] & ROW_MASK;
      if (fa.remap) row = (uint64_t)fa.remap[row];
      const double c = phase3_cos(qv, x8 + row * DIM, norms[row]);
      if (l == 0) sh.s3[j] = c;
    }
    __syncthreads();
    write_phase1_order(Kp, true, fa, qi, sh);
    return;
  }
  __syncthreads();
  FinishArgs a = fa;
  a.q = q;
  finish_query(Kp, false, a, qi, sh);
}

// ---------------------------------------------------------------------------
// The other embedding dims (vrq_search3_dim: dim a multiple of 128 up to 2048, a runtime argument).
// The same definitions as exact_scores.h with the loops over dim / 4 nibbles and dim / 128 lane pairs.
// ---------------------------------------------------------------------------
// Phase III of one row, one wave: lane l takes dims 2l, 2l+1 of every 128-dim block (coalesced 128-byte
// int8 and 512-byte query reads); exact products, exact f64 sum, one rounding to f32, f64 division.
__device__ __forceinline__ double phase3_cos_dim(const float* __restrict__ q, const int8_t* __restrict__ xrow,
                                                 double nrm, int dim) {
  double s = 0.0;
  for (int d = 2 * lane_id(); d < dim; d += 2 * WAVE) {
    const char2 x = *reinterpret_cast<const char2*>(xrow + d);
    const float2 qq = *reinterpret_cast<const float2*>(q + d);
    s += (double)qq.x * (double)x.x;
    s += (double)qq.y * (double)x.y;
  }
  s = wave_sum_f64(s);
  const float f = (float)s;
  return nrm == 0.0 ? -__builtin_inf() : (double)f / nrm;
}
// Phase II of one row, one wave (the stand-alone rescoring): the same lane -> dims map
__device__ __forceinline__ double phase2_dot_dim(const float* __restrict__ q, const uint8_t* __restrict__ code_row,
                                                 int dim) {
  double s = 0.0;
  for (int d = 2 * lane_id(); d < dim; d += 2 * WAVE) {
    const uint32_t byte = code_row[d >> 3];  // packbits is MSB-first: dim d at bit 7 - d % 8
    const float2 qq = *reinterpret_cast<const float2*>(q + d);
    s += ((byte >> (7 - (d & 7))) & 1) ? (double)qq.x : -(double)qq.x;
    s += ((byte >> (6 - (d & 7))) & 1) ? (double)qq.y : -(double)qq.y;
  }
  return wave_sum_f64(s);
}

// Phase II of the Kp candidates by nibble tables, as phase2_nibble_tables, over cb = dim / 8 code bytes in
// passes of up to 64 bytes (cb is a multiple of 16: the only pass of a 32- or 48-byte code and the second pass
// of a 96-byte code are shorter).  The same statement holds against phase2_dot_dim.
template <class SH>
__device__ void phase2_nibble_tables_dim(const float* __restrict__ q, const uint8_t* __restrict__ codes,
                                         const int64_t* __restrict__ remap, int Kp, int cb, SH& sh, double* qtab) {
  constexpr int NW = SEL_THREADS / WAVE;
  const int tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  for (int jb = 0; jb < Kp; jb += SEL_THREADS) {
    const int j = jb + NW * l + w;
    const bool live = j < Kp;
    int64_t row = (int64_t)(sh.sel[live ? j : 0] & ROW_MASK);
    if (remap) row = remap[row];
    double acc = 0.0;
    for (int b0 = 0; b0 < cb; b0 += QT_NIB / 2) {
      const int nb = cb - b0 < QT_NIB / 2 ? cb - b0 : QT_NIB / 2;  // code bytes of this pass
      uint4 cw[4];
      const uint4* src = reinterpret_cast<const uint4*>(codes + row * cb + b0);
#pragma unroll
      for (int i = 0; i < 4; ++i) cw[i] = 16 * i < nb ? src[i] : make_uint4(0, 0, 0, 0);
      __syncthreads();  // (the previous pass's lookups are done)
      for (int e = tid; e < nb * 2 * 16; e += SEL_THREADS) {
        const int p = e >> 4, v = e & 15, d0 = 4 * (2 * b0 + p);
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double x = (double)q[d0 + b];
          t += ((v >> (3 - b)) & 1) ? x : -x;
        }
        qtab[e] = t;
      }
      __syncthreads();
      if (live) {
        const uint32_t wd[16] = {cw[0].x, cw[0].y, cw[0].z, cw[0].w, cw[1].x, cw[1].y, cw[1].z, cw[1].w,
                                 cw[2].x, cw[2].y, cw[2].z, cw[2].w, cw[3].x, cw[3].y, cw[3].z, cw[3].w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (4 * k < nb) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {  // byte 4k + c of the pass (little-endian in the dword)
              const uint32_t byte = (wd[k] >> (8 * c)) & 0xffu;
              const int pb = 2 * (4 * k + c);
              acc += qtab[pb * 16 + (byte >> 4)];
              acc += qtab[(pb + 1) * 16 + (byte & 15)];
            }
          }
        }
      }
    }
    if (live) sh.s2[j] = acc;
  }
  __syncthreads();
}

// K2 for the other dims: merge of the K1d lists (histogram over every distance up to 2048) + Phase II +
// Phase III + the stable sorts.  mode: 0 = full 3-phase; 1 = Phase I only; 2 = shard (all Kp candidates,
// s2 + s3, Phase-I order), as at 1024.
template <class SH>
__global__ __launch_bounds__(SEL_THREADS, SH::kKM <= KSMALL ? 4 : 1) void select_rescore_dim_kernel(
    const uint64_t* __restrict__ lists, int nlp, int K, int dim, const uint8_t* __restrict__ codes,
    const int8_t* __restrict__ x8, const double* __restrict__ norms, const float* __restrict__ qf, int mode,
    FinishArgs fa) {
  __shared__ SH sh;
  const int qi = blockIdx.x;
  const int tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  const ChunkKeys Lq{lists + (int64_t)qi * nlp * K};
  const int Kp = select_topk(Lq, nlp, K, sh);
  if (mode == 1) {
    write_phase1_order(Kp, false, fa, qi, sh);
    return;
  }
  const float* q = qf + (int64_t)qi * dim;
  __shared__ double qtab[QT_NIB * 16];
  phase2_nibble_tables_dim(q, codes, fa.remap, Kp, dim / 8, sh, qtab);
  if (mode == 2) {
    // Phase III of every candidate, one wave per row (j, hence the row, is wave-uniform): the same
    // phase3_cos_dim call as below, so a shard's s3 is the single index's bit for bit
    for (int j = w; j < Kp; j += SEL_THREADS / WAVE) {
      int64_t row = (int64_t)(sh.sel[j] & ROW_MASK);
      if (fa.remap) row = fa.remap[row];
      const double c = phase3_cos_dim(q, x8 + row * dim, norms[row], dim);
      if (l == 0) sh.s3[j] = c;
    }
    __syncthreads();
    write_phase1_order(Kp, true, fa, qi, sh);
    return;
  }
  // Phase III of the K3 survivors of the Phase-II sort, one wave per row; finish_query then finds its
  // scores in sh.s3 (by Phase-I rank) and repeats the cheap Phase-II sort
  stable_desc_order(sh.s2, Kp, sh);
  const int K3p = fa.K3 < Kp ? fa.K3 : Kp;
  for (int i = tid; i < K3p; i += SEL_THREADS) sh.ord2[i] = sh.sidx[i];
  __syncthreads();
  for (int j = w; j < K3p; j += SEL_THREADS / WAVE) {
    int64_t row = (int64_t)(sh.sel[sh.ord2[j]] & ROW_MASK);
    if (fa.remap) row = fa.remap[row];
    const double c = phase3_cos_dim(q, x8 + row * dim, norms[row], dim);
    if (l == 0) sh.s3[sh.ord2[j]] = c;
  }
  __syncthreads();
  FinishArgs a = fa;
  a.q = q;
  finish_query(Kp, true, a, qi, sh);
}

// K2b, the finish of the fused two-phase search (vrq_search2; CohereVectorDBBinary.py:215-239 and the same
// loop of the VectorDBInt* classes, e.g. VectorDBInt8Global.py:224-252): exact merge of the lists the scan
// left (the K1 / K1d chunk lists, or the single sorted list of a matrix-core scan), one wave per candidate
// for the rescoring score of `mode` (dequant_dot, bit-identical to vrq_rescore_dequant), the stable sort by
// score descending over the Phase-I order, the first k.  No global scratch.
struct Finish2Args {
  int mode;
  const void* q;
  const double* minmax;
  double limit;
  const int64_t* remap;  // rescore row of each Phase-I row, or null
  int64_t row_offset;
  int k;
  int32_t* out_count;
  int64_t* out_rows;
  int32_t* out_dist;
  double* out_score;
  bool shard;  // vrq_shard_search2: all Kp candidates in Phase-I order with their scores, [nq][K], no sort
};

template <class SH>
__global__ __launch_bounds__(SEL_THREADS, SH::kKM <= KSMALL ? 4 : 1) void select_rescore2_kernel(
    const uint64_t* __restrict__ lists, int nl, int K, int dim, const float* __restrict__ qf, Finish2Args fa) {
  __shared__ SH sh;
  const int qi = blockIdx.x;
  const int tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  const ChunkKeys Lq{lists + (int64_t)qi * nl * K};
  const int Kp = select_topk(Lq, nl, K, sh);
  const float* q = qf + (int64_t)qi * dim;
  for (int j = w; j < Kp; j += SEL_THREADS / WAVE) {  // (j, hence the row, is wave-uniform)
    int64_t row = (int64_t)(sh.sel[j] & ROW_MASK);
    if (fa.remap) row = fa.remap[row];
    const double sc = dequant_dot(fa.mode, q, dim, fa.q, fa.minmax, fa.limit, row);
    if (l == 0) sh.s2[j] = sc;
  }
  __syncthreads();
  if (fa.shard) {  // (the same for every thread of the grid)
    for (int i = tid; i < K; i += SEL_THREADS) {
      const int64_t o = (int64_t)qi * K + i;
      const bool live = i < Kp;
      fa.out_rows[o] = live ? (int64_t)(sh.sel[i] & ROW_MASK) + fa.row_offset : -1;
      fa.out_dist[o] = live ? (int32_t)(sh.sel[i] >> KEY_ROW_BITS) : DIST_NONE;
      fa.out_score[o] = live ? sh.s2[i] : __builtin_nan("");
    }
    if (tid == 0) fa.out_count[qi] = Kp;
    return;
  }
  stable_desc_order(sh.s2, Kp, sh);  // sh.sidx[0..Kp) = Phase-I ranks by score desc, ties in Phase-I order
  const int m = fa.k < Kp ? fa.k : Kp;
  for (int i = tid; i < fa.k; i += SEL_THREADS) {
    const int64_t o = (int64_t)qi * fa.k + i;
    if (i < m) {
      const int r = sh.sidx[i];
      const uint64_t key = sh.sel[r];
      fa.out_rows[o] = (int64_t)(key & ROW_MASK) + fa.row_offset;
      fa.out_dist[o] = (int32_t)(key >> KEY_ROW_BITS);
      fa.out_score[o] = sh.s2[r];
    } else {
      fa.out_rows[o] = -1;
      fa.out_dist[o] = DIST_NONE;
      fa.out_score[o] = __builtin_nan("");
    }
  }
  if (tid == 0) fa.out_count[qi] = m;
}

// Shard merge: the lists are the shards' (dist, global row) candidates (VRQ_SEARCH_SHARD /
// vrq_shard_search3 outputs stacked [S][nq][K]); the payload carried to the finish step is s2/s3.
// The merge never reads the embedding dim: a distance up to 2048 fits the 24 key bits above
// KEY_ROW_BITS, and the host launches the instances whose histogram covers every such distance.
struct ShardKeys {
  const int32_t* counts;
  const int64_t* rows;
  const int32_t* dist;
  int nq, qi, K;
  __device__ uint64_t operator[](int i) const {
    const int s = i / K, p = i - s * K;
    const int64_t src = ((int64_t)s * nq + qi) * K + p;
    if (p >= counts[(int64_t)s * nq + qi] || rows[src] < 0) return KEY_NONE;
    return ((uint64_t)(uint32_t)dist[src] << KEY_ROW_BITS) | ((uint64_t)rows[src] & ROW_MASK);
  }
};

template <class SH>
__global__ __launch_bounds__(SEL_THREADS) void merge_shards_kernel(int S, int K, const int32_t* __restrict__ counts,
                                                                   const int64_t* __restrict__ rows,
                                                                   const int32_t* __restrict__ dist,
                                                                   const double* __restrict__ s2,
                                                                   const double* __restrict__ s3, int nq,
                                                                   FinishArgs fa) {
  __shared__ SH sh;
  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  const ShardKeys L{counts, rows, dist, nq, qi, K};
  const int Kp = select_topk(L, S, K, sh);
  for (int j = tid; j < Kp; j += SEL_THREADS) {
    const int i = sh.pay[j];
    const int s = i / K, p = i - s * K;
    const int64_t src = ((int64_t)s * nq + qi) * K + p;
    sh.s2[j] = s2[src];
    sh.s3[j] = s3[src];
  }
  __syncthreads();
  FinishArgs a = fa;
  a.row_offset = 0;
  finish_query(Kp, true, a, qi, sh);
}

// Shard merge of the two-phase search (vrq_shard_search2 outputs stacked [S][nq][K], one score per
// candidate): global top-K by (dist, global row), the stable sort by score descending over that order,
// the first k -- the tail of select_rescore2_kernel on the gathered candidates.
template <class SH>
__global__ __launch_bounds__(SEL_THREADS) void merge_shards2_kernel(
    int S, int K, const int32_t* __restrict__ counts, const int64_t* __restrict__ rows,
    const int32_t* __restrict__ dist, const double* __restrict__ score, int nq, int k,
    int32_t* __restrict__ out_count, int64_t* __restrict__ out_rows, int32_t* __restrict__ out_dist,
    double* __restrict__ out_score, int32_t* __restrict__ out_src) {
  __shared__ SH sh;
  const int qi = blockIdx.x;
  const int tid = threadIdx.x;
  const ShardKeys L{counts, rows, dist, nq, qi, K};
  const int Kp = select_topk(L, S, K, sh);
  for (int j = tid; j < Kp; j += SEL_THREADS) {
    const int i = sh.pay[j];
    const int s = i / K, p = i - s * K;
    sh.s2[j] = score[((int64_t)s * nq + qi) * K + p];
  }
  __syncthreads();
  stable_desc_order(sh.s2, Kp, sh);
  const int m = k < Kp ? k : Kp;
  for (int i = tid; i < k; i += SEL_THREADS) {
    const int64_t o = (int64_t)qi * k + i;
    const int r = i < m ? sh.sidx[i] : 0;
    out_rows[o] = i < m ? (int64_t)(sh.sel[r] & ROW_MASK) : -1;
    out_dist[o] = i < m ? (int32_t)(sh.sel[r] >> KEY_ROW_BITS) : DIST_NONE;
    out_score[o] = i < m ? sh.s2[r] : __builtin_nan("");
    if (out_src) out_src[o] = i < m ? sh.pay[r] : -1;
  }
  if (tid == 0) out_count[qi] = m;
}

// The two scores of one row for one query, one wave: at 1024 dims from the lane-resident query slice
// (exact_scores.h), at the other dims from the query in memory (the loops above).
struct Scorer1024 {
  float qv[DPL];
  __device__ Scorer1024(const float* __restrict__ qf, int qi, int) { load_q(qv, qf + (int64_t)qi * DIM); }
  __device__ double binary(const uint8_t* codes, int64_t row) const { return phase2_dot(qv, codes + row * (DIM / 8)); }
  __device__ double cosine(const int8_t* x8, int64_t row, double nrm) const {
    return phase3_cos(qv, x8 + row * DIM, nrm);
  }
};
struct ScorerDim {
  const float* q;
  int dim;
  __device__ ScorerDim(const float* __restrict__ qf, int qi, int d) : q(qf + (int64_t)qi * d), dim(d) {}
  __device__ double binary(const uint8_t* codes, int64_t row) const {
    return phase2_dot_dim(q, codes + row * (dim / 8), dim);
  }
  __device__ double cosine(const int8_t* x8, int64_t row, double nrm) const {
    return phase3_cos_dim(q, x8 + row * dim, nrm, dim);
  }
};

// Stand-alone candidate rescoring: one wave per (query, candidate).
template <class Scorer>
__global__ __launch_bounds__(256) void rescore_kernel(int which, const float* __restrict__ qf, int nq, int dim,
                                                      const uint8_t* __restrict__ codes,
                                                      const int8_t* __restrict__ x8,
                                                      const double* __restrict__ norms, int64_t n,
                                                      const int64_t* __restrict__ cand, int ncand,
                                                      double* __restrict__ out) {
  const int64_t gw = ((int64_t)blockIdx.x * 256 + threadIdx.x) / WAVE;
  if (gw >= (int64_t)nq * ncand) return;
  const int qi = (int)(gw / ncand);
  const int64_t row = cand[gw];
  if (row < 0 || row >= n) {
    if (lane_id() == 0) out[gw] = __builtin_nan("");
    return;
  }
  const Scorer sc(qf, qi, dim);
  const double v = which == 0 ? sc.binary(codes, row) : sc.cosine(x8, row, norms[row]);
  if (lane_id() == 0) out[gw] = v;
}

static int launch_rescore(int which, const float* qf, int nq, int dim, const uint8_t* codes, const int8_t* x8,
                          const double* norms, int64_t n, const int64_t* cand, int ncand, double* out,
                          hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)nq * ncand + 3) / 4));
  if (dim == DIM)
    hipLaunchKernelGGL(rescore_kernel<Scorer1024>, grid, dim3(256), 0, s, which, qf, nq, dim, codes, x8, norms, n,
                       cand, ncand, out);
  else
    hipLaunchKernelGGL(rescore_kernel<ScorerDim>, grid, dim3(256), 0, s, which, qf, nq, dim, codes, x8, norms, n,
                       cand, ncand, out);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// K2 on the lists a route's scan left in `ws`: the 1024 kernel at dim 1024, the runtime-dim kernel
// otherwise; of either, the small-LDS instance when the shape fits it.
static int launch_select(hipStream_t s, int nq, const void* ws, const Phase1Route& r, int K, int dim,
                         const uint8_t* codes, const int8_t* x8, const double* norms, const float* qf, int mode,
                         const FinishArgs& fa) {
  const uint64_t* lists = (const uint64_t*)((const uint8_t*)ws + r.off_lists);
  const bool small = K <= KSMALL && r.nl <= LSMALL;
  const dim3 grid(nq), block(SEL_THREADS);
  if (dim == DIM && small)
    hipLaunchKernelGGL(select_rescore_kernel<SelSmall>, grid, block, 0, s, lists, r.nl, r.sorted, K, codes, x8, norms,
                       qf, mode, fa);
  else if (dim == DIM)
    hipLaunchKernelGGL(select_rescore_kernel<SelBig>, grid, block, 0, s, lists, r.nl, r.sorted, K, codes, x8, norms,
                       qf, mode, fa);
  else if (small)  // (a matrix-core scan's sorted list is the single list of the merge)
    hipLaunchKernelGGL(select_rescore_dim_kernel<SelDimSmall>, grid, block, 0, s, lists, r.nl, K, dim, codes, x8,
                       norms, qf, mode, fa);
  else
    hipLaunchKernelGGL(select_rescore_dim_kernel<SelDimBig>, grid, block, 0, s, lists, r.nl, K, dim, codes, x8, norms,
                       qf, mode, fa);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// K2b on the lists a route's scan left in `ws` (a matrix-core scan's sorted list is the single list of
// the merge); the small-LDS instance when the shape fits it.
static int launch_select2(hipStream_t s, int nq, const void* ws, const Phase1Route& r, int K, int dim,
                          const float* qf, const Finish2Args& fa) {
  const uint64_t* lists = (const uint64_t*)((const uint8_t*)ws + r.off_lists);
  if (K <= KSMALL && r.nl <= LSMALL)
    hipLaunchKernelGGL(select_rescore2_kernel<Sel2Small>, dim3(nq), dim3(SEL_THREADS), 0, s, lists, r.nl, K, dim, qf,
                       fa);
  else
    hipLaunchKernelGGL(select_rescore2_kernel<Sel2Big>, dim3(nq), dim3(SEL_THREADS), 0, s, lists, r.nl, K, dim, qf,
                       fa);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// ---------------------------------------------------------------------------
// The large finish (vrq_*_large, K up to VRQ_K_LARGE_MAX): the K-lists the counting scan K1h left hold the
// exact top-K of each query, not yet in distance order.  The per-query state no longer fits LDS next to the
// sort, so scores live in the workspace and the finish is a chain of launches on it:
//   large_sort_kernel    sorts the K keys ascending (= FAISS (dist, row) order) in LDS, counts the candidates
//                        (Phase-I-only calls write their outputs here)
//   large_score_kernel   one wave per (query, candidate) over the whole grid: the stand-alone rescoring's
//                        Scorer1024 / ScorerDim / dequant_dot, so scores are bit-identical to
//                        vrq_rescore_*_dim / vrq_rescore_dequant and to vrq_search2 for every input, and to
//                        vrq_search3_dim's Phase III; to its Phase II (nibble order) under the condition
//                        of exact_scores.h, within its bound otherwise
//   large_order_kernel   sorts the pairs (descending-score image, position) lexicographically in LDS -- the
//                        stable order -- and either keeps the order of the first K3 (three-phase, after Phase
//                        II) or writes the first k outputs
// 8192 pairs of (u64, i32) take 96 KiB of LDS: that is where VRQ_K_LARGE_MAX comes from.
// ---------------------------------------------------------------------------
constexpr int LARGE_THREADS = 1024;

template <int CAP>
__global__ __launch_bounds__(LARGE_THREADS) void large_sort_kernel(uint64_t* __restrict__ lists, int K,
                                                                   int32_t* __restrict__ kp, bool write_out,
                                                                   int64_t row_offset, int32_t* __restrict__ out_count,
                                                                   int64_t* __restrict__ out_rows,
                                                                   int32_t* __restrict__ out_dist) {
  __shared__ uint64_t keys[CAP];
  __shared__ int32_t cnt;
  const int q = blockIdx.x, tid = threadIdx.x;
  uint64_t* list = lists + (int64_t)q * K;
  const int np2 = next_pow2(K);
  for (int i = tid; i < np2; i += LARGE_THREADS) keys[i] = i < K ? list[i] : KEY_NONE;
  if (tid == 0) cnt = 0;
  block_bitonic_sort_u64(keys, np2);
  for (int i = tid; i < K; i += LARGE_THREADS)  // the valid keys are a prefix: KEY_NONE is the largest key
    if (keys[i] != KEY_NONE && (i + 1 == K || keys[i + 1] == KEY_NONE)) cnt = i + 1;
  __syncthreads();
  const int Kp = cnt;
  for (int i = tid; i < K; i += LARGE_THREADS) {
    const uint64_t key = keys[i];
    list[i] = key;
    if (write_out) {
      const int64_t o = (int64_t)q * K + i;
      out_rows[o] = i < Kp ? (int64_t)(key & ROW_MASK) + row_offset : -1;
      out_dist[o] = i < Kp ? (int32_t)(key >> KEY_ROW_BITS) : DIST_NONE;
    }
  }
  if (tid == 0) {
    kp[q] = Kp;
    if (write_out && out_count) out_count[q] = Kp;
  }
}

// what a large_score_kernel launch scores: Phase II (binary), Phase III (cosine) or the two-phase score
struct LargeScoreArgs {
  int which;  // 0 binary, 1 int8 cosine, 2 dequant_dot of `mode`
  const uint64_t* lists;
  const int32_t* kp;
  const int32_t* ord;  // position -> Phase-I rank (Phase III: the Phase-II order), or null (identity)
  int K, limit;        // positions [0, min(kp, limit)) are scored
  const int64_t* remap;
  const uint8_t* codes;
  const int8_t* x8;
  const double* norms;
  int mode;
  const void* dq;
  const double* minmax;
  double dlimit;
  double* out;  // [nq][K] by position
  bool pad;     // positions [min(kp, limit), K) get NaN (the per-shard calls score into the caller's arrays)
};

template <class Scorer>
__global__ __launch_bounds__(256) void large_score_kernel(const float* __restrict__ qf, int dim, int bpq,
                                                          LargeScoreArgs a) {
  const int q = blockIdx.x / bpq;
  const int i = (blockIdx.x - q * bpq) * (256 / WAVE) + threadIdx.x / WAVE;  // wave-uniform
  const int kpq = a.kp[q];
  const int m = kpq < a.limit ? kpq : a.limit;
  const int64_t base = (int64_t)q * a.K;
  if (i >= m) {
    if (a.pad && i < a.K && lane_id() == 0) a.out[base + i] = __builtin_nan("");
    return;
  }
  const int r = a.ord ? a.ord[base + i] : i;
  int64_t row = (int64_t)(a.lists[base + r] & ROW_MASK);
  if (a.remap) row = a.remap[row];
  double v;
  if (a.which == 2) {
    v = dequant_dot(a.mode, qf + (int64_t)q * dim, dim, a.dq, a.minmax, a.dlimit, row);
  } else {
    const Scorer sc(qf, q, dim);
    v = a.which == 0 ? sc.binary(a.codes, row) : sc.cosine(a.x8, row, a.norms[row]);
  }
  if (lane_id() == 0) a.out[base + i] = v;
}

struct LargeOrderArgs {
  const double* sc;    // scores to sort, [nq][K] by position
  const int32_t* kp;
  int K, limit;        // the first min(kp, limit) positions take part
  int32_t* ord_out;    // non-null: keep the order of the first `keep` (position -> Phase-I rank) and stop
  int keep;
  const double* carry_in;  // with ord_out, non-null (shard merge): carry_out[position] = carry_in[Phase-I rank]
  double* carry_out;
  // the final write (ord_out == null)
  const int32_t* ord;  // sorted position -> Phase-I rank (three-phase), or null (the position is the rank)
  const uint64_t* lists;
  const double* s2;    // [nq][K] by Phase-I rank
  int64_t row_offset;
  int k;
  int32_t* out_count;
  int64_t* out_rows;
  int32_t* out_dist;
  double* out_s2;
  double* out_s3;      // three-phase only: a.sc of the position
  const int32_t* src;  // shard merge: shard * K + position of each Phase-I rank in the stacked inputs ...
  int32_t* out_src;    // ... written per output when non-null (-1 padded)
};

template <int CAP>
__global__ __launch_bounds__(LARGE_THREADS) void large_order_kernel(LargeOrderArgs a) {
  __shared__ uint64_t skey[CAP];
  __shared__ int32_t sidx[CAP];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int64_t base = (int64_t)q * a.K;
  const int kpq = a.kp[q];
  const int m = kpq < a.limit ? kpq : a.limit;
  const int np2 = next_pow2(m > 1 ? m : 1);
  for (int i = tid; i < np2; i += LARGE_THREADS) {
    skey[i] = i < m ? desc_key_f64(a.sc[base + i]) : KEY_NONE;
    sidx[i] = i < m ? i : 0x7fffffff;
  }
  // bitonic on (skey, sidx) lexicographic: the stable order (stable_desc_order)
  for (int size = 2; size <= np2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (np2 >> 1); i += LARGE_THREADS) {
        const int lo = ((i / stride) * stride * 2) + (i % stride);
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t ka = skey[lo], kb = skey[hi];
        const int ia = sidx[lo], ib = sidx[hi];
        const bool gt = (ka > kb) || (ka == kb && ia > ib);
        if (gt == up) {
          skey[lo] = kb;
          skey[hi] = ka;
          sidx[lo] = ib;
          sidx[hi] = ia;
        }
      }
    }
  }
  __syncthreads();
  if (a.ord_out) {
    const int keep = a.keep < m ? a.keep : m;
    for (int i = tid; i < keep; i += LARGE_THREADS) {
      a.ord_out[base + i] = sidx[i];
      if (a.carry_in) a.carry_out[base + i] = a.carry_in[base + sidx[i]];
    }
    return;
  }
  const int mo = a.k < m ? a.k : m;
  for (int i = tid; i < a.k; i += LARGE_THREADS) {
    const int64_t o = (int64_t)q * a.k + i;
    if (i < mo) {
      const int j = sidx[i];
      const int r = a.ord ? a.ord[base + j] : j;
      const uint64_t key = a.lists[base + r];
      a.out_rows[o] = (int64_t)(key & ROW_MASK) + a.row_offset;
      a.out_dist[o] = (int32_t)(key >> KEY_ROW_BITS);
      a.out_s2[o] = a.s2[base + r];
      if (a.out_s3) a.out_s3[o] = a.sc[base + j];
      if (a.out_src) a.out_src[o] = a.src[base + r];
    } else {
      a.out_rows[o] = -1;
      a.out_dist[o] = DIST_NONE;
      a.out_s2[o] = __builtin_nan("");
      if (a.out_s3) a.out_s3[o] = __builtin_nan("");
      if (a.out_src) a.out_src[o] = -1;
    }
  }
  if (tid == 0) a.out_count[q] = mo;
}

static int large_sort_launch(hipStream_t s, int nq, uint64_t* lists, int K, int32_t* kp, bool write_out,
                             int64_t row_offset, int32_t* out_count, int64_t* out_rows, int32_t* out_dist) {
  const dim3 grid(nq), block(LARGE_THREADS);
  if (K <= 1024)
    hipLaunchKernelGGL(large_sort_kernel<1024>, grid, block, 0, s, lists, K, kp, write_out, row_offset, out_count,
                       out_rows, out_dist);
  else if (K <= 2048)
    hipLaunchKernelGGL(large_sort_kernel<2048>, grid, block, 0, s, lists, K, kp, write_out, row_offset, out_count,
                       out_rows, out_dist);
  else if (K <= 4096)
    hipLaunchKernelGGL(large_sort_kernel<4096>, grid, block, 0, s, lists, K, kp, write_out, row_offset, out_count,
                       out_rows, out_dist);
  else
    hipLaunchKernelGGL(large_sort_kernel<VRQ_K_LARGE_MAX>, grid, block, 0, s, lists, K, kp, write_out, row_offset,
                       out_count, out_rows, out_dist);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

static int large_score_launch(hipStream_t s, int nq, const float* qf, int dim, const LargeScoreArgs& a) {
  const int m = a.K < a.limit ? a.K : a.limit;
  if (m < 1) return VRQ_OK;
  const int bpq = (m + 256 / WAVE - 1) / (256 / WAVE);
  const dim3 grid((unsigned)((int64_t)nq * bpq));
  if (dim == DIM)
    hipLaunchKernelGGL(large_score_kernel<Scorer1024>, grid, dim3(256), 0, s, qf, dim, bpq, a);
  else
    hipLaunchKernelGGL(large_score_kernel<ScorerDim>, grid, dim3(256), 0, s, qf, dim, bpq, a);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

static int large_order_launch(hipStream_t s, int nq, const LargeOrderArgs& a) {
  const int m = a.K < a.limit ? a.K : a.limit;  // entries sorted at the most
  const dim3 grid(nq), block(LARGE_THREADS);
  if (m <= 1024)
    hipLaunchKernelGGL(large_order_kernel<1024>, grid, block, 0, s, a);
  else if (m <= 2048)
    hipLaunchKernelGGL(large_order_kernel<2048>, grid, block, 0, s, a);
  else if (m <= 4096)
    hipLaunchKernelGGL(large_order_kernel<4096>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(large_order_kernel<VRQ_K_LARGE_MAX>, grid, block, 0, s, a);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// ---------------------------------------------------------------------------
// The large shard merge (vrq_merge_shards*_large): the global top-K of S stacked K-lists, K up to
// VRQ_K_LARGE_MAX.  S * K keys do not fit LDS (512 KiB at S = 8, K = 8192), and they need not be sorted:
// every shard's list is ascending in (dist, row) and shard s owns the rows below shard s + 1's, so the global
// (dist, row) order is the (dist, shard, position) order, and a distance is an integer in [0, 2048].  One
// workgroup per query:
//   histogram   the entries of one distance are a run inside each shard's list, so the run's head subtracts
//               its position from the bin and its tail adds its position + 1: two LDS atomics per (shard,
//               distance) instead of one per entry on an address all 64 lanes of a wave share
//   prefix      cursor[d] = count(dist < d): the global rank of the first entry at distance d
//   ranks       shard after shard: an entry's global rank is cursor[d] + its offset in its run; ranks below
//               min(K, entries) are the result -- every entry below T, and of those at T the first
//               K - count(dist < T) in (shard, position) order -- and go, with their scores and their index
//               s * K + p in the stacked inputs, straight to their slot in the workspace; then the run's
//               tail advances cursor[d] by the run length
// The stable sorts and the final write are large_order_kernel's.  An entry past its shard's count, with a
// negative row or a distance outside [0, 2048] takes no part (the first two as in merge_shards_kernel); lists
// that are not ascending give ranks that collide, never a store outside [0, K).
// ---------------------------------------------------------------------------
constexpr int MERGE_BINS = 2049;

struct MergeSelectArgs {
  int S, K, nq;
  const int32_t* counts;  // [S][nq]
  const int64_t* rows;    // [S][nq][K] global rows
  const int32_t* dist;
  const double* s2;       // the score of the two-phase merge
  const double* s3;       // null for the two-phase merge
  uint64_t* keys;         // [nq][K] by global rank, KEY_NONE padded
  int32_t* src;           // [nq][K] s * K + p, -1 padded
  double* w2;             // [nq][K] by global rank
  double* w3;
  int32_t* kp;            // [nq] min(K, entries)
};

// the distance of entry p of a shard's list, -1 where the entry takes no part
__device__ __forceinline__ int merge_dist_at(const MergeSelectArgs& a, int64_t base, int p, int cnt) {
  if (p < 0 || p >= cnt) return -1;
  const int d = a.dist[base + p];
  return a.rows[base + p] >= 0 && (uint32_t)d < (uint32_t)MERGE_BINS ? d : -1;
}

template <int PER>  // entries of one shard per thread: K <= PER * LARGE_THREADS
__global__ __launch_bounds__(LARGE_THREADS) void merge_select_kernel(MergeSelectArgs a) {
  __shared__ int32_t cursor[MERGE_BINS];    // the histogram, then the next global rank of every distance
  __shared__ int32_t runstart[MERGE_BINS];  // position of the head of the current shard's run
  __shared__ int32_t scratch[LARGE_THREADS];
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int b = tid; b < MERGE_BINS; b += LARGE_THREADS) cursor[b] = 0;
  __syncthreads();
  for (int s = 0; s < a.S; ++s) {
    const int c = a.counts[(int64_t)s * a.nq + q];
    const int cnt = c < 0 ? 0 : c < a.K ? c : a.K;
    const int64_t base = ((int64_t)s * a.nq + q) * a.K;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int p = tid + j * LARGE_THREADS;
      const int d = merge_dist_at(a, base, p, cnt);
      if (d < 0) continue;
      if (merge_dist_at(a, base, p - 1, cnt) != d) atomicSub(&cursor[d], p);
      if (merge_dist_at(a, base, p + 1, cnt) != d) atomicAdd(&cursor[d], p + 1);
    }
  }
  __syncthreads();
  // exclusive prefix over the bins: BPT consecutive bins per thread, a workgroup scan of the thread sums
  constexpr int BPT = (MERGE_BINS + LARGE_THREADS - 1) / LARGE_THREADS;
  int h[BPT], local = 0;
#pragma unroll
  for (int b = 0; b < BPT; ++b) {
    const int i = tid * BPT + b;
    h[b] = i < MERGE_BINS ? cursor[i] : 0;
    local += h[b];
  }
  scratch[tid] = local;
  __syncthreads();
  for (int o = 1; o < LARGE_THREADS; o <<= 1) {
    const int y = tid >= o ? scratch[tid - o] : 0;
    __syncthreads();
    scratch[tid] += y;
    __syncthreads();
  }
  int cum = scratch[tid] - local;
  const int total = scratch[LARGE_THREADS - 1];
#pragma unroll
  for (int b = 0; b < BPT; ++b) {
    const int i = tid * BPT + b;
    if (i < MERGE_BINS) cursor[i] = cum;
    cum += h[b];
  }
  const int want = total < a.K ? total : a.K;
  const int64_t ob = (int64_t)q * a.K;
  __syncthreads();
  for (int s = 0; s < a.S; ++s) {
    const int c = a.counts[(int64_t)s * a.nq + q];
    const int cnt = c < 0 ? 0 : c < a.K ? c : a.K;
    const int64_t base = ((int64_t)s * a.nq + q) * a.K;
    int dv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int p = tid + j * LARGE_THREADS;
      dv[j] = merge_dist_at(a, base, p, cnt);
      if (dv[j] >= 0 && merge_dist_at(a, base, p - 1, cnt) != dv[j]) runstart[dv[j]] = p;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int p = tid + j * LARGE_THREADS;
      if (dv[j] < 0) continue;
      const int rank = cursor[dv[j]] + p - runstart[dv[j]];
      if ((uint32_t)rank < (uint32_t)want) {
        a.keys[ob + rank] = ((uint64_t)(uint32_t)dv[j] << KEY_ROW_BITS) | ((uint64_t)a.rows[base + p] & ROW_MASK);
        a.src[ob + rank] = s * a.K + p;
        a.w2[ob + rank] = a.s2[base + p];
        if (a.s3) a.w3[ob + rank] = a.s3[base + p];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int p = tid + j * LARGE_THREADS;
      if (dv[j] >= 0 && merge_dist_at(a, base, p + 1, cnt) != dv[j]) cursor[dv[j]] += p - runstart[dv[j]] + 1;
    }
    __syncthreads();
  }
  for (int i = want + tid; i < a.K; i += LARGE_THREADS) {
    a.keys[ob + i] = KEY_NONE;
    a.src[ob + i] = -1;
  }
  if (tid == 0) a.kp[q] = want;
}

static int merge_select_launch(hipStream_t s, const MergeSelectArgs& a) {
  const dim3 grid(a.nq), block(LARGE_THREADS);
  if (a.K <= LARGE_THREADS)
    hipLaunchKernelGGL(merge_select_kernel<1>, grid, block, 0, s, a);
  else if (a.K <= 2 * LARGE_THREADS)
    hipLaunchKernelGGL(merge_select_kernel<2>, grid, block, 0, s, a);
  else if (a.K <= 4 * LARGE_THREADS)
    hipLaunchKernelGGL(merge_select_kernel<4>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(merge_select_kernel<VRQ_K_LARGE_MAX / LARGE_THREADS>, grid, block, 0, s, a);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// workspace of a large merge: everything is [nq][K] but the counts
struct MergePlan {
  size_t off_keys, off_src, off_w2, off_w3, off_w3p, off_ord, off_kp, bytes;
};

static bool merge_plan(int nshards, int nq, int K, MergePlan* p) {
  if (nshards < 1 || nshards > MAX_LISTS || nq < 1 || K < 1 || K > VRQ_K_LARGE_MAX) return false;
  const auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t m = (size_t)nq * K;
  size_t off = 0;
  p->off_keys = off;
  off = al(off + m * sizeof(uint64_t));
  p->off_src = off;
  off = al(off + m * sizeof(int32_t));
  p->off_w2 = off;
  off = al(off + m * sizeof(double));
  p->off_w3 = off;
  off = al(off + m * sizeof(double));
  p->off_w3p = off;  // s3 by position in the Phase-II order
  off = al(off + m * sizeof(double));
  p->off_ord = off;
  off = al(off + m * sizeof(int32_t));
  p->off_kp = off;
  off = al(off + (size_t)nq * sizeof(int32_t));
  p->bytes = off;
  return true;
}

}  // namespace vrq

using namespace vrq;

extern "C" {

// ---- Phase I: every entry point below takes its scan from the route (vrq_scan.h) ----
size_t vrq_hamming_topk_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k) {
  return phase1_workspace_bytes(n, code_bytes, nq, k);
}

size_t vrq_search3_dim_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_dim_supported(dim) ? phase1_workspace_bytes(n, dim / 8, nq, K) : 0;
}

size_t vrq_search3_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return dim == DIM ? vrq_search3_dim_workspace_size(n, dim, nq, K) : 0;
}

size_t vrq_search2_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_dim_workspace_size(n, dim, nq, K);
}

// the route of a call (n, nq, K >= 1) and the workspace check every entry point makes before it launches
static int route_checked(int64_t n, int cb, int nq, int K, int flags, size_t workspace_bytes, Phase1Route* r) {
  const int rc = phase1_route(n, cb, nq, K, flags, r);
  if (rc != VRQ_OK) return rc;
  return workspace_bytes < r->bytes ? VRQ_EWORKSPACE : VRQ_OK;
}

static FinishArgs finish_args(const int8_t* x8, const double* norms, const int64_t* remap, int64_t row_offset, int k,
                              int K3, int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_s2,
                              double* out_s3, int32_t* out_src, int kout) {
  FinishArgs fa{};
  fa.x8 = x8;
  fa.norms = norms;
  fa.remap = remap;
  fa.row_offset = row_offset;
  fa.k = k;
  fa.K3 = K3;
  fa.out_count = out_count;
  fa.out_rows = out_rows;
  fa.out_dist = out_dist;
  fa.out_s2 = out_s2;
  fa.out_s3 = out_s3;
  fa.out_src = out_src;
  fa.kout = kout;
  return fa;
}

static int fill_empty(int32_t nq, int32_t kout, int32_t* out_count, int64_t* out_rows, int32_t* out_dist,
                      double* out_s2, double* out_s3, hipStream_t s) {
  // n == 0 or K == 0: no candidates (CohereEnhancedVectorDB.py:247-249, :277-279)
  if (out_count && hipMemsetAsync(out_count, 0, sizeof(int32_t) * nq, s) != hipSuccess) return VRQ_EHIP;
  const size_t m = (size_t)nq * kout;
  if (m == 0) return VRQ_OK;
  if (out_rows && hipMemsetAsync(out_rows, 0xff, sizeof(int64_t) * m, s) != hipSuccess) return VRQ_EHIP;   // -1
  if (out_dist && hipMemsetAsync(out_dist, 0x7f, sizeof(int32_t) * m, s) != hipSuccess) return VRQ_EHIP;   // ~INT_MAX
  if (out_s2 && hipMemsetAsync(out_s2, 0xff, sizeof(double) * m, s) != hipSuccess) return VRQ_EHIP;       // NaN
  if (out_s3 && hipMemsetAsync(out_s3, 0xff, sizeof(double) * m, s) != hipSuccess) return VRQ_EHIP;
  return VRQ_OK;
}

int vrq_hamming_topk(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                     const uint8_t* queries, int32_t nq, int32_t k, int32_t* out_dist, int64_t* out_rows,
                     void* workspace, size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && out_dist && out_rows);
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || k == 0) return fill_empty(nq, k, nullptr, out_rows, out_dist, nullptr, nullptr, s);
  VRQ_CHECK_ARG(codes && queries && workspace);
  Phase1Route r;
  int rc = route_checked(n, code_bytes, nq, k, 0, workspace_bytes, &r);
  if (rc != VRQ_OK) return rc;
  rc = phase1_launch(r, codes, n, code_bytes, queries, nq, k, workspace, s, 0);
  if (rc != VRQ_OK) return rc;
  const FinishArgs fa = finish_args(nullptr, nullptr, nullptr, row_offset, 0, 0, nullptr, out_rows, out_dist, nullptr,
                                    nullptr, nullptr, k);
  return launch_select(s, nq, workspace, r, k, code_bytes * 8, nullptr, nullptr, nullptr, nullptr, 1, fa);
}

// The staged three-phase search at every dim of vrq_dim_supported.  VRQ_SEARCH_SHARD stays 1024-only on
// these entry points (their ABI-1 contract); the other dims shard through vrq_shard_search3.
int vrq_search3_dim_scan(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                         int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && K >= 0);
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  if (dim != DIM && (flags & VRQ_SEARCH_SHARD)) return VRQ_EUNSUPPORTED;
  if (nq == 0 || n == 0 || K == 0) return VRQ_OK;
  VRQ_CHECK_ARG(codes && qb && workspace);
  Phase1Route r;
  const int rc = route_checked(n, dim / 8, nq, K, flags, workspace_bytes, &r);
  if (rc != VRQ_OK) return rc;
  return phase1_launch(r, codes, n, dim / 8, qb, nq, K, workspace, (hipStream_t)stream, flags);
}

int vrq_search3_dim_finish(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                           int64_t n, int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k,
                           int32_t K, int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows,
                           int32_t* out_dist, double* out_binary, double* out_cosine, const void* workspace,
                           size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0 && K3 >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist);
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  if (dim != DIM && (flags & VRQ_SEARCH_SHARD)) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int mode = (flags & VRQ_SEARCH_PHASE1_ONLY) ? 1 : (flags & VRQ_SEARCH_SHARD) ? 2 : 0;
  const int kout = mode == 0 ? k : K;
  if (nq == 0) return VRQ_OK;
  if (mode != 1) VRQ_CHECK_ARG(out_binary && out_cosine);
  if (n == 0 || K == 0 || (mode == 0 && k == 0))
    return fill_empty(nq, kout, out_count, out_rows, out_dist, out_binary, out_cosine, s);
  VRQ_CHECK_ARG(codes && workspace);
  if (mode != 1) VRQ_CHECK_ARG(qf && x8 && norms);
  Phase1Route r;
  const int rc = route_checked(n, dim / 8, nq, K, flags, workspace_bytes, &r);
  if (rc != VRQ_OK) return rc;
  const FinishArgs fa = finish_args(x8, norms, rescore_row, row_offset, k, K3, out_count, out_rows, out_dist,
                                    out_binary, out_cosine, nullptr, kout);
  return launch_select(s, nq, workspace, r, K, dim, codes, x8, norms, qf, mode, fa);
}

int vrq_search3_dim(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                    int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                    int32_t k, int32_t K, int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows,
                    int32_t* out_dist, double* out_binary, double* out_cosine, void* workspace,
                    size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0 && K3 >= 0);
  const int mode = (flags & VRQ_SEARCH_PHASE1_ONLY) ? 1 : (flags & VRQ_SEARCH_SHARD) ? 2 : 0;
  const bool run = nq > 0 && n > 0 && K > 0 && (mode != 0 || k > 0);
  if (dim != DIM) {
    // The whole call checks every argument before it launches the scan (at 1024, the ABI-1 behaviour stays:
    // the finish checks its own after the scan), and takes no flag but these two: forcing the matrix-core
    // scan and staging it go through vrq_search3_dim_scan / _finish.
    VRQ_CHECK_ARG(out_count && out_rows && out_dist);
    if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
    if (flags & ~(VRQ_SEARCH_PHASE1_ONLY | VRQ_SEARCH_SCAN_VALU)) return VRQ_EUNSUPPORTED;
    if (nq > 0 && mode != 1) VRQ_CHECK_ARG(out_binary && out_cosine);
    if (run) VRQ_CHECK_ARG(codes && qb && workspace);
    if (run && mode != 1) VRQ_CHECK_ARG(qf && x8 && norms);
  }
  if (run) {
    const int rc = vrq_search3_dim_scan(codes, n, dim, qb, nq, K, flags, workspace, workspace_bytes, stream);
    if (rc != VRQ_OK) return rc;
  }
  return vrq_search3_dim_finish(codes, x8, norms, rescore_row, n, dim, row_offset, qf, nq, k, K, K3, flags, out_count,
                                out_rows, out_dist, out_binary, out_cosine, workspace, workspace_bytes, stream);
}

// ABI 1: the same three at dim 1024 only
int vrq_search3_scan(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                     int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && K >= 0);
  if (dim != DIM) return VRQ_EUNSUPPORTED;
  return vrq_search3_dim_scan(codes, n, dim, qb, nq, K, flags, workspace, workspace_bytes, stream);
}

int vrq_search3_finish(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                       int64_t n, int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t K,
                       int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows, int32_t* out_dist,
                       double* out_binary, double* out_cosine, const void* workspace, size_t workspace_bytes,
                       void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0 && K3 >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist);
  if (dim != DIM) return VRQ_EUNSUPPORTED;
  return vrq_search3_dim_finish(codes, x8, norms, rescore_row, n, dim, row_offset, qf, nq, k, K, K3, flags, out_count,
                                out_rows, out_dist, out_binary, out_cosine, workspace, workspace_bytes, stream);
}

int vrq_search3(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq, int32_t k,
                int32_t K, int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows, int32_t* out_dist,
                double* out_binary, double* out_cosine, void* workspace, size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0 && K3 >= 0);
  if (dim != DIM) return VRQ_EUNSUPPORTED;
  return vrq_search3_dim(codes, x8, norms, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, K3, flags, out_count,
                         out_rows, out_dist, out_binary, out_cosine, workspace, workspace_bytes, stream);
}

// ---- the per-shard call of the row-sharded three-phase search, every dim of vrq_dim_supported ----
size_t vrq_shard_search3_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_dim_workspace_size(n, dim, nq, K);
}

int vrq_shard_search3(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                      int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                      int32_t K, int32_t flags, int32_t* out_count, int64_t* out_rows, int32_t* out_dist,
                      double* out_binary, double* out_cosine, void* workspace, size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && K >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_binary && out_cosine);
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  if (flags & ~(VRQ_SEARCH_SCAN_VALU | VRQ_SEARCH_SCAN_MFMA)) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || K == 0) return fill_empty(nq, K, out_count, out_rows, out_dist, out_binary, out_cosine, s);
  VRQ_CHECK_ARG(codes && qb && workspace && qf && x8 && norms);
  if (dim == DIM)  // the ABI-1 sharded mode (k and K3 are not read there)
    return vrq_search3(codes, x8, norms, rescore_row, n, dim, row_offset, qf, qb, nq, K, K, K,
                       flags | VRQ_SEARCH_SHARD, out_count, out_rows, out_dist, out_binary, out_cosine, workspace,
                       workspace_bytes, stream);
  // the scan of the shape without the shard bit, exactly as vrq_search3_dim_scan runs it, then the shard
  // mode of the runtime-dim finish on the lists it left
  Phase1Route r;
  int rc = route_checked(n, dim / 8, nq, K, flags, workspace_bytes, &r);
  if (rc != VRQ_OK) return rc;
  rc = phase1_launch(r, codes, n, dim / 8, qb, nq, K, workspace, s, flags);
  if (rc != VRQ_OK) return rc;
  const FinishArgs fa = finish_args(x8, norms, rescore_row, row_offset, 0, 0, out_count, out_rows, out_dist,
                                    out_binary, out_cosine, nullptr, K);
  return launch_select(s, nq, workspace, r, K, dim, codes, x8, norms, qf, 2, fa);
}

// ---- introspection: the answers are read out of the route ----
int vrq_scan_kind(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t flags, int64_t* prefix_rows) {
  if (n < 1 || nq < 1 || K < 1) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  Phase1Route r;
  const int rc = phase1_route(n, dim / 8, nq, K, flags, &r);
  if (rc != VRQ_OK) return rc;
  if (prefix_rows) *prefix_rows = r.mfma ? 0 : n;  // (every row goes through the matrix-core pass)
  return r.mfma ? VRQ_SCAN_KIND_MFMA : VRQ_SCAN_KIND_VALU;
}

// the matrix-core plan of a shape; VRQ_EUNSUPPORTED where the wavefront scan runs
static int mfma_route(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t flags, const int64_t* info,
                      Phase1Route* r) {
  if (!info || n < 1 || nq < 1 || K < 1) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  const int rc = phase1_route(n, dim / 8, nq, K, flags, r);
  return rc != VRQ_OK ? rc : r->mfma ? VRQ_OK : VRQ_EUNSUPPORTED;
}

int vrq_scan_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t flags, int64_t* info) {
  Phase1Route r;
  const int rc = mfma_route(n, dim, nq, K, flags, info, &r);
  if (rc != VRQ_OK) return rc;
  const MfmaPlan& p = r.mp;
  info[0] = dim != DIM ? kMfmaKindRowsDim : p.rows ? 1 : p.swap ? 2 : 0;
  info[1] = p.mb;
  info[2] = p.chunk_rows;
  info[3] = p.nchunks;
  info[4] = p.capc;
  info[5] = (int64_t)p.off_cand;
  info[6] = (int64_t)p.off_cnt;
  info[7] = (int64_t)p.off_tau;
  info[8] = p.sample;
  info[9] = p.j;
  info[10] = (int64_t)p.off_suffix;
  info[11] = (int64_t)p.bytes;
  return VRQ_OK;
}

int vrq_scan_sample_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t flags, int64_t* info) {
  Phase1Route r;
  const int rc = mfma_route(n, dim, nq, K, flags, info, &r);
  if (rc != VRQ_OK) return rc;
  const MfmaPlan& p = r.mp;
  info[0] = p.rows_sample;
  info[1] = p.sample_chunks;
  info[2] = p.sample_chunk_rows;
  info[3] = p.sample_stride;
  info[4] = p.sample_tile_stride;
  info[5] = p.dvcols;
  return VRQ_OK;
}

int vrq_merge_shards(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts, const int64_t* rows,
                     const int32_t* dist, const double* s2, const double* s3, int32_t k, int32_t K3,
                     int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_binary,
                     double* out_cosine, int32_t* out_src, void* stream) {
  VRQ_CHECK_ARG(nshards >= 1 && nq >= 0 && K >= 0 && k >= 0 && K3 >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_binary && out_cosine);
  if (K > KMAX || nshards > MAX_LISTS) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (K == 0 || k == 0) return fill_empty(nq, k, out_count, out_rows, out_dist, out_binary, out_cosine, s);
  VRQ_CHECK_ARG(counts && rows && dist && s2 && s3);
  const FinishArgs fa = finish_args(nullptr, nullptr, nullptr, 0, k, K3, out_count, out_rows, out_dist, out_binary,
                                    out_cosine, out_src, k);
  // (the call has no dim: the instances with a bin for every distance up to 2048 serve all of them)
  if (K <= KSMALL && nshards <= LSMALL)
    hipLaunchKernelGGL(merge_shards_kernel<SelDimSmall>, dim3(nq), dim3(SEL_THREADS), 0, s, nshards, K, counts, rows,
                       dist, s2, s3, nq, fa);
  else
    hipLaunchKernelGGL(merge_shards_kernel<SelDimBig>, dim3(nq), dim3(SEL_THREADS), 0, s, nshards, K, counts, rows,
                       dist, s2, s3, nq, fa);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

int vrq_merge_shards2(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts, const int64_t* rows,
                      const int32_t* dist, const double* score, int32_t k, int32_t* out_count, int64_t* out_rows,
                      int32_t* out_dist, double* out_score, int32_t* out_src, void* stream) {
  VRQ_CHECK_ARG(nshards >= 1 && nq >= 0 && K >= 0 && k >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_score);
  if (K > KMAX || nshards > MAX_LISTS) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (K == 0 || k == 0) {
    if (out_src && k && hipMemsetAsync(out_src, 0xff, sizeof(int32_t) * (size_t)nq * k, s) != hipSuccess)
      return VRQ_EHIP;  // -1
    return fill_empty(nq, k, out_count, out_rows, out_dist, out_score, nullptr, s);
  }
  VRQ_CHECK_ARG(counts && rows && dist && score);
  if (K <= KSMALL && nshards <= LSMALL)
    hipLaunchKernelGGL(merge_shards2_kernel<Sel2Small>, dim3(nq), dim3(SEL_THREADS), 0, s, nshards, K, counts, rows,
                       dist, score, nq, k, out_count, out_rows, out_dist, out_score, out_src);
  else
    hipLaunchKernelGGL(merge_shards2_kernel<Sel2Big>, dim3(nq), dim3(SEL_THREADS), 0, s, nshards, K, counts, rows,
                       dist, score, nq, k, out_count, out_rows, out_dist, out_score, out_src);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// ---- stand-alone rescoring: every dim of vrq_dim_supported; the ABI-1 names take 1024 only ----
int vrq_rescore_binary_dim(const float* qf, int32_t nq, int32_t dim, const uint8_t* codes, int64_t n,
                           const int64_t* cand_rows, int32_t ncand, double* out, void* stream) {
  VRQ_CHECK_ARG(nq >= 0 && ncand >= 0 && n >= 0);
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  if ((int64_t)nq * ncand == 0) return VRQ_OK;
  VRQ_CHECK_ARG(qf && codes && cand_rows && out);
  return launch_rescore(0, qf, nq, dim, codes, nullptr, nullptr, n, cand_rows, ncand, out, (hipStream_t)stream);
}

int vrq_rescore_int8_cosine_dim(const float* qf, int32_t nq, int32_t dim, const int8_t* x8, const double* norms,
                                int64_t n, const int64_t* cand_rows, int32_t ncand, double* out, void* stream) {
  VRQ_CHECK_ARG(nq >= 0 && ncand >= 0 && n >= 0);
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  if ((int64_t)nq * ncand == 0) return VRQ_OK;
  VRQ_CHECK_ARG(qf && x8 && norms && cand_rows && out);
  return launch_rescore(1, qf, nq, dim, nullptr, x8, norms, n, cand_rows, ncand, out, (hipStream_t)stream);
}

int vrq_rescore_binary(const float* qf, int32_t nq, int32_t dim, const uint8_t* codes, int64_t n,
                       const int64_t* cand_rows, int32_t ncand, double* out, void* stream) {
  VRQ_CHECK_ARG(nq >= 0 && ncand >= 0 && n >= 0);
  if (dim != DIM) return VRQ_EUNSUPPORTED;
  return vrq_rescore_binary_dim(qf, nq, dim, codes, n, cand_rows, ncand, out, stream);
}

int vrq_rescore_int8_cosine(const float* qf, int32_t nq, int32_t dim, const int8_t* x8, const double* norms,
                            int64_t n, const int64_t* cand_rows, int32_t ncand, double* out, void* stream) {
  VRQ_CHECK_ARG(nq >= 0 && ncand >= 0 && n >= 0);
  if (dim != DIM) return VRQ_EUNSUPPORTED;
  return vrq_rescore_int8_cosine_dim(qf, nq, dim, x8, norms, n, cand_rows, ncand, out, stream);
}

int vrq_dim_supported(int32_t dim) {
  return dim == DIM || (dim > 0 && dim % 8 == 0 && dim_code_bytes_supported(dim / 8)) ? 1 : 0;
}

// ---- the fused two-phase search (every dim of vrq_dim_supported) ----
static bool search2_mode_ok(int mode) {
  return (mode >= VRQ_ENC_INT8_GLOBAL && mode <= VRQ_ENC_INT4_LOCAL) || mode == VRQ_RESCORE_F32 ||
         mode == VRQ_RESCORE_SIGNED_BINARY;
}

int vrq_search2_finish(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                       const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                       int32_t nq, int32_t k, int32_t K, int32_t flags, int32_t* out_count, int64_t* out_rows,
                       int32_t* out_dist, double* out_score, const void* workspace, size_t workspace_bytes,
                       void* stream) {
  VRQ_CHECK_ARG(search2_mode_ok(mode));
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_score);
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  if (flags & ~(VRQ_SEARCH_SCAN_VALU | VRQ_SEARCH_SCAN_MFMA)) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || K == 0 || k == 0) return fill_empty(nq, k, out_count, out_rows, out_dist, out_score, nullptr, s);
  VRQ_CHECK_ARG(codes && workspace && qf && q);
  if (mode == VRQ_ENC_INT8_LOCAL || mode == VRQ_ENC_INT4_LOCAL) VRQ_CHECK_ARG(minmax);
  Phase1Route r;
  const int rc = route_checked(n, dim / 8, nq, K, flags, workspace_bytes, &r);
  if (rc != VRQ_OK) return rc;
  const Finish2Args fa{mode, q, minmax, limit, rescore_row, row_offset, k, out_count, out_rows, out_dist, out_score,
                       false};
  return launch_select2(s, nq, workspace, r, K, dim, qf, fa);
}

int vrq_search2(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, int32_t* out_count,
                int64_t* out_rows, int32_t* out_dist, double* out_score, void* workspace, size_t workspace_bytes,
                void* stream) {
  VRQ_CHECK_ARG(search2_mode_ok(mode));
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_score);
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  if (flags & ~(VRQ_SEARCH_SCAN_VALU | VRQ_SEARCH_SCAN_MFMA)) return VRQ_EUNSUPPORTED;
  if (nq > 0 && n > 0 && K > 0 && k > 0) {
    VRQ_CHECK_ARG(codes && qb && workspace && qf && q);
    if (mode == VRQ_ENC_INT8_LOCAL || mode == VRQ_ENC_INT4_LOCAL) VRQ_CHECK_ARG(minmax);
    const int rc = vrq_search3_dim_scan(codes, n, dim, qb, nq, K, flags, workspace, workspace_bytes, stream);
    if (rc != VRQ_OK) return rc;
  }
  return vrq_search2_finish(mode, codes, q, minmax, limit, rescore_row, n, dim, row_offset, qf, nq, k, K, flags,
                            out_count, out_rows, out_dist, out_score, workspace, workspace_bytes, stream);
}

// ---- the per-shard call of the row-sharded two-phase search ----
size_t vrq_shard_search2_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_dim_workspace_size(n, dim, nq, K);
}

int vrq_shard_search2(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                      const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                      const uint8_t* qb, int32_t nq, int32_t K, int32_t flags, int32_t* out_count, int64_t* out_rows,
                      int32_t* out_dist, double* out_score, void* workspace, size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(search2_mode_ok(mode));
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && K >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_score);
  if (!vrq_dim_supported(dim) || K > KMAX) return VRQ_EUNSUPPORTED;
  if (flags & ~(VRQ_SEARCH_SCAN_VALU | VRQ_SEARCH_SCAN_MFMA)) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || K == 0) return fill_empty(nq, K, out_count, out_rows, out_dist, out_score, nullptr, s);
  VRQ_CHECK_ARG(codes && qb && workspace && qf && q);
  if (mode == VRQ_ENC_INT8_LOCAL || mode == VRQ_ENC_INT4_LOCAL) VRQ_CHECK_ARG(minmax);
  Phase1Route r;
  int rc = route_checked(n, dim / 8, nq, K, flags, workspace_bytes, &r);
  if (rc != VRQ_OK) return rc;
  rc = phase1_launch(r, codes, n, dim / 8, qb, nq, K, workspace, s, flags);
  if (rc != VRQ_OK) return rc;
  const Finish2Args fa{mode, q, minmax, limit, rescore_row, row_offset, K, out_count, out_rows, out_dist, out_score,
                       true};
  return launch_select2(s, nq, workspace, r, K, dim, qf, fa);
}

// ---- K up to VRQ_K_LARGE_MAX: the counting scan K1h (hamming_count.hip) + the large finish ----
int vrq_scan_large_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int64_t* info) {
  if (!info || n < 1 || nq < 1 || K < 1) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  CountPlan p;
  const int rc = count_route(n, dim / 8, nq, K, VRQ_LARGE_ENGINE_VALU, false, &p);
  if (rc != VRQ_OK) return rc;
  info[0] = p.chunk_rows;
  info[1] = p.nchunks;
  info[2] = p.qpw;
  info[3] = 0;  // (no bounding prefix: every distance is counted)
  info[4] = (int64_t)p.off_hist;
  info[5] = (int64_t)p.off_tc;
  info[6] = (int64_t)p.off_lists;
  info[7] = (int64_t)p.bytes;
  return VRQ_OK;
}

// the workspace of a call of the counting scan: K1h's own (*_large, *_filtered), or either engine's (*_batch)
static size_t count_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K, bool either) {
  CountPlan p;
  const int engine = either ? VRQ_LARGE_ENGINE_AUTO : VRQ_LARGE_ENGINE_VALU;
  return vrq_dim_supported(dim) && count_route(n, dim / 8, nq, K, engine, either, &p) == VRQ_OK ? p.need : 0;
}

size_t vrq_search3_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return count_workspace_size(n, dim, nq, K, false);
}

size_t vrq_search2_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_large_workspace_size(n, dim, nq, K);
}

size_t vrq_hamming_topk_large_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k) {
  return code_bytes > 0 && code_bytes <= 256 ? vrq_search3_large_workspace_size(n, code_bytes * 8, nq, k) : 0;
}

// the filtered calls need no more: the bitmap is the caller's
size_t vrq_search3_filtered_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_large_workspace_size(n, dim, nq, K);
}

size_t vrq_search2_filtered_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_large_workspace_size(n, dim, nq, K);
}

size_t vrq_hamming_topk_filtered_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k) {
  return vrq_hamming_topk_large_workspace_size(n, code_bytes, nq, k);
}

size_t vrq_scan_filtered_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_large_workspace_size(n, dim, nq, K);
}

// What a call asks of the counting scan, one value per family of entry points.  The filtered calls
// (vrq_*_filtered) are the *_large calls with a row bitmap handed to K1h; the batch calls (vrq_*_batch) are the
// same calls again with a choice of the scan's engine, a workspace that covers either engine, and a bitmap
// that may be null (no filter).  The per-query calls (vrq_*_perquery) are the batch calls with nsets bitmaps and
// a set id per query in place of the one bitmap.
struct CountCall {
  int engine = VRQ_LARGE_ENGINE_VALU;  // VRQ_LARGE_ENGINE_*; a *_large / *_filtered call runs K1h
  bool either = false;                 // the workspace covers either engine (*_batch, *_perquery)
  bool filtered = false;               // the call reads `filter.allow`
  bool perquery = false;               // the call reads `filter.query_set`
  RowFilter filter;
};
static CountCall filtered_call(const uint64_t* allow) {
  return {VRQ_LARGE_ENGINE_VALU, false, true, false, RowFilter{allow, 0, 0, nullptr}};
}
static CountCall batch_call(const uint64_t* allow, int engine) {
  return {engine, true, allow != nullptr, false, RowFilter{allow, 0, 0, nullptr}};
}
static CountCall perquery_call(const uint64_t* allow, int nsets, int64_t set_words, const int32_t* query_set,
                               int engine) {
  return {engine, true, true, true, RowFilter{allow, nsets, set_words, query_set}};
}
static bool engine_ok(int engine) { return engine >= VRQ_LARGE_ENGINE_AUTO && engine <= VRQ_LARGE_ENGINE_MFMA; }

// The route of a call that scans (n, nq, K >= 1), after the other pointers a non-empty call reads: the
// bitmap's check, the plan and the workspace check, before anything is launched.  (AUTO's choice does not
// depend on the filter: one table entry per code size serves both kinds.)
static int count_route_checked(int64_t n, int cb, int nq, int K, const CountCall& c, size_t workspace_bytes,
                               CountPlan* p) {
  if (c.filtered) VRQ_CHECK_ARG(c.filter.allow && ((uintptr_t)c.filter.allow & 7) == 0);
  if (c.perquery) {
    VRQ_CHECK_ARG(c.filter.query_set && ((uintptr_t)c.filter.query_set & 3) == 0);
    VRQ_CHECK_ARG(c.filter.nsets >= 1 && c.filter.set_words >= (n + 63) / 64);
  }
  const int rc = count_route(n, cb, nq, K, c.engine, c.either, p);
  if (rc != VRQ_OK) return rc;
  return workspace_bytes < p->need ? VRQ_EWORKSPACE : VRQ_OK;
}

static int scan_large_impl(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                           int32_t stages, void* workspace, size_t workspace_bytes, void* stream,
                           const CountCall& call) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && K >= 0);
  if (!vrq_dim_supported(dim) || K > VRQ_K_LARGE_MAX) return VRQ_EUNSUPPORTED;
  if (stages & ~kLargeStageAll) return VRQ_EUNSUPPORTED;
  if (nq == 0 || n == 0 || K == 0) return VRQ_OK;
  VRQ_CHECK_ARG(codes && qb && workspace);
  CountPlan p;
  const int rc = count_route_checked(n, dim / 8, nq, K, call, workspace_bytes, &p);
  if (rc != VRQ_OK) return rc;
  return count_route_launch(p, codes, n, dim / 8, qb, nq, K, (uint8_t*)workspace, (hipStream_t)stream, stages,
                            call.filter);
}

int vrq_scan_large(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                   int32_t stages, void* workspace, size_t workspace_bytes, void* stream) {
  return scan_large_impl(codes, n, dim, qb, nq, K, stages, workspace, workspace_bytes, stream, CountCall{});
}

int vrq_scan_filtered(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                      int32_t stages, const uint64_t* allow, void* workspace, size_t workspace_bytes, void* stream) {
  return scan_large_impl(codes, n, dim, qb, nq, K, stages, workspace, workspace_bytes, stream,
                         filtered_call(allow));
}

static int hamming_topk_large_impl(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                                   const uint8_t* queries, int32_t nq, int32_t k, int32_t* out_dist,
                                   int64_t* out_rows, void* workspace, size_t workspace_bytes, void* stream,
                                   const CountCall& call) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && out_dist && out_rows);
  if (code_bytes <= 0 || code_bytes > 256 || !vrq_dim_supported(code_bytes * 8) || k > VRQ_K_LARGE_MAX)
    return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || k == 0) return fill_empty(nq, k, nullptr, out_rows, out_dist, nullptr, nullptr, s);
  VRQ_CHECK_ARG(codes && queries && workspace);
  CountPlan p;
  int rc = count_route_checked(n, code_bytes, nq, k, call, workspace_bytes, &p);
  if (rc != VRQ_OK) return rc;
  uint8_t* ws = (uint8_t*)workspace;
  rc = count_route_launch(p, codes, n, code_bytes, queries, nq, k, ws, s, 0, call.filter);
  if (rc != VRQ_OK) return rc;
  return large_sort_launch(s, nq, (uint64_t*)(ws + p.off_lists), k, (int32_t*)(ws + p.off_kp), true, row_offset,
                           nullptr, out_rows, out_dist);
}

int vrq_hamming_topk_large(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                           const uint8_t* queries, int32_t nq, int32_t k, int32_t* out_dist, int64_t* out_rows,
                           void* workspace, size_t workspace_bytes, void* stream) {
  return hamming_topk_large_impl(codes, n, code_bytes, row_offset, queries, nq, k, out_dist, out_rows, workspace,
                                 workspace_bytes, stream, CountCall{});
}

int vrq_hamming_topk_filtered(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                              const uint8_t* queries, int32_t nq, int32_t k, const uint64_t* allow,
                              int32_t* out_dist, int64_t* out_rows, void* workspace, size_t workspace_bytes,
                              void* stream) {
  return hamming_topk_large_impl(codes, n, code_bytes, row_offset, queries, nq, k, out_dist, out_rows, workspace,
                                 workspace_bytes, stream, filtered_call(allow));
}

static int search3_large_impl(const uint8_t* codes, const int8_t* x8, const double* norms,
                              const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset,
                              const float* qf, const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t K3,
                              int32_t flags, int32_t* out_count, int64_t* out_rows, int32_t* out_dist,
                              double* out_binary, double* out_cosine, void* workspace, size_t workspace_bytes,
                              void* stream, const CountCall& call) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0 && K3 >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist);
  if (!vrq_dim_supported(dim) || K > VRQ_K_LARGE_MAX || k > VRQ_K_LARGE_MAX) return VRQ_EUNSUPPORTED;
  if (flags & ~VRQ_SEARCH_PHASE1_ONLY) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const bool p1 = flags & VRQ_SEARCH_PHASE1_ONLY;
  const int kout = p1 ? K : k;
  if (nq == 0) return VRQ_OK;
  if (!p1) VRQ_CHECK_ARG(out_binary && out_cosine);
  if (n == 0 || K == 0 || (!p1 && k == 0))
    return fill_empty(nq, kout, out_count, out_rows, out_dist, out_binary, out_cosine, s);
  VRQ_CHECK_ARG(codes && qb && workspace);
  if (!p1) VRQ_CHECK_ARG(qf && x8 && norms);
  CountPlan p;
  int rc = count_route_checked(n, dim / 8, nq, K, call, workspace_bytes, &p);
  if (rc != VRQ_OK) return rc;
  uint8_t* ws = (uint8_t*)workspace;
  uint64_t* lists = (uint64_t*)(ws + p.off_lists);
  int32_t* kp = (int32_t*)(ws + p.off_kp);
  int32_t* ord = (int32_t*)(ws + p.off_ord);
  double* s2 = (double*)(ws + p.off_s2);
  double* s3 = (double*)(ws + p.off_s3);
  rc = count_route_launch(p, codes, n, dim / 8, qb, nq, K, ws, s, 0, call.filter);
  if (rc != VRQ_OK) return rc;
  rc = large_sort_launch(s, nq, lists, K, kp, p1, row_offset, out_count, out_rows, out_dist);
  if (rc != VRQ_OK || p1) return rc;
  // Phase II of every candidate, its stable order, the first K3
  LargeScoreArgs sa{};
  sa.which = 0;
  sa.lists = lists;
  sa.kp = kp;
  sa.K = K;
  sa.limit = K;
  sa.remap = rescore_row;
  sa.codes = codes;
  sa.x8 = x8;
  sa.norms = norms;
  sa.out = s2;
  rc = large_score_launch(s, nq, qf, dim, sa);
  if (rc != VRQ_OK) return rc;
  LargeOrderArgs oa{};
  oa.sc = s2;
  oa.kp = kp;
  oa.K = K;
  oa.limit = K;
  oa.ord_out = ord;
  oa.keep = K3;
  rc = large_order_launch(s, nq, oa);
  if (rc != VRQ_OK) return rc;
  // Phase III of those, by position in the Phase-II order; its stable order, the first k
  sa.which = 1;
  sa.ord = ord;
  sa.limit = K3;
  sa.out = s3;
  rc = large_score_launch(s, nq, qf, dim, sa);
  if (rc != VRQ_OK) return rc;
  LargeOrderArgs fa{};
  fa.sc = s3;
  fa.kp = kp;
  fa.K = K;
  fa.limit = K3;
  fa.ord = ord;
  fa.lists = lists;
  fa.s2 = s2;
  fa.row_offset = row_offset;
  fa.k = k;
  fa.out_count = out_count;
  fa.out_rows = out_rows;
  fa.out_dist = out_dist;
  fa.out_s2 = out_binary;
  fa.out_s3 = out_cosine;
  return large_order_launch(s, nq, fa);
}

int vrq_search3_large(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                      int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                      int32_t k, int32_t K, int32_t K3, int32_t flags, int32_t* out_count, int64_t* out_rows,
                      int32_t* out_dist, double* out_binary, double* out_cosine, void* workspace,
                      size_t workspace_bytes, void* stream) {
  return search3_large_impl(codes, x8, norms, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, K3, flags,
                            out_count, out_rows, out_dist, out_binary, out_cosine, workspace, workspace_bytes, stream,
                            CountCall{});
}

int vrq_search3_filtered(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                         int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                         int32_t k, int32_t K, int32_t K3, int32_t flags, const uint64_t* allow, int32_t* out_count,
                         int64_t* out_rows, int32_t* out_dist, double* out_binary, double* out_cosine,
                         void* workspace, size_t workspace_bytes, void* stream) {
  return search3_large_impl(codes, x8, norms, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, K3, flags,
                            out_count, out_rows, out_dist, out_binary, out_cosine, workspace, workspace_bytes, stream,
                            filtered_call(allow));
}

static int search2_large_impl(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                              const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset,
                              const float* qf, const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags,
                              int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_score,
                              void* workspace, size_t workspace_bytes, void* stream, const CountCall& call) {
  VRQ_CHECK_ARG(search2_mode_ok(mode));
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && k >= 0 && K >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_score);
  if (!vrq_dim_supported(dim) || K > VRQ_K_LARGE_MAX || k > VRQ_K_LARGE_MAX) return VRQ_EUNSUPPORTED;
  if (mode == VRQ_RESCORE_SIGNED_BINARY && dim % 128 != 0) return VRQ_EUNSUPPORTED;
  if (flags) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || K == 0 || k == 0) return fill_empty(nq, k, out_count, out_rows, out_dist, out_score, nullptr, s);
  VRQ_CHECK_ARG(codes && qb && workspace && qf && q);
  if (mode == VRQ_ENC_INT8_LOCAL || mode == VRQ_ENC_INT4_LOCAL) VRQ_CHECK_ARG(minmax);
  CountPlan p;
  int rc = count_route_checked(n, dim / 8, nq, K, call, workspace_bytes, &p);
  if (rc != VRQ_OK) return rc;
  uint8_t* ws = (uint8_t*)workspace;
  uint64_t* lists = (uint64_t*)(ws + p.off_lists);
  int32_t* kp = (int32_t*)(ws + p.off_kp);
  double* s2 = (double*)(ws + p.off_s2);
  rc = count_route_launch(p, codes, n, dim / 8, qb, nq, K, ws, s, 0, call.filter);
  if (rc != VRQ_OK) return rc;
  rc = large_sort_launch(s, nq, lists, K, kp, false, 0, nullptr, nullptr, nullptr);
  if (rc != VRQ_OK) return rc;
  LargeScoreArgs sa{};
  sa.which = 2;
  sa.lists = lists;
  sa.kp = kp;
  sa.K = K;
  sa.limit = K;
  sa.remap = rescore_row;
  sa.mode = mode;
  sa.dq = q;
  sa.minmax = minmax;
  sa.dlimit = limit;
  sa.out = s2;
  rc = large_score_launch(s, nq, qf, dim, sa);
  if (rc != VRQ_OK) return rc;
  LargeOrderArgs fa{};
  fa.sc = s2;
  fa.kp = kp;
  fa.K = K;
  fa.limit = K;
  fa.lists = lists;
  fa.s2 = s2;
  fa.row_offset = row_offset;
  fa.k = k;
  fa.out_count = out_count;
  fa.out_rows = out_rows;
  fa.out_dist = out_dist;
  fa.out_s2 = out_score;
  return large_order_launch(s, nq, fa);
}

int vrq_search2_large(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                      const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                      const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, int32_t* out_count,
                      int64_t* out_rows, int32_t* out_dist, double* out_score, void* workspace,
                      size_t workspace_bytes, void* stream) {
  return search2_large_impl(mode, codes, q, minmax, limit, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, flags,
                            out_count, out_rows, out_dist, out_score, workspace, workspace_bytes, stream, CountCall{});
}

int vrq_search2_filtered(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                         const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                         const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, const uint64_t* allow,
                         int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_score,
                         void* workspace, size_t workspace_bytes, void* stream) {
  return search2_large_impl(mode, codes, q, minmax, limit, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, flags,
                            out_count, out_rows, out_dist, out_score, workspace, workspace_bytes, stream,
                            filtered_call(allow));
}

// ---- the batch calls: the *_large / *_filtered calls with the scan's engine chosen (K1h or K1hm) ----
// (the bitmap's alignment is checked where the *_filtered calls check theirs: after the empty-shape returns)
int vrq_large_engine(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t filtered) {
  if (n < 1 || nq < 1 || K < 1) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  (void)filtered;  // one minimum batch per code size serves both kinds of scan, so the plan call needs no such axis
  CountPlan p;
  const int rc = count_route(n, dim / 8, nq, K, VRQ_LARGE_ENGINE_AUTO, true, &p);
  return rc != VRQ_OK ? rc : p.engine;
}

size_t vrq_search3_batch_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return count_workspace_size(n, dim, nq, K, true);
}

size_t vrq_search2_batch_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_batch_workspace_size(n, dim, nq, K);
}

size_t vrq_scan_batch_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_batch_workspace_size(n, dim, nq, K);
}

size_t vrq_hamming_topk_batch_workspace_size(int64_t n, int32_t code_bytes, int32_t nq, int32_t k) {
  return code_bytes > 0 && code_bytes <= 256 ? vrq_search3_batch_workspace_size(n, code_bytes * 8, nq, k) : 0;
}

int vrq_scan_batch_plan(int64_t n, int32_t dim, int32_t nq, int32_t K, int32_t engine, int64_t* info) {
  if (!info || n < 1 || nq < 1 || K < 1 || !engine_ok(engine)) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  CountPlan p;
  const int rc = count_route(n, dim / 8, nq, K, engine, true, &p);
  if (rc != VRQ_OK) return rc;
  info[0] = p.engine;
  info[1] = p.chunk_rows;
  info[2] = p.nchunks;
  info[3] = p.qpw;
  info[4] = p.nqb;
  info[5] = p.flush_rows;
  info[6] = (int64_t)p.off_hist;
  info[7] = (int64_t)p.off_tc;
  info[8] = (int64_t)p.off_lists;
  info[9] = (int64_t)p.need;
  return VRQ_OK;
}

int vrq_scan_batch(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                   int32_t stages, const uint64_t* allow, void* workspace, size_t workspace_bytes, void* stream,
                   int32_t engine) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return scan_large_impl(codes, n, dim, qb, nq, K, stages, workspace, workspace_bytes, stream,
                         batch_call(allow, engine));
}

int vrq_hamming_topk_batch(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                           const uint8_t* queries, int32_t nq, int32_t k, const uint64_t* allow, int32_t* out_dist,
                           int64_t* out_rows, void* workspace, size_t workspace_bytes, void* stream,
                           int32_t engine) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return hamming_topk_large_impl(codes, n, code_bytes, row_offset, queries, nq, k, out_dist, out_rows, workspace,
                                 workspace_bytes, stream, batch_call(allow, engine));
}

int vrq_search3_batch(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                      int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                      int32_t k, int32_t K, int32_t K3, int32_t flags, const uint64_t* allow, int32_t* out_count,
                      int64_t* out_rows, int32_t* out_dist, double* out_binary, double* out_cosine,
                      void* workspace, size_t workspace_bytes, void* stream, int32_t engine) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return search3_large_impl(codes, x8, norms, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, K3, flags,
                            out_count, out_rows, out_dist, out_binary, out_cosine, workspace, workspace_bytes, stream,
                            batch_call(allow, engine));
}

int vrq_search2_batch(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                      const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                      const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, const uint64_t* allow,
                      int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_score,
                      void* workspace, size_t workspace_bytes, void* stream, int32_t engine) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return search2_large_impl(mode, codes, q, minmax, limit, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, flags,
                            out_count, out_rows, out_dist, out_score, workspace, workspace_bytes, stream,
                            batch_call(allow, engine));
}

// ---- the per-query calls: the batch calls with a set of bitmaps and one set id per query ----
int vrq_scan_perquery(const uint8_t* codes, int64_t n, int32_t dim, const uint8_t* qb, int32_t nq, int32_t K,
                      int32_t stages, const uint64_t* allow, void* workspace, size_t workspace_bytes, void* stream,
                      int32_t engine, int32_t nsets, int64_t set_words, const int32_t* query_set) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return scan_large_impl(codes, n, dim, qb, nq, K, stages, workspace, workspace_bytes, stream,
                         perquery_call(allow, nsets, set_words, query_set, engine));
}

int vrq_hamming_topk_perquery(const uint8_t* codes, int64_t n, int32_t code_bytes, int64_t row_offset,
                              const uint8_t* queries, int32_t nq, int32_t k, const uint64_t* allow,
                              int32_t* out_dist, int64_t* out_rows, void* workspace, size_t workspace_bytes,
                              void* stream, int32_t engine, int32_t nsets, int64_t set_words,
                              const int32_t* query_set) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return hamming_topk_large_impl(codes, n, code_bytes, row_offset, queries, nq, k, out_dist, out_rows, workspace,
                                 workspace_bytes, stream, perquery_call(allow, nsets, set_words, query_set, engine));
}

int vrq_search3_perquery(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                         int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb, int32_t nq,
                         int32_t k, int32_t K, int32_t K3, int32_t flags, const uint64_t* allow, int32_t* out_count,
                         int64_t* out_rows, int32_t* out_dist, double* out_binary, double* out_cosine,
                         void* workspace, size_t workspace_bytes, void* stream, int32_t engine, int32_t nsets,
                         int64_t set_words, const int32_t* query_set) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return search3_large_impl(codes, x8, norms, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, K3, flags,
                            out_count, out_rows, out_dist, out_binary, out_cosine, workspace, workspace_bytes, stream,
                            perquery_call(allow, nsets, set_words, query_set, engine));
}

int vrq_search2_perquery(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                         const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                         const uint8_t* qb, int32_t nq, int32_t k, int32_t K, int32_t flags, const uint64_t* allow,
                         int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_score,
                         void* workspace, size_t workspace_bytes, void* stream, int32_t engine, int32_t nsets,
                         int64_t set_words, const int32_t* query_set) {
  VRQ_CHECK_ARG(engine_ok(engine));
  return search2_large_impl(mode, codes, q, minmax, limit, rescore_row, n, dim, row_offset, qf, qb, nq, k, K, flags,
                            out_count, out_rows, out_dist, out_score, workspace, workspace_bytes, stream,
                            perquery_call(allow, nsets, set_words, query_set, engine));
}

// ---- the per-shard calls for K up to VRQ_K_LARGE_MAX: K1h, the sort, the scores of every candidate ----
size_t vrq_shard_search3_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_large_workspace_size(n, dim, nq, K);
}

size_t vrq_shard_search2_large_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t K) {
  return vrq_search3_large_workspace_size(n, dim, nq, K);
}

// scan + sort into the caller's [nq][K] rows / dist / count; leaves `sa` ready to score every position
static int large_shard_phase1(const CountPlan& p, const uint8_t* codes, int64_t n, int32_t dim, int64_t row_offset,
                              const uint8_t* qb, int32_t nq, int32_t K, const int64_t* rescore_row,
                              int32_t* out_count, int64_t* out_rows, int32_t* out_dist, uint8_t* ws, hipStream_t s,
                              LargeScoreArgs* sa) {
  uint64_t* lists = (uint64_t*)(ws + p.off_lists);
  int32_t* kp = (int32_t*)(ws + p.off_kp);
  int rc = count_route_launch(p, codes, n, dim / 8, qb, nq, K, ws, s, 0, RowFilter{});
  if (rc != VRQ_OK) return rc;
  rc = large_sort_launch(s, nq, lists, K, kp, true, row_offset, out_count, out_rows, out_dist);
  sa->lists = lists;
  sa->kp = kp;
  sa->K = K;
  sa->limit = K;
  sa->remap = rescore_row;
  sa->pad = true;
  return rc;
}

int vrq_shard_search3_large(const uint8_t* codes, const int8_t* x8, const double* norms, const int64_t* rescore_row,
                            int64_t n, int32_t dim, int64_t row_offset, const float* qf, const uint8_t* qb,
                            int32_t nq, int32_t K, int32_t flags, int32_t* out_count, int64_t* out_rows,
                            int32_t* out_dist, double* out_binary, double* out_cosine, void* workspace,
                            size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && K >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_binary && out_cosine);
  if (!vrq_dim_supported(dim) || K > VRQ_K_LARGE_MAX) return VRQ_EUNSUPPORTED;
  if (flags) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || K == 0) return fill_empty(nq, K, out_count, out_rows, out_dist, out_binary, out_cosine, s);
  VRQ_CHECK_ARG(codes && qb && workspace && qf && x8 && norms);
  CountPlan p;
  int rc = count_route_checked(n, dim / 8, nq, K, CountCall{}, workspace_bytes, &p);
  if (rc != VRQ_OK) return rc;
  LargeScoreArgs sa{};
  rc = large_shard_phase1(p, codes, n, dim, row_offset, qb, nq, K, rescore_row, out_count, out_rows, out_dist,
                          (uint8_t*)workspace, s, &sa);
  if (rc != VRQ_OK) return rc;
  sa.codes = codes;
  sa.x8 = x8;
  sa.norms = norms;
  sa.which = 0;
  sa.out = out_binary;
  rc = large_score_launch(s, nq, qf, dim, sa);
  if (rc != VRQ_OK) return rc;
  sa.which = 1;
  sa.out = out_cosine;
  return large_score_launch(s, nq, qf, dim, sa);
}

int vrq_shard_search2_large(int32_t mode, const uint8_t* codes, const void* q, const double* minmax, double limit,
                            const int64_t* rescore_row, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                            const uint8_t* qb, int32_t nq, int32_t K, int32_t flags, int32_t* out_count,
                            int64_t* out_rows, int32_t* out_dist, double* out_score, void* workspace,
                            size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(search2_mode_ok(mode));
  VRQ_CHECK_ARG(n >= 0 && nq >= 0 && K >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_score);
  if (!vrq_dim_supported(dim) || K > VRQ_K_LARGE_MAX) return VRQ_EUNSUPPORTED;
  if (mode == VRQ_RESCORE_SIGNED_BINARY && dim % 128 != 0) return VRQ_EUNSUPPORTED;
  if (flags) return VRQ_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (n == 0 || K == 0) return fill_empty(nq, K, out_count, out_rows, out_dist, out_score, nullptr, s);
  VRQ_CHECK_ARG(codes && qb && workspace && qf && q);
  if (mode == VRQ_ENC_INT8_LOCAL || mode == VRQ_ENC_INT4_LOCAL) VRQ_CHECK_ARG(minmax);
  CountPlan p;
  int rc = count_route_checked(n, dim / 8, nq, K, CountCall{}, workspace_bytes, &p);
  if (rc != VRQ_OK) return rc;
  LargeScoreArgs sa{};
  rc = large_shard_phase1(p, codes, n, dim, row_offset, qb, nq, K, rescore_row, out_count, out_rows, out_dist,
                          (uint8_t*)workspace, s, &sa);
  if (rc != VRQ_OK) return rc;
  sa.which = 2;
  sa.mode = mode;
  sa.dq = q;
  sa.minmax = minmax;
  sa.dlimit = limit;
  sa.out = out_score;
  return large_score_launch(s, nq, qf, dim, sa);
}

// ---- the merge of the per-shard outputs for K up to VRQ_K_LARGE_MAX ----
size_t vrq_merge_shards_large_workspace_size(int32_t nshards, int32_t nq, int32_t K) {
  MergePlan p;
  return merge_plan(nshards, nq, K, &p) ? p.bytes : 0;
}

// the arguments both merges share, checked before anything is launched; *run = false: nothing to merge
static int merge_large_checked(int32_t nshards, int32_t nq, int32_t K, int32_t k, const void* counts,
                               const void* rows, const void* dist, const void* sc_a, const void* sc_b,
                               const void* workspace, size_t workspace_bytes, MergePlan* p, bool* run) {
  *run = false;
  if (K > VRQ_K_LARGE_MAX || k > VRQ_K_LARGE_MAX || nshards > MAX_LISTS) return VRQ_EUNSUPPORTED;
  if (nq == 0 || K == 0 || k == 0) return VRQ_OK;
  VRQ_CHECK_ARG(counts && rows && dist && sc_a && sc_b && workspace);
  if (!merge_plan(nshards, nq, K, p)) return VRQ_EUNSUPPORTED;
  if (workspace_bytes < p->bytes) return VRQ_EWORKSPACE;
  *run = true;
  return VRQ_OK;
}

static int fill_empty_merge(int32_t nq, int32_t k, int32_t* out_count, int64_t* out_rows, int32_t* out_dist,
                            double* out_a, double* out_b, int32_t* out_src, hipStream_t s) {
  if (out_src && k && hipMemsetAsync(out_src, 0xff, sizeof(int32_t) * (size_t)nq * k, s) != hipSuccess)
    return VRQ_EHIP;  // -1
  return fill_empty(nq, k, out_count, out_rows, out_dist, out_a, out_b, s);
}

int vrq_merge_shards_large(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts, const int64_t* rows,
                           const int32_t* dist, const double* s2, const double* s3, int32_t k, int32_t K3,
                           int32_t* out_count, int64_t* out_rows, int32_t* out_dist, double* out_binary,
                           double* out_cosine, int32_t* out_src, void* workspace, size_t workspace_bytes,
                           void* stream) {
  VRQ_CHECK_ARG(nshards >= 1 && nq >= 0 && K >= 0 && k >= 0 && K3 >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_binary && out_cosine);
  MergePlan p;
  bool run;
  int rc = merge_large_checked(nshards, nq, K, k, counts, rows, dist, s2, s3, workspace, workspace_bytes, &p, &run);
  if (rc != VRQ_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (!run) return fill_empty_merge(nq, k, out_count, out_rows, out_dist, out_binary, out_cosine, out_src, s);
  uint8_t* ws = (uint8_t*)workspace;
  MergeSelectArgs ma{nshards, K, nq, counts, rows, dist, s2, s3, (uint64_t*)(ws + p.off_keys),
                     (int32_t*)(ws + p.off_src), (double*)(ws + p.off_w2), (double*)(ws + p.off_w3),
                     (int32_t*)(ws + p.off_kp)};
  rc = merge_select_launch(s, ma);
  if (rc != VRQ_OK) return rc;
  // the stable order by s2 and the first K3 of it, with their s3 by position
  int32_t* ord = (int32_t*)(ws + p.off_ord);
  double* w3p = (double*)(ws + p.off_w3p);
  LargeOrderArgs oa{};
  oa.sc = ma.w2;
  oa.kp = ma.kp;
  oa.K = K;
  oa.limit = K;
  oa.ord_out = ord;
  oa.keep = K3;
  oa.carry_in = ma.w3;
  oa.carry_out = w3p;
  rc = large_order_launch(s, nq, oa);
  if (rc != VRQ_OK) return rc;
  LargeOrderArgs fa{};
  fa.sc = w3p;
  fa.kp = ma.kp;
  fa.K = K;
  fa.limit = K3;
  fa.ord = ord;
  fa.lists = ma.keys;
  fa.s2 = ma.w2;
  fa.k = k;
  fa.out_count = out_count;
  fa.out_rows = out_rows;
  fa.out_dist = out_dist;
  fa.out_s2 = out_binary;
  fa.out_s3 = out_cosine;
  fa.src = ma.src;
  fa.out_src = out_src;
  return large_order_launch(s, nq, fa);
}

int vrq_merge_shards2_large(int32_t nshards, int32_t nq, int32_t K, const int32_t* counts, const int64_t* rows,
                            const int32_t* dist, const double* score, int32_t k, int32_t* out_count,
                            int64_t* out_rows, int32_t* out_dist, double* out_score, int32_t* out_src,
                            void* workspace, size_t workspace_bytes, void* stream) {
  VRQ_CHECK_ARG(nshards >= 1 && nq >= 0 && K >= 0 && k >= 0);
  VRQ_CHECK_ARG(out_count && out_rows && out_dist && out_score);
  MergePlan p;
  bool run;
  int rc =
      merge_large_checked(nshards, nq, K, k, counts, rows, dist, score, score, workspace, workspace_bytes, &p, &run);
  if (rc != VRQ_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (nq == 0) return VRQ_OK;
  if (!run) return fill_empty_merge(nq, k, out_count, out_rows, out_dist, out_score, nullptr, out_src, s);
  uint8_t* ws = (uint8_t*)workspace;
  MergeSelectArgs ma{nshards, K, nq, counts, rows, dist, score, nullptr, (uint64_t*)(ws + p.off_keys),
                     (int32_t*)(ws + p.off_src), (double*)(ws + p.off_w2), (double*)(ws + p.off_w3),
                     (int32_t*)(ws + p.off_kp)};
  rc = merge_select_launch(s, ma);
  if (rc != VRQ_OK) return rc;
  LargeOrderArgs fa{};
  fa.sc = ma.w2;
  fa.kp = ma.kp;
  fa.K = K;
  fa.limit = K;
  fa.lists = ma.keys;
  fa.s2 = ma.w2;
  fa.k = k;
  fa.out_count = out_count;
  fa.out_rows = out_rows;
  fa.out_dist = out_dist;
  fa.out_s2 = out_score;
  fa.src = ma.src;
  fa.out_src = out_src;
  return large_order_launch(s, nq, fa);
}

}  // extern "C"
