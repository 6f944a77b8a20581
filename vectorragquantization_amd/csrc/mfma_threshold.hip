// mfma_threshold.hip -- the stages around the matrix passes of every matrix-core Phase-I scan (K1m, K1s, K1r
// at 128 code bytes, K1rd at the other code sizes), once: thresholds from the dense sample
// (sample_select_kernel), the proof of the sampled threshold (sample_check_kernel) and the merge of the
// candidate lists into the exact top-K (suffix_topk_kernel), plus the host side both planners and both
// launchers share.  No MFMA here.
//
// The code size CB (bytes) is a compile-time parameter, instantiated for 32, 48, 64, 96, 128, 192 and 256
// and chosen by one switch (for_cb): each instance keeps its query in registers, an unrolled row_dist and
// LDS arrays of its own dim.  Every constant derives from DIM = 8 CB: the dense pass's u16 lane minima
// carry v + DIM (v = dist - pc(q)) in 2 DIM + 1 bins, list keys carry (dist - tau + DIM + 1) << 40 | row.
#include <type_traits>

#include "vrq_internal.h"
#include "vrq_scan.h"

namespace vrq {

template <int CB>
struct ThrCode {
  static constexpr int DIM = 8 * CB;       // code bits
  static constexpr int QW = CB / 4;        // query dwords
  static constexpr int NB = 2 * DIM + 1;   // sample bins: v + DIM, v = dist - pc(q) in [-DIM, DIM]
  static constexpr int KEY_BIAS = DIM + 1; // key field = dist - tau + KEY_BIAS
  static constexpr int HB = 2 * DIM + 2;   // v-field histogram bins
};

// Thresholds from the dense sample (S lane minima per query, each the exact distance of a distinct row):
//   tau_p(q) = d_(K) + 1, accept dist <= the K-th smallest sample distance: the sample rows alone
//              put >= K corpus rows under it, so the candidates always hold the exact top-K
//              (the guaranteed threshold of the re-run);
//   tau_s(q) = d_(j) + 1 for the plan's j < K: with iid rows the corpus holds ~j*n/S rows under
//              it, >= K with probability 1 - 1e-6 (plan); sample_check_kernel proves it per query.
// One workgroup per query: histogram of the S u16 values v + DIM.
template <int CB>
__global__ __launch_bounds__(256) void sample_select_kernel(const uint16_t* __restrict__ dv, int64_t S,
                                                            const uint8_t* __restrict__ queries, int K, int j,
                                                            int32_t* __restrict__ tau_s, int32_t* __restrict__ tau_p,
                                                            int32_t* __restrict__ rerun, int32_t* __restrict__ qbflag,
                                                            int nqb) {
  constexpr int DIM = ThrCode<CB>::DIM, NB = ThrCode<CB>::NB;
  __shared__ uint32_t hist[NB + 3];
  __shared__ int pcq;
  const int qi = blockIdx.x, tid = threadIdx.x;
  if (qi == 0 && qbflag)
    for (int i = tid; i < nqb; i += 256) qbflag[i] = 0;
  for (int i = tid; i < NB; i += 256) hist[i] = 0;
  if (tid == 0) pcq = 0;
  __syncthreads();
  if (tid < ThrCode<CB>::QW)
    atomicAdd(&pcq, __popc(reinterpret_cast<const uint32_t*>(queries + (int64_t)qi * CB)[tid]));
  const uint16_t* d = dv + (int64_t)qi * S;
  const int64_t S8 = S & ~int64_t(7);
  // 16-B loads of 8 values, 8 loads in flight per thread (one workgroup per query: with few queries
  // the pass is latency-bound on a handful of CUs)
  constexpr int U = 8;
  auto add8 = [&](const uint4& w) {
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = x[k] & 0xffff, hi = x[k] >> 16;
      if (lo < (uint32_t)NB) atomicAdd(&hist[lo], 1u);
      if (hi < (uint32_t)NB) atomicAdd(&hist[hi], 1u);
    }
  };
  int64_t i = (int64_t)tid * 8;
  for (; i + (U - 1) * 256 * 8 < S8; i += U * 256 * 8) {
    uint4 w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = *reinterpret_cast<const uint4*>(d + i + u * 256 * 8);
#pragma unroll
    for (int u = 0; u < U; ++u) add8(w[u]);
  }
  for (; i < S8; i += 256 * 8) add8(*reinterpret_cast<const uint4*>(d + i));
  for (int64_t i = S8 + tid; i < S; i += 256)
    if (d[i] < NB) atomicAdd(&hist[d[i]], 1u);
  __syncthreads();
  if (tid < 64) {  // one wave: prefix sums over NB bins, BPL per lane
    constexpr int BPL = (NB + 63) / 64;
    int loc = 0;
    for (int i = 0; i < BPL; ++i) {
      const int b = tid * BPL + i;
      if (b < NB) loc += (int)hist[b];
    }
    int inc = loc;
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(inc, o, 64);
      if (tid >= o) inc += y;
    }
    // k-th smallest: bin b holds it iff cum < k <= cum + hist[b]
    int cum = inc - loc, rk = NB, rj = NB;
    for (int i = 0; i < BPL; ++i) {
      const int b = tid * BPL + i;
      if (b < NB) {
        const int hh = (int)hist[b];
        if (cum < K && cum + hh >= K) rk = b;
        if (cum < j && cum + hh >= j) rj = b;
        cum += hh;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      rk = min(rk, __shfl_xor(rk, o, 64));
      rj = min(rj, __shfl_xor(rj, o, 64));
    }
    if (tid == 0) {
      // fewer than K valid sample values (not for a planned sample): accept every row
      const int dk = rk < NB ? rk - DIM + pcq : DIM;
      const int dj = rj < NB ? rj - DIM + pcq : DIM;
      tau_p[qi] = dk + 1;
      tau_s[qi] = (j < K ? dj : dk) + 1;
      rerun[qi] = 0;  // (the suffix reads tau_p for re-run queries; until a recheck, none)
    }
  }
}

// Proof of the sampled threshold per query: C = candidates with dist < tau_s over the whole corpus
// (the list lengths; an overflowed list counts > capc, and its exact rescan needs no threshold).
// C >= K means the K-th smallest key of the corpus has dist < tau_s, so the candidates hold the
// exact top-K.  Otherwise the query is flagged for the re-run with tau_p.  One wave per query.
__global__ __launch_bounds__(256) void sample_check_kernel(const int32_t* __restrict__ ccnt, int nchunks, int K,
                                                           int nq, int32_t* __restrict__ rerun,
                                                           int32_t* __restrict__ qbflag, int qpb) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), l = lane_id();
  if (q >= nq) return;
  int64_t c = 0;
  for (int i = l; i < nchunks; i += 64) c += ccnt[(int64_t)q * nchunks + i];
  c = wave_sum_i64(c);
  const bool fail = c < K;
  if (l == 0) {
    rerun[q] = fail ? 1 : 0;
    if (fail) atomicOr(&qbflag[q / qpb], 1);
  }
}

// Suffix candidates -> one sorted list of K keys dist << 40 | row per query (KEY_NONE padded).
// The matrix pass left, per (query, chunk), a list of keys (v + DIM + 1) << 40 | row (v = dist - tau(q))
// and its length.  Exact in every case:
//   all lists complete, total <= SUF_CAP  -> sort them all;
//   all lists complete, total  > SUF_CAP  -> histogram of the v-field, threshold T = K-th smallest v, sort
//                                            the keys with v <= T (if they fit);
//   some list overflowed (or neither fits) -> exact rescan of the corpus (distance histogram of DIM + 1
//                                            bins, dist == T ties in row order).
constexpr int SUF_THREADS = 256;
constexpr int SUF_CAP = 4096;
// the most chunks a plan makes (256 CUs x MWAVES x two workgroups per CU): the parallel list gather keeps
// its chunk offsets in the histogram's space, which therefore holds at least this many + 1 at every dim
constexpr int SUF_MAX_CHUNKS = 2048;
// the in-LDS filter below runs with m > SUF_THREADS >= K keys, so its threshold bin always exists
static_assert(kMfmaMaxK <= SUF_THREADS, "the in-LDS filter needs K <= SUF_THREADS");

template <int CB>
struct SufShared {
  static constexpr int HB = ThrCode<CB>::HB;
  static constexpr int HW = (HB > SUF_MAX_CHUNKS + 1 ? HB : SUF_MAX_CHUNKS + 1) + 2;
  uint32_t hist[HW];
  uint64_t buf[SUF_CAP];
  uint32_t qw[ThrCode<CB>::QW];
  int32_t misc[8];
  int32_t scan[SUF_THREADS / WAVE];
};

template <int CB>
__device__ __forceinline__ int row_dist(const uint8_t* __restrict__ codes, int64_t r, const uint32_t (&qw)[CB / 4]) {
  const uint4* p = reinterpret_cast<const uint4*>(codes + r * CB);
  int d = 0;
#pragma unroll
  for (int c = 0; c < CB / 16; ++c) {
    const uint4 v = p[c];
    d += __popc(v.x ^ qw[4 * c]) + __popc(v.y ^ qw[4 * c + 1]) + __popc(v.z ^ qw[4 * c + 2]) +
         __popc(v.w ^ qw[4 * c + 3]);
  }
  return d;
}

// block-wide exclusive scan (SUF_THREADS threads), total in *tot
__device__ inline int suf_excl_scan(int v, int* tot, int32_t* scratch) {
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
  for (int i = 0; i < SUF_THREADS / WAVE; ++i) {
    const int s = scratch[i];
    if (i < w) base += s;
    all += s;
  }
  __syncthreads();
  *tot = all;
  return base + x - v;
}

// Exact top-K of the query over rows [0, n) by brute force (one workgroup): distance histogram ->
// threshold T, then the dist < T rows (any order, sorted by the caller) and the first R rows with
// dist == T in row order.  Leaves m keys (real dist) in sh.buf; returns m.
template <int CB>
__device__ int suffix_rescan(const uint8_t* __restrict__ codes, int64_t n, int K, SufShared<CB>& sh) {
  constexpr int DIM = ThrCode<CB>::DIM, QW = ThrCode<CB>::QW;
  const int tid = threadIdx.x;
  for (int i = tid; i < DIM + 1; i += SUF_THREADS) sh.hist[i] = 0;
  __syncthreads();
  uint32_t qw[QW];
#pragma unroll
  for (int i = 0; i < QW; ++i) qw[i] = sh.qw[i];
  for (int64_t r = tid; r < n; r += SUF_THREADS) atomicAdd(&sh.hist[row_dist<CB>(codes, r, qw)], 1u);
  __syncthreads();
  if (tid == 0) {
    int cum = 0, T = DIM + 1, clt = 0;
    for (int d = 0; d < DIM + 1; ++d) {
      if (cum + (int)sh.hist[d] >= K) {
        T = d;
        clt = cum;
        break;
      }
      cum += (int)sh.hist[d];
    }
    if (T == DIM + 1) clt = cum;
    sh.misc[0] = T;
    sh.misc[1] = clt;
    sh.misc[2] = 0;  // dist < T appended
    sh.misc[3] = 0;  // dist == T taken
  }
  __syncthreads();
  const int T = sh.misc[0], clt = sh.misc[1];
  const int R = K - clt;
  for (int64_t base = 0; base < n; base += SUF_THREADS) {
    const int64_t r = base + tid;
    const int d = r < n ? row_dist<CB>(codes, r, qw) : 0x7fffffff;
    if (d < T) {
      const int pos = atomicAdd(&sh.misc[2], 1);
      sh.buf[pos] = ((uint64_t)(uint32_t)d << KEY_ROW_BITS) | (uint64_t)r;
    }
    const int eq = (d == T) ? 1 : 0;
    if (__syncthreads_or(eq)) {
      int tot;
      const int pre = suf_excl_scan(eq, &tot, sh.scan);  // rank among this block's eq rows, row order
      const int rank = sh.misc[3] + pre;
      if (eq && rank < R) sh.buf[clt + rank] = ((uint64_t)(uint32_t)d << KEY_ROW_BITS) | (uint64_t)r;
      __syncthreads();
      if (tid == 0) sh.misc[3] += tot;
      __syncthreads();
    }
  }
  __syncthreads();
  const int taken = sh.misc[3] < R ? sh.misc[3] : R;
  return clt + (taken > 0 ? taken : 0);
}

template <int CB>
__global__ __launch_bounds__(SUF_THREADS) void suffix_topk_kernel(
    const uint8_t* __restrict__ codes, int64_t n, const uint8_t* __restrict__ queries,
    const uint64_t* __restrict__ cand, const int32_t* __restrict__ ccnt, int nchunks, int capc, int K,
    const int32_t* __restrict__ tau_main, const int32_t* __restrict__ tau_p, const int32_t* __restrict__ rerun,
    uint64_t* __restrict__ out) {
  using Sh = SufShared<CB>;
  constexpr int HB = Sh::HB;
  __shared__ Sh sh;
  const int qi = blockIdx.x, tid = threadIdx.x;
  if (tid < ThrCode<CB>::QW) sh.qw[tid] = reinterpret_cast<const uint32_t*>(queries + (int64_t)qi * CB)[tid];
  if (tid < 8) sh.misc[tid] = 0;
  __syncthreads();
  const int32_t* cq = ccnt + (int64_t)qi * nchunks;
  const uint64_t* Cq = cand + (int64_t)qi * nchunks * capc;
  // the v-field of a key, clamped to the last bin (a corrupt key gives a wrong rank, not an LDS write
  // out of bounds)
  auto vbin = [](uint64_t key) {
    const uint32_t f = (uint32_t)(key >> KEY_ROW_BITS);
    return f < (uint32_t)HB ? f : (uint32_t)(HB - 1);
  };
  // per-chunk counts -> offsets (CPT chunks per thread)
  const int CPT = (nchunks + SUF_THREADS - 1) / SUF_THREADS;
  int mine = 0, over = 0;
  for (int j = 0; j < CPT; ++j) {
    const int c = tid * CPT + j;
    if (c < nchunks) {
      const int v = cq[c];
      over |= v > capc;
      mine += v < capc ? v : capc;
    }
  }
  int total;
  int off = suf_excl_scan(mine, &total, sh.scan);
  const bool overflow = __syncthreads_or(over) != 0;
  // the threshold the query's lists were recorded with: the main pass's, or tau_p after a re-run;
  // dist = v-field + tau(q) - (DIM + 1)
  const int tauq = (rerun && rerun[qi]) ? tau_p[qi] : tau_main[qi];
  const int64_t dfix = (int64_t)tauq - ThrCode<CB>::KEY_BIAS;
  int m = -1;
  bool real_dist = false;
  if (!overflow && total <= SUF_CAP && nchunks < Sh::HW) {  // (the chunk offsets fit the histogram array)
    // every list entry gathered by its own thread (entry e of chunk c = the largest c with coff[c] <= e):
    // independent loads, all in flight at once (a per-thread loop over its chunks' entries waited for
    // each load before its LDS store)
    int32_t* coff = reinterpret_cast<int32_t*>(sh.hist);
    for (int j = 0; j < CPT; ++j) {
      const int c = tid * CPT + j;
      if (c < nchunks) {
        const int v = cq[c];
        coff[c] = off;
        off += v < capc ? v : capc;
      }
    }
    if (tid == 0) coff[nchunks] = total;
    __syncthreads();
    for (int e = tid; e < total; e += SUF_THREADS) {
      int lo = 0, hi = nchunks;  // coff[lo] <= e < coff[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (coff[mid] <= e) lo = mid; else hi = mid;
      }
      sh.buf[e] = Cq[(int64_t)lo * capc + (e - coff[lo])];
    }
    m = total;
  } else if (!overflow) {
    // histogram over the v-field of every candidate, threshold T with >= K keys at v <= T
    for (int i = tid; i < HB; i += SUF_THREADS) sh.hist[i] = 0;
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
      const int v = cq[c];
      for (int i = tid; i < v; i += SUF_THREADS) atomicAdd(&sh.hist[vbin(Cq[(int64_t)c * capc + i])], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      int cum = 0, T = HB - 1;
      for (int d = 0; d < HB; ++d) {
        cum += (int)sh.hist[d];
        if (cum >= K) {
          T = d;
          break;
        }
      }
      sh.misc[5] = T;
      sh.misc[6] = cum;  // keys with v <= T
      sh.misc[7] = 0;
    }
    __syncthreads();
    if (sh.misc[6] <= SUF_CAP) {
      const uint32_t T = (uint32_t)sh.misc[5];
      for (int c = 0; c < nchunks; ++c) {
        const int v = cq[c];
        for (int i = tid; i < v; i += SUF_THREADS) {
          const uint64_t key = Cq[(int64_t)c * capc + i];
          if (vbin(key) <= T) sh.buf[atomicAdd(&sh.misc[7], 1)] = key;
        }
      }
      __syncthreads();
      m = sh.misc[7];
    }
  }
  __syncthreads();
  if (m < 0) {  // overflowed list, or too many candidates: exact rescan (real distances)
    m = suffix_rescan<CB>(codes, n, K, sh);
    real_dist = true;
  }
  __syncthreads();
  if (!real_dist && m > SUF_THREADS) {
    // only the keys with v <= T (T: the K-th smallest v-field) can be among the first K: histogram, then
    // keep those in place, so the sort below usually runs on ~K keys instead of every candidate
    for (int i = tid; i < HB; i += SUF_THREADS) sh.hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += SUF_THREADS) atomicAdd(&sh.hist[vbin(sh.buf[i])], 1u);
    __syncthreads();
    {  // T = the smallest v with cum(v) >= K (m > SUF_THREADS >= K keys: it exists); one block scan
      constexpr int BPT = (HB + SUF_THREADS - 1) / SUF_THREADS;
      int loc = 0;
      for (int b = 0; b < BPT; ++b) {
        const int d = tid * BPT + b;
        if (d < HB) loc += (int)sh.hist[d];
      }
      int tot;
      int cum = suf_excl_scan(loc, &tot, sh.scan);
      for (int b = 0; b < BPT; ++b) {
        const int d = tid * BPT + b;
        if (d >= HB) break;
        const int h = (int)sh.hist[d];
        if (cum < K && cum + h >= K) sh.misc[5] = d;
        cum += h;
      }
      if (tid == 0) sh.misc[7] = 0;
    }
    __syncthreads();
    const uint32_t T = (uint32_t)sh.misc[5];
    constexpr int KPT = SUF_CAP / SUF_THREADS;  // keys per thread (m <= SUF_CAP)
    uint64_t kk[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) kk[j] = tid + j * SUF_THREADS < m ? sh.buf[tid + j * SUF_THREADS] : KEY_NONE;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (kk[j] != KEY_NONE && vbin(kk[j]) <= T) sh.buf[atomicAdd(&sh.misc[7], 1)] = kk[j];
    __syncthreads();
    m = sh.misc[7];
  }
  if (m <= SUF_THREADS) {
    // one key per thread: its rank among the m distinct keys (broadcast LDS reads), one scatter
    const uint64_t ki = tid < m ? sh.buf[tid] : KEY_NONE;
    if (tid < 4) sh.buf[m + tid] = KEY_NONE;  // padding for the 4-key reads (m <= SUF_THREADS < SUF_CAP - 4)
    __syncthreads();
    int rank = 0;
    if (tid < m) {
      for (int j = 0; j < m; j += 4) {  // four broadcast reads in flight
        const uint64_t a = sh.buf[j], b = sh.buf[j + 1], c = sh.buf[j + 2], d = sh.buf[j + 3];
        rank += (a < ki ? 1 : 0) + (b < ki ? 1 : 0) + (c < ki ? 1 : 0) + (d < ki ? 1 : 0);
      }
    }
    __syncthreads();
    if (tid < m) sh.buf[rank] = ki;
    __syncthreads();
  } else {
    const int np2 = next_pow2(m);
    for (int i = m + tid; i < np2; i += SUF_THREADS) sh.buf[i] = KEY_NONE;
    __syncthreads();
    block_bitonic_sort_u64(sh.buf, np2);
  }
  uint64_t* o = out + (int64_t)qi * K;
  const uint64_t ROWM = (1ull << KEY_ROW_BITS) - 1;
  for (int i = tid; i < K; i += SUF_THREADS) {
    uint64_t key = KEY_NONE;
    if (i < m) {
      key = sh.buf[i];
      if (!real_dist) key = ((uint64_t)((int64_t)(key >> KEY_ROW_BITS) + dfix) << KEY_ROW_BITS) | (key & ROWM);
    }
    o[i] = key;
  }
}

// ---- host side ----

// f(integral_constant<int, cb>) for a supported code size
template <class F>
static int for_cb(int cb, F&& f) {
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

// P(Poisson(lam) >= j) <= 1e-6: the sampled order j that an iid corpus proves with that probability
int mfma_sample_order(double lam, int K) {
  double term = __builtin_exp(-lam), cdf = 0.0;
  for (int j = 1; j < K; ++j) {
    cdf += term;  // P(X <= j-1)
    if (1.0 - cdf <= 1e-6) return j;
    term *= lam / j;
  }
  return K;
}

void mfma_plan_lists(MfmaPlan* p, int64_t n, int nq, int K) {
  // per-(query, chunk) list capacity: 4x the hits expected under tau_p (K * chunk_rows / sample, iid rows)
  const int64_t expect = (K * p->chunk_rows + p->sample - 1) / p->sample;
  int capc = 64;
  while (capc < 4 * expect && capc < 4096) capc <<= 1;
  p->capc = capc;
  p->j = mfma_sample_order((double)K * (double)p->sample / (double)n, K);
  // workspace: dv [nq][dvcols] u16 | suffix list [nq][K] | cand [nq][nchunks][capc] |
  //            list lengths [nq][nchunks] | tau_s, tau_p, rerun [nq] | qbflag [nqb]
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  p->off_suffix = al((size_t)nq * p->dvcols * sizeof(uint16_t));
  p->off_cand = p->off_suffix + al((size_t)nq * K * sizeof(uint64_t));
  p->off_cnt = p->off_cand + al((size_t)nq * p->nchunks * p->capc * sizeof(uint64_t));
  p->off_tau = p->off_cnt + al((size_t)nq * p->nchunks * sizeof(int32_t));
  p->bytes = p->off_tau + 3 * al((size_t)nq * sizeof(int32_t)) + (size_t)p->nqb * sizeof(int32_t);
}

int mfma_sample_select_launch(const MfmaPlan& p, const MfmaWorkspace& w, const uint8_t* q, int cb, int nq, int K,
                              hipStream_t s) {
  return for_cb(cb, [&](auto CBC) -> int {
    hipLaunchKernelGGL(sample_select_kernel<decltype(CBC)::value>, dim3(nq), dim3(256), 0, s, (const uint16_t*)w.dv,
                       p.dvcols, q, K, p.j, w.tau_s, w.tau_p, w.rerun, w.qbflag, p.nqb);
    VRQ_LAUNCH_CHECK();
    return VRQ_OK;
  });
}

int mfma_sample_check_launch(const MfmaPlan& p, const MfmaWorkspace& w, int nq, int K, hipStream_t s) {
  hipLaunchKernelGGL(sample_check_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, (const int32_t*)w.ccnt, p.nchunks, K, nq,
                     w.rerun, w.qbflag, p.qpb);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

int mfma_suffix_launch(const MfmaPlan& p, const MfmaWorkspace& w, const uint8_t* codes, int64_t n, int cb,
                       const uint8_t* q, int nq, int K, hipStream_t s) {
  const bool sampled = p.j < K;  // otherwise the matrix pass ran with tau_p and nothing re-ran
  return for_cb(cb, [&](auto CBC) -> int {
    hipLaunchKernelGGL(suffix_topk_kernel<decltype(CBC)::value>, dim3(nq), dim3(SUF_THREADS), 0, s, codes, n, q,
                       (const uint64_t*)w.cand, (const int32_t*)w.ccnt, p.nchunks, p.capc, K,
                       (const int32_t*)(sampled ? w.tau_s : w.tau_p), (const int32_t*)w.tau_p,
                       (const int32_t*)(sampled ? w.rerun : nullptr), w.suffix);
    VRQ_LAUNCH_CHECK();
    return VRQ_OK;
  });
}

}  // namespace vrq
