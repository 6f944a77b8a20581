// exhaustive_dim.hip -- K5d: the exact exhaustive score + top-k scan at every supported embedding dim
// (256, 384, 512, 768, 1024, 1536, 2048), behind vrq_gemm_topk_dim / vrq_flat_ip_topk_dim.
//
// Scores (exact_scores.h; phase2_dot_dim / phase3_cos_dim of select_rescore.hip), one per (query, row):
//   VRQ_GEMM_BINARY       sum of +-q_i over the code bits (packbits MSB first), f64
//   VRQ_GEMM_INT8_COSINE  (double)(float)(sum q_i * x_i in f64) / norm, -inf where norm == 0
//   VRQ_GEMM_FLOAT_IP     (double)(float)(sum q_i * x_i in f64)
// every product exact in f64 (24-bit x 24-bit significands at most, so the fma below rounds once, the
// sum), f64 sums, one rounding to f32, f64 division.  Result per query: the min(k, n) rows with the
// largest score ordered (score desc, row asc); +0.0 and -0.0 tie (desc_key_f64), -inf ranks last.
// No approximation, no threshold pass, no fallback: every score is computed exactly once.
//
// Scan kernel (k5d_scan_kernel): a one-wave workgroup owns one row chunk and one block of QB queries, one
// row per lane, 64-row tiles.
//  * Rows go HBM -> VGPRs -> LDS in slabs of SB <= 128 bytes per row (C = SB / 16 pieces): consecutive
//    lanes load consecutive 16-byte pieces of a row, so a wave instruction covers 64 / C whole row
//    slabs; the next slab's loads are in flight while the current one is scored (two LDS buffers, one
//    workgroup barrier per slab, which for a one-wave workgroup is a wait, not an s_barrier).
//  * Lane l reads piece c of its row at 16-byte slot l * C + (c + rot(l)) % C; the loader applies the
//    inverse rotation to its source address and writes LDS linearly.  rot per C (k5d_rot): the four
//    16-lane groups of a ds_read_b128 then fall on 16 distinct slots mod 16 for every piece index.
//  * The QB queries are pre-widened to f64 in the workspace as [query block][dim][QB]; the scan reads
//    them at wave-uniform addresses (scalar loads, SGPR operands of the f64 FMAs), so a query value
//    costs no VALU or LDS instruction.  (The LDS broadcast form costs one ds_read per two FMAs.)
//  * Per element one conversion of the row value, then QB FMAs.  With few queries the per-query sum
//    is split over 4 / QB accumulators so the dependent-FMA latency is covered.
//  * Top-k per (query, chunk): keys desc_key_f64(score) (u64) + chunk row (u32) are ballot-compacted
//    into a CAP-entry LDS list under the running k-th key; a full list is cut to its exact top k by a
//    bitonic sort on (key, row).  Rows arrive in ascending order, so a row whose key equals the k-th
//    key never displaces it: the test is key < tau.
// Merge kernel (k5d_merge_kernel): a workgroup folds chunk lists through an LDS bitonic sort of up to 2048
// entries; long merges fold 32 groups of lists per query in parallel first, then the 32 group results.  Every loop has a fixed trip count; no workgroup waits
// on another.
#include "vrq_internal.h"

namespace vrq {
namespace k5d {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr int TILE_ROWS = 64;
constexpr int MAX_CHUNKS = 2048;   // bounds the lists: nq * chunks * k entries, whatever n is
constexpr int TARGET_WGS = 2048;   // 256 CUs x 8 one-wave workgroups
constexpr int MERGE_NT = 256;
constexpr int MERGE_CAP = 2048;    // >= 2 * KMAX
constexpr int MERGE_BUDGET = 65536;  // list entries per query: chunks <= MERGE_BUDGET / k (at least 16)
constexpr int MERGE_GROUPS = 32;
constexpr int KMAX5 = 1024;
constexpr uint64_t KEY_PAD = ~0ull;
constexpr uint32_t ROW_PAD = ~0u;

// rotation of lane / row l's pieces in a slab of C 16-byte pieces
__host__ __device__ constexpr int k5d_rot(int C, int l) {
  return C == 2 ? (l >> 3) % 2 : C == 4 ? (l >> 2) % 4 : C == 6 ? (l >> 4) % 6 : C == 8 ? (l >> 1) % 8 : 0;  // C == 3: 0
}

struct Plan {
  int sb;             // slab bytes per row
  int qb;             // queries per workgroup
  int nqb;            // query blocks
  int cap;            // list capacity per (query, chunk) in LDS
  int nchunks;
  int64_t chunk_rows;
  int ngroups, gsize;  // merge: groups of gsize chunk lists are folded first when the lists are long
  // qd f64 [nqb][dim][qb] at 0; keys u64 / rows u32 [nq][nchunks][k]; group results [nq][ngroups][k]
  size_t off_key, off_row, off_gkey, off_grow, bytes;
};

__host__ inline int row_bytes(int mode, int dim) {
  return mode == VRQ_GEMM_BINARY ? dim / 8 : mode == VRQ_GEMM_INT8_COSINE ? dim : 4 * dim;
}

__host__ inline int plan(int mode, int64_t n, int dim, int nq, int k, Plan* p) {
  if (mode != VRQ_GEMM_BINARY && mode != VRQ_GEMM_INT8_COSINE && mode != VRQ_GEMM_FLOAT_IP) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  if (n < 1 || nq < 1 || k < 1) return VRQ_EINVAL;
  if (k > KMAX5 || n >= (1ll << 32)) return VRQ_EUNSUPPORTED;
  const int rb = row_bytes(mode, dim);
  p->sb = rb <= 128 ? rb : (rb % 128 == 0 ? 128 : 96);  // 192-byte code rows: two slabs of 96
  p->cap = next_pow2(k + TILE_ROWS) < 128 ? 128 : next_pow2(k + TILE_ROWS);  // one tile fits after a cut
  int qb = p->cap <= 256 ? 8 : p->cap <= 512 ? 4 : 1;  // lists: qb * cap * 12 B <= 24 KiB of LDS
  if (nq == 1) qb = 1;
  if (nq <= 4 && qb > 4) qb = 4;
  p->qb = qb;
  p->nqb = (nq + qb - 1) / qb;
  const int64_t ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
  int64_t want = (TARGET_WGS + p->nqb - 1) / p->nqb;
  int64_t maxc = MERGE_BUDGET / k;  // bounds the merge's work per query as well as the lists
  maxc = maxc < 16 ? 16 : maxc > MAX_CHUNKS ? MAX_CHUNKS : maxc;
  want = want < 1 ? 1 : want > maxc ? maxc : want;
  want = want > ntiles ? ntiles : want;
  const int64_t tpc = (ntiles + want - 1) / want;
  p->chunk_rows = tpc * TILE_ROWS;
  p->nchunks = (int)((ntiles + tpc - 1) / tpc);
  const size_t qd = (size_t)p->nqb * qb * dim * sizeof(double);
  const size_t ent = (size_t)nq * p->nchunks * k;
  // more list entries than one merge round takes: fold groups of lists in parallel first
  const int groups = (int64_t)p->nchunks * k > MERGE_CAP - k ? (p->nchunks < MERGE_GROUPS ? p->nchunks : MERGE_GROUPS) : 1;
  p->gsize = (p->nchunks + groups - 1) / groups;
  p->ngroups = (p->nchunks + p->gsize - 1) / p->gsize;
  const size_t gent = p->ngroups > 1 ? (size_t)nq * p->ngroups * k : 0;
  p->off_key = (qd + 255) & ~(size_t)255;
  p->off_row = p->off_key + ((ent * 8 + 255) & ~(size_t)255);
  p->off_gkey = p->off_row + ((ent * 4 + 255) & ~(size_t)255);
  p->off_grow = p->off_gkey + ((gent * 8 + 255) & ~(size_t)255);
  p->bytes = p->off_grow + ((gent * 4 + 255) & ~(size_t)255);
  return VRQ_OK;
}

// queries f32 [nq][dim] -> f64 [nqb][dim][QB]; absent queries of the last block are zero
__global__ void k5d_prep_kernel(const float* __restrict__ qf, int nq, int dim, int qb, int64_t total,
                                double* __restrict__ qd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % qb);
  const int64_t r = i / qb;
  const int e = (int)(r % dim);
  const int64_t q = (r / dim) * qb + j;
  qd[i] = q < nq ? (double)qf[q * dim + e] : 0.0;
}

// (key, row) ascending bitonic sort of n_pow2 LDS entries by all threads of the block
__device__ inline void sort_pairs(uint64_t* key, uint32_t* row, int n_pow2) {
  for (int size = 2; size <= n_pow2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < (n_pow2 >> 1); i += blockDim.x) {
        const int lo = ((i / stride) * stride * 2) + (i % stride);
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t x = key[lo], y = key[hi];
        const uint32_t rx = row[lo], ry = row[hi];
        const bool gt = x > y || (x == y && rx > ry);
        if (gt == up) {
          key[lo] = y;
          key[hi] = x;
          row[lo] = ry;
          row[hi] = rx;
        }
      }
    }
  }
  __syncthreads();
}

// The query stream of one slab (or piece): NEL f64 values at a wave-uniform address, handed to use(s, q)
// in order, 16 at a time.  The two s_load_dwordx16 of a batch and their wait are ONE asm statement, as
// K1's load_q: the 32 SGPRs are valid where it ends, so the compiler can neither hoist a slab's loads
// together (that spilled hundreds of SGPRs) nor touch a destination before its data has landed.  pin() is called before each batch.
typedef uint32_t v16u __attribute__((ext_vector_type(16)));
__device__ __forceinline__ double sgpr_f64(const v16u& v, int i) {
  return __builtin_bit_cast(double, ((uint64_t)v[2 * i + 1] << 32) | v[2 * i]);
}
template <int NEL, class F, class P>
__device__ __forceinline__ void stream_q(const double* __restrict__ base, F&& use, P&& pin) {
  constexpr int NB = 16;
  static_assert(NEL % NB == 0, "stream length");
#pragma unroll
  for (int b = 0; b < NEL / NB; ++b) {
    v16u lo, hi;
    const double* p = base + b * NB;
    pin();  // volatile, reads the accumulators: the previous batch's FMAs stay above this batch's loads
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo), "=&s"(hi)
                 : "s"(p));
#pragma unroll
    for (int i = 0; i < 8; ++i) use(b * NB + i, sgpr_f64(lo, i));
#pragma unroll
    for (int i = 0; i < 8; ++i) use(b * NB + 8 + i, sgpr_f64(hi, i));
  }
}

template <int MODE, int QB, int C>
__global__ __launch_bounds__(64) void k5d_scan_kernel(const uint8_t* __restrict__ rows, const double* __restrict__ norms,
                                                      int64_t n, int dim, int rb, const double* __restrict__ qd, int nq,
                                                      int k, int cap, int64_t chunk_rows, int nchunks, int nqb,
                                                      uint64_t* __restrict__ out_key, uint32_t* __restrict__ out_row) {
  constexpr int SB = C * 16;
  constexpr int A = QB >= 4 ? 1 : 4 / QB;  // accumulators per query
  // elements per 16-byte piece
  constexpr int EPP = MODE == VRQ_GEMM_BINARY ? 128 : MODE == VRQ_GEMM_INT8_COSINE ? 16 : 4;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  v4u* slab = reinterpret_cast<v4u*>(smem);                                   // [2][64 * C]
  uint64_t* lkey = reinterpret_cast<uint64_t*>(smem + 2 * TILE_ROWS * SB);    // [QB][cap]
  uint32_t* lrow = reinterpret_cast<uint32_t*>(lkey + (size_t)QB * cap);      // [QB][cap]

  const int chunk = blockIdx.x / nqb;
  const int qblk = blockIdx.x - chunk * nqb;
  const int64_t row0 = (int64_t)chunk * chunk_rows;
  const int64_t row1 = row0 + chunk_rows < n ? row0 + chunk_rows : n;
  const int nrows = (int)(row1 - row0);
  const int ntiles = (nrows + TILE_ROWS - 1) / TILE_ROWS;
  const int ns = rb / SB;  // slabs per row
  const int l = threadIdx.x;
  const int q0 = qblk * QB;
  const int nqa = nq - q0 < QB ? nq - q0 : QB;
  const double* __restrict__ qbase = qd + (int64_t)qblk * dim * QB;

  int cnt[QB];
  uint64_t tau[QB];
#pragma unroll
  for (int j = 0; j < QB; ++j) {
    cnt[j] = 0;
    tau[j] = KEY_PAD;
  }

  // loader: 16-byte unit p = gi * 64 + l of a slab is (row p / C, LDS piece slot p % C)
  int ld_r[C], ld_c[C];
#pragma unroll
  for (int gi = 0; gi < C; ++gi) {
    const int p = gi * 64 + l;
    const int r = p / C, cs = p % C;
    ld_r[gi] = r;
    ld_c[gi] = (cs + C - k5d_rot(C, r)) % C;  // the piece that row r reads at slot cs
  }
  const int rot = k5d_rot(C, l);
  v4u st[C];
  auto gload = [&](int t, int sl) __attribute__((always_inline)) {
#pragma unroll
    for (int gi = 0; gi < C; ++gi) {
      int64_t row = row0 + (int64_t)t * TILE_ROWS + ld_r[gi];
      row = row < row1 ? row : row1 - 1;  // ragged last tile: clamp (those lanes never accept)
      st[gi] = *reinterpret_cast<const v4u*>(rows + row * rb + sl * SB + ld_c[gi] * 16);
    }
  };
  auto lwrite = [&](int b) __attribute__((always_inline)) {
#pragma unroll
    for (int gi = 0; gi < C; ++gi) slab[b * TILE_ROWS * C + gi * 64 + l] = st[gi];
  };

  auto accept = [&](int j, uint64_t key, uint32_t lrw, bool valid) __attribute__((always_inline)) {
    bool acc = valid && key < tau[j];
    uint64_t mask = __ballot(acc);
    if (mask) {
      int nnew = __popcll(mask);
      uint64_t* kj = lkey + (size_t)j * cap;
      uint32_t* rj = lrow + (size_t)j * cap;
      if (cnt[j] + nnew > cap) {
        for (int i = cnt[j] + l; i < cap; i += WAVE) {
          kj[i] = KEY_PAD;
          rj[i] = ROW_PAD;
        }
        sort_pairs(kj, rj, cap);
        cnt[j] = cnt[j] < k ? cnt[j] : k;
        if (cnt[j] >= k) tau[j] = kj[k - 1];
        acc = valid && key < tau[j];
        mask = __ballot(acc);
        nnew = __popcll(mask);
      }
      if (acc) {
        const int pos = cnt[j] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        kj[pos] = key;
        rj[pos] = lrw;
      }
      cnt[j] += nnew;  // (other lanes read the list only in sort_pairs, behind its barrier)
    }
  };

  double accv[QB][A];
#pragma unroll
  for (int j = 0; j < QB; ++j)
#pragma unroll
    for (int a = 0; a < A; ++a) accv[j][a] = 0.0;

  auto pin = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < QB; ++j)
#pragma unroll
      for (int a = 0; a < A; ++a) asm volatile("" : "+v"(accv[j][a]));
  };

  const int total = ntiles * ns;
  gload(0, 0);
  lwrite(0);
  __syncthreads();
  int t = 0, sl = 0;
  for (int i = 0; i < total; ++i) {
    int tn = t, sn = sl + 1;
    if (sn == ns) {
      sn = 0;
      tn = t + 1;
    }
    if (i + 1 < total) gload(tn, sn);
    const v4u* buf = slab + (i & 1) * TILE_ROWS * C;
    if constexpr (MODE == VRQ_GEMM_BINARY) {  // 128 * QB terms per piece: the piece loop stays rolled
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        const v4u v = buf[l * C + (c + rot) % C];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        stream_q<128 * QB>(qbase + (int64_t)((sl * C + c) * 128) * QB, [&](int s, double q) __attribute__((always_inline)) {
          const int e = s / QB, j = s % QB;  // dim order: byte (e / 8) % 4 of dword e / 32, bit 7 - e % 8
          const bool bit = (w[e >> 5] >> (8 * ((e >> 3) & 3) + 7 - (e & 7))) & 1u;
          accv[j][e % A] += bit ? q : -q;
        }, pin);
      }
    } else {
      v4u pv[C];
#pragma unroll
      for (int c = 0; c < C; ++c) pv[c] = buf[l * C + (c + rot) % C];
      stream_q<C * EPP * QB>(qbase + (int64_t)(sl * C * EPP) * QB, [&](int s, double q) __attribute__((always_inline)) {
        const int c = s / (EPP * QB), e = (s / QB) % EPP, j = s % QB;
        const v4u v = pv[c];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        double x;
        if constexpr (MODE == VRQ_GEMM_INT8_COSINE)
          x = (double)(int32_t)(int8_t)((w[e >> 2] >> (8 * (e & 3))) & 0xffu);
        else
          x = (double)__uint_as_float(w[e]);
        accv[j][e % A] = __builtin_fma(q, x, accv[j][e % A]);  // the product is exact: one rounding, the sum's
      }, pin);
    }
    if (i + 1 < total) lwrite((i + 1) & 1);
    __syncthreads();
    if (sl == ns - 1) {  // the tile's rows are complete
      const int local = t * TILE_ROWS + l;
      const bool valid = local < nrows;
      double nrm = 1.0;
      if constexpr (MODE == VRQ_GEMM_INT8_COSINE) nrm = norms[valid ? row0 + local : row0];
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        double s = accv[j][0];
        if constexpr (A == 2) s = accv[j][0] + accv[j][1];
        if constexpr (A == 4) s = (accv[j][0] + accv[j][1]) + (accv[j][2] + accv[j][3]);
#pragma unroll
        for (int a = 0; a < A; ++a) accv[j][a] = 0.0;
        if constexpr (MODE == VRQ_GEMM_INT8_COSINE) s = nrm == 0.0 ? -__builtin_inf() : (double)(float)s / nrm;
        if constexpr (MODE == VRQ_GEMM_FLOAT_IP) s = (double)(float)s;
        if (j < nqa) accept(j, desc_key_f64(s), (uint32_t)local, valid);
      }
    }
    t = tn;
    sl = sn;
  }

  // chunk done: the exact top-k of each query's list, (key, row asc), padded
#pragma unroll
  for (int j = 0; j < QB; ++j) {
    if (j >= nqa) break;
    uint64_t* kj = lkey + (size_t)j * cap;
    uint32_t* rj = lrow + (size_t)j * cap;
    for (int i = cnt[j] + l; i < cap; i += WAVE) {
      kj[i] = KEY_PAD;
      rj[i] = ROW_PAD;
    }
    sort_pairs(kj, rj, cap);
    const int m = cnt[j] < k ? cnt[j] : k;
    const int64_t o = ((int64_t)(q0 + j) * nchunks + chunk) * k;
    for (int i = l; i < k; i += WAVE) {
      out_key[o + i] = i < m ? kj[i] : KEY_PAD;
      out_row[o + i] = i < m ? (uint32_t)(row0 + rj[i]) : ROW_PAD;  // n < 2^32
    }
  }
}

__device__ __forceinline__ double key_to_score(uint64_t key) {
  const uint64_t u = ~key;  // ascending image
  const uint64_t b = (u & 0x8000000000000000ull) ? (u & 0x7fffffffffffffffull) : ~u;
  return __longlong_as_double((long long)b);
}

// One workgroup per (query, group): folds the group's gsize lists of k sorted entries into its top k,
// a round of up to MERGE_CAP - k new entries at a time behind the k kept ones (bitonic sort of the
// smallest power of two that holds them).  With gkey set it writes the group's list (first level of
// long merges); otherwise the final result.
__global__ __launch_bounds__(MERGE_NT) void k5d_merge_kernel(const uint64_t* __restrict__ keys,
                                                             const uint32_t* __restrict__ rws, int nlists, int gsize,
                                                             int ngroups, int k, int64_t n, int64_t row_offset,
                                                             uint64_t* __restrict__ gkey, uint32_t* __restrict__ grow,
                                                             int32_t* __restrict__ out_count,
                                                             int64_t* __restrict__ out_rows, double* __restrict__ out_scores) {
  __shared__ uint64_t key[MERGE_CAP];
  __shared__ uint32_t row[MERGE_CAP];
  const int q = blockIdx.x / ngroups, g = blockIdx.x - q * ngroups;
  const int l0 = g * gsize, l1 = l0 + gsize < nlists ? l0 + gsize : nlists;
  const int64_t total = (int64_t)(l1 - l0) * k;
  const uint64_t* kq = keys + ((int64_t)q * nlists + l0) * k;
  const uint32_t* rq = rws + ((int64_t)q * nlists + l0) * k;
  const int step = MERGE_CAP - k;
  for (int i = threadIdx.x; i < k; i += MERGE_NT) {
    key[i] = KEY_PAD;
    row[i] = ROW_PAD;
  }
  for (int64_t base = 0; base < total; base += step) {
    const int nnew = total - base < step ? (int)(total - base) : step;
    const int np2 = next_pow2(k + nnew);  // <= MERGE_CAP
    for (int i = threadIdx.x; i < np2 - k; i += MERGE_NT) {
      key[k + i] = i < nnew ? kq[base + i] : KEY_PAD;
      row[k + i] = i < nnew ? rq[base + i] : ROW_PAD;
    }
    sort_pairs(key, row, np2);  // starts and ends with a barrier
  }
  if (gkey) {
    const int64_t o = ((int64_t)q * ngroups + g) * k;
    for (int i = threadIdx.x; i < k; i += MERGE_NT) {
      gkey[o + i] = key[i];
      grow[o + i] = row[i];
    }
    return;
  }
  const int m = (int64_t)k < n ? k : (int)n;
  for (int i = threadIdx.x; i < k; i += MERGE_NT) {
    out_rows[(int64_t)q * k + i] = i < m ? row_offset + (int64_t)row[i] : -1;
    out_scores[(int64_t)q * k + i] = i < m ? key_to_score(key[i]) : __builtin_nan("");
  }
  if (threadIdx.x == 0) out_count[q] = m;
}

template <int MODE, int QB, int C>
static int launch_c(const Plan& p, const uint8_t* rows, const double* norms, int64_t n, int dim, int rb,
                    const double* qd, int nq, int k, uint64_t* okey, uint32_t* orow, hipStream_t s) {
  const size_t lds = (size_t)2 * TILE_ROWS * C * 16 + (size_t)QB * p.cap * 12;
  hipLaunchKernelGGL((k5d_scan_kernel<MODE, QB, C>), dim3((unsigned)(p.nchunks * p.nqb)), dim3(64), lds, s, rows, norms,
                     n, dim, rb, qd, nq, k, p.cap, p.chunk_rows, p.nchunks, p.nqb, okey, orow);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

template <int MODE, int QB>
static int launch_q(const Plan& p, const uint8_t* rows, const double* norms, int64_t n, int dim, int rb,
                    const double* qd, int nq, int k, uint64_t* okey, uint32_t* orow, hipStream_t s) {
  if constexpr (MODE == VRQ_GEMM_BINARY) {
    switch (p.sb / 16) {
      case 2: return launch_c<MODE, QB, 2>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
      case 3: return launch_c<MODE, QB, 3>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
      case 4: return launch_c<MODE, QB, 4>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
      case 6: return launch_c<MODE, QB, 6>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
      case 8: return launch_c<MODE, QB, 8>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
      default: return VRQ_EUNSUPPORTED;
    }
  } else {
    if (p.sb != 128) return VRQ_EUNSUPPORTED;
    return launch_c<MODE, QB, 8>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
  }
}

template <int MODE>
static int launch_m(const Plan& p, const uint8_t* rows, const double* norms, int64_t n, int dim, int rb,
                    const double* qd, int nq, int k, uint64_t* okey, uint32_t* orow, hipStream_t s) {
  switch (p.qb) {
    case 1: return launch_q<MODE, 1>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
    case 4: return launch_q<MODE, 4>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
    case 8: return launch_q<MODE, 8>(p, rows, norms, n, dim, rb, qd, nq, k, okey, orow, s);
    default: return VRQ_EUNSUPPORTED;
  }
}

static int run(int mode, const void* rows, const double* norms, int64_t n, int dim, int64_t row_offset,
               const float* qf, int nq, int k, int32_t* out_count, int64_t* out_rows, double* out_scores,
               void* workspace, size_t workspace_bytes, hipStream_t s) {
  Plan p;
  const int rc = plan(mode, n, dim, nq, k, &p);
  if (rc != VRQ_OK) return rc;
  if (workspace_bytes < p.bytes) return VRQ_EWORKSPACE;
  uint8_t* ws = (uint8_t*)workspace;
  double* qd = (double*)ws;
  uint64_t* okey = (uint64_t*)(ws + p.off_key);
  uint32_t* orow = (uint32_t*)(ws + p.off_row);
  const int64_t total = (int64_t)p.nqb * p.qb * dim;
  hipLaunchKernelGGL(k5d_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, qf, nq, dim, p.qb, total,
                     qd);
  VRQ_LAUNCH_CHECK();
  const int rb = row_bytes(mode, dim);
  const uint8_t* r8 = (const uint8_t*)rows;
  int rc2;
  if (mode == VRQ_GEMM_BINARY)
    rc2 = launch_m<VRQ_GEMM_BINARY>(p, r8, norms, n, dim, rb, qd, nq, k, okey, orow, s);
  else if (mode == VRQ_GEMM_INT8_COSINE)
    rc2 = launch_m<VRQ_GEMM_INT8_COSINE>(p, r8, norms, n, dim, rb, qd, nq, k, okey, orow, s);
  else
    rc2 = launch_m<VRQ_GEMM_FLOAT_IP>(p, r8, norms, n, dim, rb, qd, nq, k, okey, orow, s);
  if (rc2 != VRQ_OK) return rc2;
  const uint64_t* mk = okey;
  const uint32_t* mr = orow;
  int nlists = p.nchunks;
  if (p.ngroups > 1) {
    uint64_t* gk = (uint64_t*)(ws + p.off_gkey);
    uint32_t* gr = (uint32_t*)(ws + p.off_grow);
    hipLaunchKernelGGL(k5d_merge_kernel, dim3((unsigned)nq * p.ngroups), dim3(MERGE_NT), 0, s, mk, mr, nlists, p.gsize,
                       p.ngroups, k, n, row_offset, gk, gr, (int32_t*)nullptr, (int64_t*)nullptr, (double*)nullptr);
    VRQ_LAUNCH_CHECK();
    mk = gk;
    mr = gr;
    nlists = p.ngroups;
  }
  hipLaunchKernelGGL(k5d_merge_kernel, dim3(nq), dim3(MERGE_NT), 0, s, mk, mr, nlists, nlists, 1, k, n, row_offset,
                     (uint64_t*)nullptr, (uint32_t*)nullptr, out_count, out_rows, out_scores);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// flags of the _dim entry points where K5d runs
static int flags_ok(int flags) {
  return (flags & ~(VRQ_GEMM_SCAN_EXACT | VRQ_GEMM_NO_FALLBACK)) == 0;
}

}  // namespace k5d
}  // namespace vrq

using namespace vrq;

extern "C" {

size_t vrq_gemm_topk_dim_workspace_size(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k) {
  if (dim == 1024) return vrq_gemm_topk_workspace_size(mode, n, dim, nq, k);
  k5d::Plan p;
  if (k5d::plan(mode, n, dim, nq, k, &p) != VRQ_OK) return 0;
  return p.bytes;
}

int vrq_gemm_topk_dim_plan(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  k5d::Plan p;
  const int rc = k5d::plan(mode, n, dim, nq, k, &p);
  if (rc != VRQ_OK) return rc == VRQ_EINVAL ? VRQ_EUNSUPPORTED : rc;
  info[0] = k5d::TILE_ROWS;
  info[1] = p.chunk_rows;
  info[2] = p.nchunks;
  info[3] = p.qb;
  info[4] = p.cap;
  info[5] = (int64_t)p.bytes;
  return VRQ_OK;
}

int vrq_gemm_topk_dim(int32_t mode, const uint8_t* codes, const int8_t* x8, const double* norms, int64_t n,
                      int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t flags,
                      int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (dim == 1024 && !(flags & VRQ_GEMM_SCAN_EXACT))
    return vrq_gemm_topk(mode, codes, x8, norms, n, dim, row_offset, qf, nq, k, flags, out_count, out_rows,
                         out_scores, workspace, workspace_bytes, stream);
  if (mode != VRQ_GEMM_BINARY && mode != VRQ_GEMM_INT8_COSINE) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(qf && out_count && out_rows && out_scores && workspace && n > 0 && nq > 0 && k > 0);
  if (mode == VRQ_GEMM_BINARY) VRQ_CHECK_ARG(codes);
  if (mode == VRQ_GEMM_INT8_COSINE) VRQ_CHECK_ARG(x8 && norms);
  if (!k5d::flags_ok(flags)) return VRQ_EUNSUPPORTED;  // no stages: K5d is one pass
  const void* rows = mode == VRQ_GEMM_BINARY ? (const void*)codes : (const void*)x8;
  return k5d::run(mode, rows, norms, n, dim, row_offset, qf, nq, k, out_count, out_rows, out_scores, workspace,
                  workspace_bytes, (hipStream_t)stream);
}

int vrq_flat_ip_topk_dim(const float* xf, const int8_t* x8, const double* inv_scale, const double* bounds, int64_t n,
                         int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t flags,
                         int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (dim == 1024 && !(flags & VRQ_GEMM_SCAN_EXACT))
    return vrq_flat_ip_topk(xf, x8, inv_scale, bounds, n, dim, row_offset, qf, nq, k, flags, out_count, out_rows,
                            out_scores, workspace, workspace_bytes, stream);
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(xf && qf && out_count && out_rows && out_scores && workspace && n > 0 && nq > 0 && k > 0);
  if (!k5d::flags_ok(flags)) return VRQ_EUNSUPPORTED;
  return k5d::run(VRQ_GEMM_FLOAT_IP, xf, nullptr, n, dim, row_offset, qf, nq, k, out_count, out_rows, out_scores,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
