// gemm_topk_dim.hip -- K5md: exhaustive int8-cosine (Phase-III) top-k of a query batch against the whole
// corpus on the matrix cores (v_mfma_i32_32x32x32_i8) at the embedding dims other than 1024:
// 256, 384, 512, 768, 1536, 2048.  Behind vrq_gemm_topk_dim_mfma; K5 (gemm_topk.hip) stays the d = 1024
// pipeline and K5d (exhaustive_dim.hip) the exact f64 scan.
//
// The method is K5's (the header of gemm_topk.hip has the exactness argument): prep q/S = a + rho with one
// int8 piece a; a dense sample pass keeps the running max of u = f32(<a, x>) * (1 / f32(norm)) per
// (query, sample chunk, lane row); select takes U = the k-th largest maximum and thr = U - 2 Delta; the
// main pass appends every row with u >= thr to a per-(query, chunk) list; finish rescores the lists by the
// exact definition (exact_scores.h at run-time dim: the lane -> dims map and summation order of
// phase3_cos_dim, so the scores are vrq_rescore_int8_cosine_dim's bit for bit), retries an overflowed
// query once at the raised threshold alpha s_k + beta - Delta, and hands what is left to an exact scan.
//
// Delta = ||rho||_2 (1 + eps) + eps ||q/S||_2, eps = 2^-20.  Cauchy-Schwarz does not see d.  The f32 slack at
// d = 2048: A = <a, x> is exact in i32 but |A| reaches 127 * 127 * 2048 > 2^24, so the roundings on the u
// path are v_cvt_f32_i32 (2^-24; exact below 2^24, i.e. up to d = 1024), the norm's f64 -> f32 (2^-24),
// v_rcp_f32 (1 ulp: 2^-23) and the product (2^-24; the main pass tests the sign of one fma instead):
// (1 + 2^-24)^3 (1 + 2^-23) - 1 < 2^-21 relative to |u| <= ||a|| <= ||q/S|| + ||rho||.  The reference score
// s' = s / S carries the f32 rounding of the dot: 2^-24 ||q/S||.  Sum < (2^-21 + 2^-24)(||q/S|| + ||rho||)
// < eps (||q/S|| + ||rho||), which is what Delta adds to ||rho||.
//
// Matrix pass (k5md_pass_kernel<KS, DENSE>, KS = d / 32 k-steps): one workgroup per CU and query block;
// the int8 A fragments of its queries for all of d stay in the accumulator file for the whole chunk;
// 32-row tiles (32 d bytes + 32 f64 norms) stream HBM -> LDS by LDS-DMA in a ring of 2, in 1-KiB pieces
// dealt round-robin to the waves and spread over the MFMA shadow; the threshold tests of tile t-1 run in
// tile t's MFMA shadow and its hits reach a per-wave LDS stage in tile t+1, drained once per chunk.
//   d <= 256     8 waves (two per SIMD) x 2 M-blocks of 32 queries: a B fragment feeds two MFMAs  (512 / WG)
//   d = 384..768 8 waves x 32 queries                                                             (256 / WG)
//   d >= 1536    4 waves (one per SIMD) x 32 queries, the 192 / 256 A registers in the AGPR half  (128 / WG)
// LDS image of a tile: row rr at byte rr * d, its 16-byte chunk c at slot c ^ x(rr), where
//   x(rr) = rr & 15        when d / 16 is a multiple of 16 (K5's rule),
//   x(rr) = (rr >> 1) & 7  at d = 384 (24 chunks per row: the row stride is 8 slots mod 16, so the row's
//                          parity picks the half and the XOR stays inside a group of 8 chunks).
// The DMA applies x to its source address and writes LDS linearly.  A ds_read_b128 of B fragments (lane
// (r, h) reads chunk 2s + h of row r) then finds 16 distinct slots mod 16 in each of its four 16-lane
// groups at every dim (DESIGN section 5 "K5md" enumerates them).
// A ragged last tile is shifted back to end at the chunk's end (rows already seen are masked), so every
// DMA reads a whole in-bounds tile; a chunk shorter than 32 rows clamps its rows.  Every loop has a fixed
// trip count and no workgroup waits on another.
#include <math.h>

#include "mfma_common.h"
#include "vrq_internal.h"

namespace vrq {
namespace g5d {

constexpr int GRT = 32;       // corpus rows per tile
constexpr int STG = 1024;     // staged hit entries per wave (u32: query-in-wave << 26 | chunk row)
constexpr int64_t kMaxChunkRows = (int64_t(1) << 26) - 32;
constexpr int FIN_CAP = 8192, CAP_MULT = 16, kChunkMult = 4;  // K5's planning rules
constexpr int64_t kMinSample = 32768, kMaxSample = 1 << 21;
constexpr int KMAX5 = 1024, FB_BATCH = 1024, MAX_CHUNKS = 2048;
constexpr int BA = 2, NR = 4;  // B fragments read BA k-steps ahead into a ring of NR

__host__ __device__ constexpr int swz(int cpr, int rr) { return cpr % 16 == 0 ? (rr & 15) : ((rr >> 1) & 7); }

template <int KS>
struct Shape {
  static constexpr int D = 32 * KS, CPR = D / 16;
  // waves: two per SIMD while 32 queries' fragments fit beside them.  KS = 32 exists for the gathered calls alone
  // (unfiltered 1024 is K5's): its thresholded 8-wave instance needs 3 registers more than the 128 it has beside
  // the 128 fragment registers once the list entries are live, so it takes the 4-wave shape
  static constexpr int W = KS >= 32 ? 4 : 8;
  static constexpr int MB = KS <= 8 ? 2 : 1;   // M-blocks of 32 queries per wave
  static constexpr int QW = 32 * MB, QB = W * QW, NE = 16 * MB;
  static constexpr int XB = CPR % 16 == 0 ? 4 : 3;  // chunk-index bits the swizzle touches
  static constexpr int NA = 1 << (XB - 1);          // B addresses kept per lane (the rest: immediate offsets)
  static constexpr int TB = GRT * D, PKT = TB + GRT * 8;  // tile bytes, ring slot bytes (+ norms)
  static constexpr int PPW = (KS + W - 1) / W;      // 1-KiB row pieces per wave and tile (+ 1: the norms)
  static constexpr int DS = (KS - 2) / (PPW + 1) > 0 ? (KS - 2) / (PPW + 1) : 1;  // k-steps between pieces
  static constexpr int TPS = (NE + KS - 1) / KS;    // threshold tests per k-step
  static constexpr int EOFF = KS >= 24 ? 4 : 0;
};

__device__ __forceinline__ v16i mfma_i8(const v4i& a, const v4i& b, const v16i& c) {
  return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ void lds_read_f64(double& d, uint32_t a) {
  asm volatile("ds_read_b64 %0, %1" : "=v"(d) : "v"(a) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read128_off(v4i& d, uint32_t a) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(a), "n"(OFF) : "memory");
}
// the row list of a gathered kernel instance (none: the contiguous instances)
__device__ __forceinline__ const uint32_t* gather_rows() { return nullptr; }
__device__ __forceinline__ const uint32_t* gather_rows(const uint32_t* rows) { return rows; }
// a 4-byte load that the compiler does not wait for: d holds the value after the next wait_vm<0> (which names
// it "+v"); the destination is an in/out operand, see lds_read128_inplace
__device__ __forceinline__ void load_u32_async(uint32_t& d, const uint32_t* p) {
  asm volatile("global_load_dword %0, %1, off" : "+v"(d) : "v"(p) : "memory");
}
// monotone u32 image of a float for ascending order; NaN -> 0 (below -inf)
__device__ __forceinline__ uint32_t fkey(float u) {
  const uint32_t b = __float_as_uint(u);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ double desc_key_inv(uint64_t key) {
  const uint64_t a = ~key;
  return __longlong_as_double((long long)((a & 0x8000000000000000ull) ? (a & 0x7fffffffffffffffull) : ~a));
}
// XCD-aware bijective block remap: consecutive logical blocks share one XCD's L2
__device__ __forceinline__ int xcd_logical(int b, int nb) {
  const int xcd = b & 7, slot = b >> 3, q8 = nb >> 3, r8 = nb & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// ---------------------------------------------------------------------------------------------
// prep: one wave per (padded) query.  qa[q] = the int8 piece a in natural dim order, d bytes;
// delta[q] = Delta_q in u units; alpha[q] = 1 / S, beta[q] = 0 (s' = alpha s + beta).
__global__ __launch_bounds__(256) void k5md_prep_kernel(const float* __restrict__ qf, int nq, int nq_pad, int dim,
                                                        int8_t* __restrict__ qa, double* __restrict__ delta,
                                                        double* __restrict__ alpha, double* __restrict__ beta) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), l = lane_id();
  if (q >= nq_pad) return;
  int8_t* o = qa + (int64_t)q * dim;
  if (q >= nq) {  // padding queries: zero pieces (their thresholds never accept)
    for (int i = l; i < dim; i += WAVE) o[i] = 0;
    if (l == 0) {
      delta[q] = 0.0;
      alpha[q] = 0.0;
      beta[q] = 0.0;
    }
    return;
  }
  const float* qv = qf + (int64_t)q * dim;
  float mx = 0.f;
  for (int i = l; i < dim; i += WAVE) mx = fmaxf(mx, fabsf(qv[i]));
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, WAVE));
  const double invS = mx > 0.f ? 127.0 / (double)mx : 1.0;
  double r2 = 0.0, q2 = 0.0;
  for (int i = l; i < dim; i += WAVE) {
    const double x = (double)qv[i] * invS;
    double a = rint(x);  // |a| <= 127
    a = a > 127.0 ? 127.0 : (a < -127.0 ? -127.0 : a);
    const double rho = x - a;  // exact, |rho| <= 1/2
    r2 += rho * rho;
    q2 += (double)qv[i] * (double)qv[i];
    o[i] = (int8_t)a;
  }
  r2 = wave_sum_f64(r2);
  q2 = wave_sum_f64(q2);
  constexpr double SLACK = 1.0 / (1 << 20);  // the header's sum of roundings, < 2^-20
  if (l == 0) {
    delta[q] = sqrt(r2) * (1.0 + SLACK) + SLACK * sqrt(q2) * invS;
    alpha[q] = invS;
    beta[q] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------
// The matrix pass.  DENSE = the sample pass (max of u over each lane row's rows of the chunk ->
// dv[q][chunk * 32 + lane row]) else the thresholded pass (u >= thr[q] -> candidate lists).  Chunk c covers
// rows [c * chunk_stride, + chunk_rows).  qbflag (retry pass): only query blocks holding a retried query.
//
// G... is empty, or one `const uint32_t* rows` (K5g, the gathered pass behind the *_rows calls): the pass then
// runs in virtual row space -- n = m = the length of the list, and chunks, tiles, the shifted last tile, the
// clamp of a short chunk and the staged hits are all in virtual rows v -- and only the DMA source addresses go
// through the list: the piece of tile row rr reads x8 + rows[v] * D, the norm lanes norms + rows[v].  A lane
// loads the list entry of each of its pieces (and of its norm lane) itself, PPW + 1 four-byte loads per tile
// from one or two cache lines, into gi[]: tile t + 2's entries are requested right after tile t + 1's piece
// went out (during tile t), so the wait_vm<0> at the top of tile t + 1 -- which is there for tile t + 1's
// DMA -- retires them, and the k-loop gets no wait and no cross-lane or LDS operation of its own.
template <int KS, bool DENSE, class... G>
__global__ __launch_bounds__(Shape<KS>::W * 64, 1) void k5md_pass_kernel(
    const int8_t* __restrict__ x8, const double* __restrict__ norms, int64_t n, const int8_t* __restrict__ qa, int nq,
    const float* __restrict__ thr, uint32_t* __restrict__ cand, int32_t* __restrict__ ccnt, int capc,
    int64_t chunk_rows, int64_t chunk_stride, int nchunks, int nqb, float* __restrict__ dv, int64_t dv_stride,
    const int32_t* __restrict__ qbflag, G... gather) {
  using S = Shape<KS>;
  constexpr bool GATHER = sizeof...(G) != 0;
  static_assert(sizeof...(G) <= 1, "one row list");
  constexpr int D = S::D, CPR = S::CPR, W = S::W, MB = S::MB, QW = S::QW, NE = S::NE, NA = S::NA, XB = S::XB;
  constexpr int TB = S::TB, PKT = S::PKT, PPW = S::PPW, DS = S::DS, TPS = S::TPS, EOFF = S::EOFF;
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * PKT];
  // per-(query, this chunk) list lengths (one row per wave), then each wave's hit stage
  __shared__ int32_t lcnt[W * QW + (DENSE ? 0 : W * STG)];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = lane_id(), r = l & 31, h = l >> 5;
  const int L = xcd_logical(blockIdx.x, gridDim.x);
  const int chunk = L / nqb, qb = L - chunk * nqb;
  if (chunk >= nchunks) return;
  if (qbflag && qbflag[qb] == 0) return;
  const int64_t row0 = (int64_t)chunk * chunk_stride;
  const int64_t row1 = (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  if (row0 >= row1) return;
  const int nrows = (int)(row1 - row0);
  const int ntiles = (nrows + GRT - 1) / GRT;
  const uint32_t sm0 = lds_addr(smem);

  // tile t covers chunk rows [tstart(t), tstart(t) + 32): the last tile of a ragged chunk is shifted back
  const bool tiny = nrows < GRT;
  auto tstart = [&](int t) { return tiny ? 0 : (t * GRT < nrows - GRT ? t * GRT : nrows - GRT); };
  auto lane_valid = [&](int t) { return tiny ? r < nrows : r >= t * GRT - tstart(t); };

  // LDS-DMA: piece p = w + W i of a tile fills LDS bytes [1024 p, + 1024) of the slot; lane l's 16 bytes are
  // slot g = 64 p + l = (tile row rr, slot-in-row cs), read from chunk cs ^ x(rr) of that row
  uint32_t loff[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int g = (w + W * i) * 64 + l, rr = g / CPR, cs = g % CPR;
    loff[i] = (uint32_t)(rr * D + ((cs ^ swz(CPR, rr)) << 4));
  }
  // K5g: gi[i] = the list entry (physical row) of this lane's tile row of piece i, gi[PPW] that of norm lane
  // l's row l >> 1, for the tile whose DMA goes out next; gvirt(t, i) = the virtual row it is read from
  uint32_t gi[GATHER ? PPW + 1 : 1];
  const uint32_t* const rows = gather_rows(gather...);
  auto gvirt = [&](int t, int i) {
    const int rr = i == PPW ? (l >> 1) : (int)(loff[i < PPW ? i : 0] / (uint32_t)D);
    return row0 + (tiny ? (rr < nrows ? rr : nrows - 1) : tstart(t) + rr);
  };
  auto issue_gathered = [&](int slot_i, int i) {  // piece i of the tile gi[] stands for
    uint8_t* slot = smem + slot_i * PKT;
    if (i == PPW) {
      const uint8_t* g = reinterpret_cast<const uint8_t*>(norms + gi[GATHER ? PPW : 0]) + 4 * (l & 1);
      uint8_t* ld = slot + TB;
      __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)ld, 4, 0, 0);
      return;
    }
    const int p = w + W * i;
    if (p >= KS) return;
    const uint32_t lo = loff[i < PPW ? i : 0];
    const uint8_t* g = reinterpret_cast<const uint8_t*>(x8) + (int64_t)gi[GATHER && i < PPW ? i : 0] * D + lo % (uint32_t)D;
    uint8_t* ld = slot + p * 1024;
    __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)ld, 16, 0, 0);
  };
  auto issue_piece = [&](int t, int slot_i, int i) {  // whole tiles; i == PPW: the tile's 32 norms
    if constexpr (GATHER) {
      issue_gathered(slot_i, i);
      // the same piece's entry two tiles on (the last tile again past the end: always a row of the list)
      if (i == PPW || w + W * i < KS) load_u32_async(gi[i], rows + gvirt(t + 1 < ntiles ? t + 1 : ntiles - 1, i));
      return;
    }
    const int64_t tr0 = row0 + tstart(t);
    uint8_t* slot = smem + slot_i * PKT;
    // (pointer arguments through locals: a compound expression makes the host pass drop the launch stub)
    if (i == PPW) {
      const uint8_t* g = reinterpret_cast<const uint8_t*>(norms + tr0) + 4 * l;
      uint8_t* ld = slot + TB;
      __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)ld, 4, 0, 0);
      return;
    }
    const int p = w + W * i;
    if (p >= KS) return;
    const uint8_t* g = reinterpret_cast<const uint8_t*>(x8) + tr0 * D + loff[i < PPW ? i : 0];
    uint8_t* ld = slot + p * 1024;
    __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)ld, 16, 0, 0);
  };
  auto issue_tiny = [&](int i) {  // the single tile of a chunk shorter than 32 rows: clamp rows
    if (i == PPW) {
      int64_t nr = row0 + (l >> 1);
      nr = nr < row1 ? nr : row1 - 1;
      const uint8_t* g = reinterpret_cast<const uint8_t*>(norms + nr) + 4 * (l & 1);
      uint8_t* ld = smem + TB;
      __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)ld, 4, 0, 0);
      return;
    }
    const int p = w + W * i;
    if (p >= KS) return;
    const uint32_t lo = loff[i < PPW ? i : 0];
    int64_t row = row0 + (int)(lo / D);
    row = row < row1 ? row : row1 - 1;
    const uint8_t* g = reinterpret_cast<const uint8_t*>(x8) + row * D + (lo % D);
    uint8_t* ld = smem + p * 1024;
    __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)ld, 16, 0, 0);
  };
  if constexpr (GATHER) {  // tile 0's entries (waited for here), its pieces, then tile 1's entries behind them
#pragma unroll
    for (int i = 0; i <= PPW; ++i) gi[i] = (i == PPW || w + W * i < KS) ? rows[gvirt(0, i)] : 0u;
  }
  static_for<0, PPW + 1>([&](auto I) {
    constexpr int i = decltype(I)::value;
    if constexpr (GATHER)
      issue_piece(0, 0, i);
    else if (tiny)
      issue_tiny(i);
    else
      issue_piece(0, 0, i);
  });

  // A fragments of this wave's M-blocks of 32 queries, every k-step -> accumulator file
  const int qbase = qb * S::QB + w * QW;
  v4i A[MB][KS];
#pragma unroll
  for (int j = 0; j < MB; ++j) {
    const int8_t* qp = qa + (int64_t)(qbase + 32 * j + r) * D + h * 16;
#pragma unroll
    for (int s = 0; s < KS; ++s) A[j][s] = *reinterpret_cast<const v4i*>(qp + s * 32);
  }
#pragma unroll
  for (int j = 0; j < MB; ++j)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+a"(A[j][s]));
  // test e of a lane: M-block e >> 4, accumulator register e & 15 -> query row of the wave
  auto qrow = [&](int e) { return 32 * (e >> 4) + ((e & 3) + 8 * ((e >> 2) & 3) + 4 * h); };
  float th[DENSE ? 1 : NE];
  if constexpr (!DENSE) {
#pragma unroll
    for (int e = 0; e < NE; ++e) th[e] = thr[qbase + qrow(e)];
    // landed before the tile loop (a wait for them inside it would also wait for the tile's DMA)
#pragma unroll
    for (int e = 0; e < NE; ++e) asm volatile("" : "+v"(th[e]));
  }

  // B fragment of k-step s for lane (r, h) = chunk 2s + h of tile row r: the swizzle touches the low XB
  // bits of the chunk index (NA addresses per lane), the bits above are an immediate offset
  uint32_t boff[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) boff[j] = (uint32_t)(r * D + (((2 * j + h) ^ swz(CPR, r)) << 4));

  const uint32_t lc0 = lds_addr(lcnt + w * QW);
  const uint32_t sg0 = lds_addr(lcnt + W * QW + (DENSE ? 0 : w * STG));  // this wave's hit stage
  int nst = 0;                                                         // staged entries (wave-uniform)
  if (!DENSE && l < QW) lcnt[w * QW + l] = 0;                          // visible after the first tile's barrier
  v16i acc[2][MB] = {};                                                // [tile parity][M-block]
  float ures[DENSE ? NE : 1];
#pragma unroll
  for (int e = 0; e < (DENSE ? NE : 1); ++e) ures[e] = __builtin_nanf("");
  uint32_t hm = 0, hmd = 0;  // hit bits (bit e = test e) of the tile being tested / of the tile before it
  float invc = 0.f, invp = 0.f;  // 1/||x|| of this lane's row of tiles t, t-1 (NaN: zero norm or a row seen before)
  const v16i zero = {};
  const int64_t qstride = (int64_t)nchunks * capc;

  // hit of query-in-wave ql at chunk row cr -> its (query, chunk) list; a list past capc keeps counting,
  // which the finish kernel reads as an overflow
  auto to_list = [&](int ql, int cr) {
    int pos;
    lds_add_rtn32(pos, lc0 + (uint32_t)(ql * 4), 1);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pos)::"memory");
    if (pos < capc) cand[(int64_t)(qbase + ql) * qstride + (int64_t)chunk * capc + pos] = (uint32_t)(row0 + cr);
  };
  auto drain = [&]() {  // the staged entries -> lists (once per chunk, or when the stage is nearly full)
    for (int i0 = 0; i0 < nst; i0 += 64) {
      const int i = i0 + l;
      int e = 0;
      if (i < nst) lds_read32(e, sg0 + (uint32_t)(i * 4));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e)::"memory");
      if (i < nst) to_list((int)((uint32_t)e >> 26), e & 0x3ffffff);
    }
    nst = 0;
  };
  auto flush = [&](int tt, uint32_t m) {  // hit bits of tile tt -> the stage
    if (__ballot(m != 0) == 0) return;
    const int lr = tstart(tt) + r;
    if (!__ballot((m & (m - 1)) != 0)) {
      // at most one hit per lane (the usual case): one staged entry per hit lane at its rank among them
      const uint64_t lanes = __ballot(m != 0);
      if (m) {
        int pos = nst + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(lanes >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lanes, 0));
        pos = pos < STG - 1 ? pos : STG - 1;  // (never binds: the stage drains above STG - 64)
        lds_write32(sg0 + (uint32_t)(pos * 4), (int)(((uint32_t)qrow(__builtin_ctz(m)) << 26) | (uint32_t)lr));
      }
      nst += __popcll(lanes);
      if (nst > STG - 64) drain();
    } else {
      for (int e = 0; e < NE; ++e)  // several hits in a lane: straight to the lists
        if ((m >> e) & 1u) to_list(qrow(e), lr);
    }
  };
  // u of test e from one tile's accumulators (NaN for rows without a score); the thresholded pass folds the
  // threshold in (one fma: the sign of f32(A) * inv - thr, no rounding in between)
  auto test = [&](const v16i (&a)[MB], int e, float inv) {
    const float f = (float)a[e >> 4][e & 15];
    if constexpr (DENSE)
      ures[e] = fmaxf(ures[e], f * inv);
    else
      hm |= fmaf(f, inv, -th[e]) >= 0.f ? (1u << e) : 0u;
  };

  int sl = 0;  // t & 1
  auto tile = [&](auto PAR, auto FIRST, int t) {
    constexpr int p = decltype(PAR)::value;
    constexpr bool first = decltype(FIRST)::value;  // tile 0: no previous tile to test
    // tile t's DMA landed (this wave's part; the barrier covers the other waves'), and every wave is done
    // reading the slot that tile t + 1 overwrites
    wait_vm<0>();
    if constexpr (GATHER) {  // ... and so did the list entries requested behind it
#pragma unroll
      for (int i = 0; i <= PPW; ++i) asm volatile("" : "+v"(gi[i]));
    }
    barrier_all();
    const uint32_t slot = sm0 + (uint32_t)(sl * PKT);
    const bool dma = t + 1 < ntiles;
    const int tn = dma ? t + 1 : t;
    double nv = 0.0;
    lds_read_f64(nv, slot + TB + (uint32_t)(r * 8));
    uint32_t badr[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) badr[j] = slot + boff[j];
    v4i ring[NR];
    auto readB = [&](auto SS) {
      constexpr int s = decltype(SS)::value;
      lds_read128_off<(s >> (XB - 1)) * (16 << XB)>(ring[s & (NR - 1)], badr[s & (NA - 1)]);
    };
    static_for<0, BA>([&](auto SS) { readB(SS); });
    VRQ_SCHED_FENCE();
    static_for<0, KS>([&](auto SS) {
      constexpr int s = decltype(SS)::value;
      if constexpr (s + BA < KS) {
        readB(std::integral_constant<int, s + BA>{});
        // all but the BA newest LDS operations are complete: B(s), and the norm (issued before B(0))
        asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(ring[s & (NR - 1)]), "+v"(nv) : "n"(BA) : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(ring[s & (NR - 1)]) : "n"(KS - 1 - s) : "memory");
      }
#pragma unroll
      for (int j = 0; j < MB; ++j) acc[p][j] = mfma_i8(A[j][s], ring[s & (NR - 1)], s == 0 ? zero : acc[p][j]);
#pragma unroll
      for (int j = 0; j < MB; ++j) asm volatile("" : "+v"(acc[p][j]));
      if constexpr (s == 1 && !DENSE) {
        if (t >= 2) flush(t - 2, hmd);
        VRQ_SCHED_FENCE();
      }
      // DMA of tile t + 1, spread over the MFMA shadow
      if constexpr (s >= 2 && (s - 2) % DS == 0 && (s - 2) / DS <= PPW)
        if (dma) issue_piece(tn, sl ^ 1, (s - 2) / DS);
      // threshold tests / dense values of tile t-1
      if constexpr (!first && s >= EOFF && (s - EOFF) * TPS < NE) {
#pragma unroll
        for (int e = (s - EOFF) * TPS; e < (s - EOFF + 1) * TPS && e < NE; ++e) {
          test(acc[p ^ 1], e, invp);
          // pin the test at this k-step (IR-level sinking would gather them behind the last MFMA)
          if constexpr (DENSE)
            asm volatile("" : "+v"(ures[e]));
          else
            asm volatile("" : "+v"(hm));
        }
      }
      if constexpr (s == KS / 2) {  // 1/||x|| of this tile's row r (branch-free)
        const float rc = __builtin_amdgcn_rcpf((float)nv);
        invc = ((nv > 0.0) & lane_valid(t)) ? rc : __builtin_nanf("");
      }
      VRQ_SCHED_FENCE();
    });
    invp = invc;
    hmd = hm;
    hm = 0;
    sl ^= 1;
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using NOTFIRST = std::integral_constant<bool, false>;
  tile(I0{}, std::integral_constant<bool, true>{}, 0);
  int t = 1;
  for (; t + 1 < ntiles; t += 2) {
    tile(I1{}, NOTFIRST{}, t);
    tile(I0{}, NOTFIRST{}, t + 1);
  }
  if (t < ntiles) tile(I1{}, NOTFIRST{}, t);
  wait_vm<0>();
  // tile ntiles-2 (tested during the last tile), then the last tile itself
  if (!DENSE && ntiles >= 2) flush(ntiles - 2, hmd);
  const int pl = (ntiles - 1) & 1;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    if (pl)
      test(acc[1], e, invp);
    else
      test(acc[0], e, invp);
  }
  if constexpr (DENSE) {  // the lane maxima of the chunk -> dv[q][chunk * 32 + r]
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int q = qbase + qrow(e);
      if (q < nq) dv[(int64_t)q * dv_stride + (int64_t)chunk * GRT + r] = ures[e];
    }
  } else {
    flush(ntiles - 1, hm);
    drain();
    wait_lgkm0();
    if (l < QW && qbase + l < nq) ccnt[(int64_t)(qbase + l) * nchunks + chunk] = lcnt[w * QW + l];
  }
}

// ---------------------------------------------------------------------------------------------
// select (K5's gemm_select_kernel): per query, U = k-th largest valid value of dv (nsc sample chunks of 32
// lane maxima; 3-pass radix select on the monotone key), thr = U - 2 Delta rounded down (-inf when the
// sample holds fewer than k finite values); zeroes the query's list lengths.  Padding queries: thr = +inf.
__global__ __launch_bounds__(256) void k5md_select_kernel(const float* __restrict__ dv, int64_t dv_stride,
                                                          int64_t sstride, int nsc, int64_t n, int k,
                                                          const double* __restrict__ delta, float* __restrict__ thr,
                                                          int32_t* __restrict__ ccnt, int nchunks, int nq,
                                                          int32_t* __restrict__ qbflag, int nqb) {
  __shared__ uint32_t hist[2048];
  __shared__ uint32_t res[3];
  const int q = blockIdx.x, tid = threadIdx.x;
  if (q == 0)
    for (int i = tid; i < nqb; i += 256) qbflag[i] = 0;
  if (q >= nq) {
    if (tid == 0) thr[q] = __builtin_inff();
    return;
  }
  for (int i = tid; i < nchunks; i += 256) ccnt[(int64_t)q * nchunks + i] = 0;
  const float* d = dv + (int64_t)q * dv_stride;
  uint32_t prefix = 0, pmask = 0;
  int kk = k;
  bool ok = true;
  constexpr int SH[3] = {21, 10, 0}, NBITS[3] = {11, 11, 10};
  for (int pass = 0; pass < 3 && ok; ++pass) {
    const int sh = SH[pass];
    const uint32_t dm = (1u << NBITS[pass]) - 1;
    for (int i = tid; i < 2048; i += 256) hist[i] = 0;
    __syncthreads();
    for (int c = 0; c < nsc; ++c) {
      const int64_t rb = (int64_t)c * sstride;
      const int64_t len = (rb + GRT <= n) ? GRT : (n > rb ? n - rb : 0);
      if (tid < len) {
        const uint32_t key = fkey(d[(int64_t)c * GRT + tid]);
        if ((key & pmask) == prefix) atomicAdd(&hist[(key >> sh) & dm], 1u);
      }
    }
    __syncthreads();
    if (tid < 64) {  // top-down search: lane L owns bins [32L, 32L + 32)
      uint32_t loc = 0;
      for (int i = 0; i < 32; ++i) loc += hist[tid * 32 + i];
      uint32_t suf = loc;  // inclusive suffix sum over lanes >= tid
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_down(suf, o, 64);
        if (tid + o < 64) suf += y;
      }
      uint32_t above = suf - loc;
      int found = -1;
      uint32_t abv = 0;
      for (int i = 31; i >= 0; --i) {
        const uint32_t hc = hist[tid * 32 + i];
        if (above < (uint32_t)kk && above + hc >= (uint32_t)kk) {
          found = tid * 32 + i;
          abv = above;
        }
        above += hc;
      }
      const uint64_t bal = __ballot(found >= 0);
      if (tid == 0) res[0] = bal ? 1u : 0u;
      if (found >= 0) {
        res[1] = (uint32_t)found;
        res[2] = abv;
      }
    }
    __syncthreads();
    if (!res[0]) {
      ok = false;
    } else {
      kk -= (int)res[2];
      prefix |= res[1] << sh;
      pmask |= dm << sh;
    }
    __syncthreads();
  }
  if (tid == 0) {
    float t = -__builtin_inff();
    if (ok && prefix != 0u) t = __double2float_rd((double)fkey_inv(prefix) - 2.0 * delta[q]);
    thr[q] = t;
  }
}

// ---------------------------------------------------------------------------------------------
// exact (score desc, row asc) pair sort in LDS: ascending (key, row), key = desc_key_f64(score)
__device__ inline void sort_pairs(uint64_t* key, uint32_t* row, int n_pow2) {
  for (int size = 2; size <= n_pow2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < (n_pow2 >> 1); i += blockDim.x) {
        const int lo = ((i / stride) * stride * 2) + (i % stride), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t ka = key[lo], kb = key[hi];
        const uint32_t ra = row[lo], rb = row[hi];
        const bool gt = ka > kb || (ka == kb && ra > rb);
        if (gt == up) {
          key[lo] = kb;
          key[hi] = ka;
          row[lo] = rb;
          row[hi] = ra;
        }
      }
    }
  }
  __syncthreads();
}

// The reference score of one row, one wave: phase3_cos_dim's lane -> dims map and order (lane l takes dims
// 2l, 2l+1 of every 128-dim block; exact products, f64 sum, one rounding to f32, f64 division), with the
// query read from LDS.
__device__ __forceinline__ double cos_row(const float* qs, const int8_t* __restrict__ xrow, double nrm, int dim) {
  double s = 0.0;
  for (int d = 2 * lane_id(); d < dim; d += 2 * WAVE) {
    const char2 x = *reinterpret_cast<const char2*>(xrow + d);
    const float2 qq = *reinterpret_cast<const float2*>(qs + d);
    s += (double)qq.x * (double)x.x;
    s += (double)qq.y * (double)x.y;
  }
  s = wave_sum_f64(s);
  const float f = (float)s;
  return nrm == 0.0 ? -__builtin_inf() : (double)f / nrm;
}

// =============================================================================================
// Finish and exact scan: one stage for the three scores.  A score family F -- Int8Cos, FloatIP<KS>, Binary --
// is the kernels' first argument; it holds the corpus pointers and is everything a score has of its own:
//   F::OCC                 workgroups per CU asked of the compiler (the launch bound)
//   F::Lds                 the LDS of its per-workgroup query state, a base of FinShared (empty: FloatIP's
//                          query is in registers)
//   f.query(qf, q, sh)     makes query q ready and returns the state score_batch takes; what it writes to LDS is
//                          published by the caller's next barrier
//   f.score_batch(qs, base, end, count, row_at, admit)
//                          scores the candidates row_at(j), base <= j < end <= count, and hands each to
//                          admit(mine, key, row), mine = this thread speaks for the row: how candidates are dealt
//                          to threads or waves and the order of the loads
// and, on the host, its prep-kernel launch, its pass-kernel launch and family<KS>(), the device family at a dim.
constexpr int FIN_NT = 512, FIN_NW = FIN_NT / WAVE;
template <class QS>
struct FinShared : QS {
  uint64_t key[KMAX5 + FB_BATCH];
  uint32_t row[KMAX5 + FB_BATCH];
  int32_t pre[MAX_CHUNKS + 1];  // exclusive prefix of the (capped) list lengths
  int32_t fill, over;
};

// Running exact top-k over candidate rows row_at(j), j < count, in batches of FB_BATCH: a row enters the LDS
// sort only if it beats the current k-th by (score desc, row asc).  key/row[0..kc) hold the list in order after
// each batch.  All threads call it; returns kc = min(k, count).  count >= 1.
template <class F, class Q, class RowAt, class Sh>
__device__ __forceinline__ int running_topk(const F& f, const Q& qs, int64_t count, RowAt row_at, int k, Sh& sh) {
  const int tid = threadIdx.x;
  if (tid == 0) sh.fill = 0;
  int kc = 0;
  __syncthreads();
  for (int64_t base = 0; base < count; base += FB_BATCH) {
    const uint64_t kk = kc == k ? sh.key[k - 1] : KEY_NONE;
    const uint32_t kr = kc == k ? sh.row[k - 1] : 0xffffffffu;
    const int64_t end = base + FB_BATCH < count ? base + FB_BATCH : count;
    f.score_batch(qs, base, end, count, row_at, [&](bool mine, uint64_t key_r, uint32_t rr) {
      if (mine && (kc < k || key_r < kk || (key_r == kk && rr < kr))) {
        const int i = kc + atomicAdd(&sh.fill, 1);
        sh.key[i] = key_r;
        sh.row[i] = rr;
      }
    });
    __syncthreads();
    const int fl = sh.fill;
    if (fl > 0) {
      const int tot = kc + fl, np2 = next_pow2(tot);
      for (int i = tot + tid; i < np2; i += FIN_NT) {
        sh.key[i] = KEY_NONE;
        sh.row[i] = 0xffffffffu;
      }
      sort_pairs(sh.key, sh.row, np2);
      kc = tot < k ? tot : k;
    }
    __syncthreads();
    if (tid == 0) sh.fill = 0;
    __syncthreads();
  }
  return kc;
}

template <class Sh>
__device__ __forceinline__ void write_result(int q, int k, int kc, int64_t row_offset, const Sh& sh,
                                             int32_t* out_count, int64_t* out_rows, double* out_scores) {
  for (int i = threadIdx.x; i < k; i += FIN_NT) {
    const int64_t o = (int64_t)q * k + i;
    out_rows[o] = i < kc ? (int64_t)sh.row[i] + row_offset : -1;
    out_scores[o] = i < kc ? desc_key_inv(sh.key[i]) : __builtin_nan("");
  }
  if (threadIdx.x == 0) out_count[q] = kc;
}

// finish (K5's contract): the query's lists -> exact scores -> running top-k, with fb_flag: 0 = served,
// 2 = retry (a list overflowed with >= min(k, n) candidates recorded: the recorded k-th score s_k bounds the
// true one from below, so thr = alpha s_k + beta - Delta keeps every row of the exact top-k), 1 = exact scan
// (fewer than min(k, n) candidates, or an overflow in the retry pass).  RETRY serves the retried queries.
// G... as in k5md_pass_kernel: with a row list the lists hold virtual rows, n is the list's length, and row_at
// hands out rows[v] -- ascending like v, so scores, ties and outputs are those of the physical rows.
template <class F, bool RETRY, class... G>
__global__ __launch_bounds__(FIN_NT, F::OCC) void k5m_finish_kernel(
    const F f, int64_t n, int64_t row_offset, const float* __restrict__ qf, int k,
    const uint32_t* __restrict__ cand, const int32_t* __restrict__ ccnt, int nchunks, int capc, int qpb,
    int32_t* __restrict__ out_count, int64_t* __restrict__ out_rows, double* __restrict__ out_scores,
    int32_t* __restrict__ fb_flag, float* __restrict__ thr, const double* __restrict__ alpha,
    const double* __restrict__ beta, const double* __restrict__ delta, int32_t* __restrict__ qbflag, G... gather) {
  __shared__ FinShared<typename F::Lds> sh;
  constexpr bool GATHER = sizeof...(G) != 0;
  const uint32_t* const rows = gather_rows(gather...);
  const int q = blockIdx.x, tid = threadIdx.x;
  if (RETRY && fb_flag[q] != 2) return;
  if (tid == 0) sh.over = 0;
  __syncthreads();
  const int32_t* cq = ccnt + (int64_t)q * nchunks;
  for (int c = tid; c < nchunks; c += FIN_NT) {
    const int x = cq[c];
    if (x > capc) sh.over = 1;
    sh.pre[c + 1] = x < capc ? x : capc;
  }
  const auto qs = f.query(qf, q, sh);
  __syncthreads();
  if (tid < WAVE) {  // inclusive scan of pre[1 .. nchunks] by one wave: 32 entries per lane, then the lanes
    constexpr int PER = MAX_CHUNKS / WAVE;
    int part = 0;
    for (int i = 0; i < PER; ++i) {
      const int c = tid * PER + i;
      if (c < nchunks) part += sh.pre[c + 1];
    }
    int incl = part;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int y = __shfl_up(incl, d, WAVE);
      if (tid >= d) incl += y;
    }
    int run = incl - part;
    for (int i = 0; i < PER; ++i) {
      const int c = tid * PER + i;
      if (c < nchunks) {
        run += sh.pre[c + 1];
        sh.pre[c + 1] = run;
      }
    }
    if (tid == 0) sh.pre[0] = 0;
  }
  __syncthreads();
  const int total = sh.pre[nchunks];
  const int need = (int)((int64_t)k < n ? k : n);
  const bool over = sh.over != 0;
  if (total < need || (RETRY && over)) {
    if (tid == 0) {
      fb_flag[q] = 1;
      thr[q] = __builtin_inff();
    }
    return;
  }
  const uint32_t* Cq = cand + (int64_t)q * nchunks * capc;
  // candidate j of the concatenated lists: the largest chunk lo with pre[lo] <= j (fixed 11 steps)
  auto row_at = [&](int64_t j) {
    int lo = 0;
#pragma unroll
    for (int st = MAX_CHUNKS / 2; st > 0; st >>= 1) {
      const int mid = lo + st;
      if (mid < nchunks && sh.pre[mid] <= j) lo = mid;
    }
    const uint32_t v = Cq[(int64_t)lo * capc + (j - sh.pre[lo])];
    if constexpr (GATHER) return rows[v];
    return v;
  };
  const int kc = running_topk(f, qs, total, row_at, k, sh);
  if (!RETRY && over) {
    if (tid == 0) {
      const double t2 = alpha[q] * desc_key_inv(sh.key[kc - 1]) + beta[q] - delta[q];
      thr[q] = __double2float_rd(t2 - 1e-9 * fabs(t2));
      fb_flag[q] = 2;
      atomicOr(&qbflag[q / qpb], 1);
    }
    return;
  }
  write_result(q, k, kc, row_offset, sh, out_count, out_rows, out_scores);
  if (tid == 0) {
    fb_flag[q] = 0;
    thr[q] = __builtin_inff();
  }
}

// the exact scan of the flagged queries (heavy ties, zero-norm rows): one workgroup per flagged query scores
// every row (of the list) through the family's own rounds and score function; skip (VRQ_GEMM_NO_FALLBACK)
// reports the query as unserved instead.  running_topk's first barrier publishes the query state.
template <class F, class... G>
__global__ __launch_bounds__(FIN_NT, F::OCC) void k5m_fallback_kernel(
    const F f, int64_t n, int64_t row_offset, const float* __restrict__ qf, int k, int32_t* __restrict__ out_count,
    int64_t* __restrict__ out_rows, double* __restrict__ out_scores, const int32_t* __restrict__ fb_flag, bool skip,
    G... gather) {
  __shared__ FinShared<typename F::Lds> sh;
  const uint32_t* const rows = gather_rows(gather...);
  const int q = blockIdx.x, tid = threadIdx.x;
  if (fb_flag[q] != 1) return;
  if (skip) {
    for (int i = tid; i < k; i += FIN_NT) {
      out_rows[(int64_t)q * k + i] = -1;
      out_scores[(int64_t)q * k + i] = __builtin_nan("");
    }
    if (tid == 0) out_count[q] = -1;
    return;
  }
  const auto qs = f.query(qf, q, sh);
  const int kc = running_topk(
      f, qs, n, [=](int64_t j) { return sizeof...(G) ? rows[j] : (uint32_t)j; }, k, sh);
  write_result(q, k, kc, row_offset, sh, out_count, out_rows, out_scores);
}

// K5md's score: int8 rows by cos_row, the float query in LDS, one row per wave and round.
struct Int8Cos {
  const int8_t* x8;
  const double* norms;
  int dim;
  static constexpr int OCC = 1;
  struct Lds {
    float q[2048];
  };
  template <class Sh>
  __device__ __forceinline__ const float* query(const float* __restrict__ qf, int q, Sh& sh) const {
    for (int i = threadIdx.x; i < dim; i += FIN_NT) sh.q[i] = qf[(int64_t)q * dim + i];
    return sh.q;
  }
  template <class RowAt, class Admit>
  __device__ __forceinline__ void score_batch(const float* qs, int64_t base, int64_t end, int64_t, RowAt row_at,
                                              Admit admit) const {
    const int l = lane_id(), w = threadIdx.x >> 6;
    for (int64_t j = base + w; j < end; j += FIN_NW) {
      const uint32_t rr = row_at(j);
      admit(l == 0, desc_key_f64(cos_row(qs, x8 + (int64_t)rr * dim, norms[rr], dim)), rr);
    }
  }
  template <class... A>
  void prep(dim3 grid, hipStream_t s, A... a) const {
    hipLaunchKernelGGL(k5md_prep_kernel, grid, dim3(256), 0, s, a...);
  }
  template <int KS, bool DENSE, class... A>
  void pass(dim3 grid, dim3 blk, hipStream_t s, A... a) const {
    hipLaunchKernelGGL((k5md_pass_kernel<KS, DENSE>), grid, blk, 0, s, x8, norms, a...);
  }
  template <int KS>
  Int8Cos family() const {
    return *this;
  }
};

// ---------------------------------------------------------------------------------------------
struct Plan {
  int qpb, nqb, nq_pad;  // queries per block (by dim), query blocks, padded queries
  int64_t scr, sstride, scols;
  int nsc;
  int64_t chunk_rows;
  int nchunks, capc;
  size_t off_delta, off_alpha, off_beta, off_qbf, off_thr, off_flag, off_cnt, off_cand, off_dv, bytes;
};

// dim -> KS = dim / 32, the one place: fn(std::integral_constant<int, KS>) -> int at a served dim, else
// VRQ_EUNSUPPORTED.  KS = 32 exists for the gathered calls only (the *_rows calls; unfiltered 1024 is K5's).
template <class Fn>
static int with_ks(int dim, bool gather, Fn fn) {
  switch (dim) {
    case 256: return fn(std::integral_constant<int, 8>{});
    case 384: return fn(std::integral_constant<int, 12>{});
    case 512: return fn(std::integral_constant<int, 16>{});
    case 768: return fn(std::integral_constant<int, 24>{});
    case 1024: return gather ? fn(std::integral_constant<int, 32>{}) : VRQ_EUNSUPPORTED;
    case 1536: return fn(std::integral_constant<int, 48>{});
    case 2048: return fn(std::integral_constant<int, 64>{});
    default: return VRQ_EUNSUPPORTED;
  }
}

__host__ inline int queries_per_block(int dim, bool gather = false) {  // 0: no pass at this dim
  const int qb = with_ks(dim, gather, [](auto KS) { return Shape<decltype(KS)::value>::QB; });
  return qb > 0 ? qb : 0;
}

// K5's planning rules (gemm_plan) with the query block a function of dim
__host__ inline int plan_shape(int64_t n, int dim, int nq, int k, Plan* p, bool gather = false) {
  p->qpb = queries_per_block(dim, gather);
  if (p->qpb == 0 || n < 1 || n >= (int64_t(1) << 32) || nq < 1 || k < 1 || k > KMAX5) return VRQ_EUNSUPPORTED;
  p->nqb = (nq + p->qpb - 1) / p->qpb;
  p->nq_pad = p->nqb * p->qpb;
  const int want1 = 256 / p->nqb > 0 ? 256 / p->nqb : 1;  // one workgroup per CU and query block
  const int want = want1 * kChunkMult;
  int64_t S = (int64_t)((double)CAP_MULT * (double)k * (double)n / (double)FIN_CAP);
  if (S < kMinSample) S = kMinSample;
  if (S > kMaxSample) S = kMaxSample;
  if (S > n) S = n;
  int64_t nsc = want1 > (2 * (int64_t)k + GRT - 1) / GRT ? want1 : (2 * (int64_t)k + GRT - 1) / GRT;
  const int64_t scr = ((S + nsc - 1) / nsc + GRT - 1) / GRT * GRT;
  nsc = (S + scr - 1) / scr;
  p->scr = scr;
  p->nsc = (int)nsc;
  p->sstride = n / nsc >= scr ? n / nsc : scr;  // chunks never overlap; the last may be cut at n
  p->scols = nsc * GRT;
  int64_t cr = (n + want - 1) / want;
  cr = (cr + GRT - 1) / GRT * GRT;
  if ((n + cr - 1) / cr > MAX_CHUNKS) cr = ((n + MAX_CHUNKS - 1) / MAX_CHUNKS + GRT - 1) / GRT * GRT;
  if (cr > kMaxChunkRows) cr = kMaxChunkRows;
  p->chunk_rows = cr;
  p->nchunks = (int)((n + cr - 1) / cr);
  const int64_t expect = ((int64_t)k * cr + S - 1) / S;
  int capc = 64;
  while (capc < CAP_MULT * expect && capc < 4096) capc <<= 1;
  while (capc < 512 && (double)nq * p->nchunks * (2 * capc) * sizeof(uint32_t) <= (double)(1 << 30)) capc <<= 1;
  p->capc = capc;
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  p->off_delta = al((size_t)p->nq_pad * dim);
  p->off_alpha = p->off_delta + al((size_t)p->nq_pad * sizeof(double));
  p->off_beta = p->off_alpha + al((size_t)p->nq_pad * sizeof(double));
  p->off_qbf = p->off_beta + al((size_t)p->nq_pad * sizeof(double));
  p->off_thr = p->off_qbf + al((size_t)p->nqb * sizeof(int32_t));
  p->off_flag = p->off_thr + al((size_t)p->nq_pad * sizeof(float));
  p->off_cnt = p->off_flag + al((size_t)nq * sizeof(int32_t));
  p->off_cand = p->off_cnt + al((size_t)nq * p->nchunks * sizeof(int32_t));
  p->off_dv = p->off_cand + al((size_t)nq * p->nchunks * p->capc * sizeof(uint32_t));
  p->bytes = p->off_dv + al((size_t)nq * p->scols * sizeof(float));
  return VRQ_OK;
}

// the plan of vrq_gemm_topk_dim_mfma*: the int8-cosine mode alone
__host__ inline int plan(int mode, int64_t n, int dim, int nq, int k, Plan* p) {
  if (mode == VRQ_GEMM_FLOAT_IP) return VRQ_EINVAL;
  if (mode != VRQ_GEMM_INT8_COSINE) return VRQ_EUNSUPPORTED;
  return plan_shape(n, dim, nq, k, p);
}

// "auto": the smallest batch from which K5md beat K5d by more than the run-to-run spread at that dim
// (profiles/exhaustive_mfma_bench.jsonl; measured at nq = 1, 8, 64, 1024); 0 = not measured, stays on K5d
__host__ inline int min_batch(int dim) {
  switch (dim) {
    case 256: case 384: case 512: case 768: return 8;  // 1.08x-1.57x at nq = 8, 0.24x-0.27x at nq = 1
    case 1536: case 2048: return 64;                   // 0.92x / 0.75x at nq = 8, 4.7x / 4.5x at nq = 64
    default: return 0;
  }
}

// =============================================================================================
// K5mf: exact float32 inner-product top-k (IndexFlatIP) on the matrix cores at the same six dims, behind
// vrq_flat_ip_topk_dim_mfma.  The sample and main passes are k5md_pass_kernel over flat_ip_prepare's operands
// (x8 = the per-row-scaled int8 image b_r of the float rows, inv_scale = 1 / s_r in the place of the norms:
// u = f32(<a, b_r>) * (1 / f32(inv_scale_r)) ~ s_r <a, b_r>), as K5 does at 1024; select, the plan and the
// list layout are K5md's.  New here: the corpus preparation and the query prep at a run-time dim, and a
// finish (and exact scan) that rescores float rows, 4 d bytes each.
//
// Delta = (||rho|| B0 + ||q/S|| B1)(1 + eps) + eps (||q/S|| + ||rho||) B0, eps = 2^-20, (B0, B1) = the corpus
// bounds max ||s_r b_r||, max ||x_r - s_r b_r||.  Exact part: u* - s'* = <a - q/S, s_r b_r> - <q/S, x_r - s_r b_r>,
// so |u* - s'*| <= ||rho|| B0 + ||q/S|| B1 (Cauchy-Schwarz; d does not enter).  Roundings for d <= 2048:
//   u path, relative to |u*| = |s_r <a, b_r>| <= ||a|| B0 <= (||q/S|| + ||rho||) B0:
//     A = <a, b_r> is exact in i32, |A| <= 127 * 127 * 2048 < 2^25: v_cvt_f32_i32 rounds above 2^24, i.e. at
//     d = 1536 and 2048 (2^-24); inv_scale f64 -> f32 (2^-24; its own f64 rounding, 2^-53, is far below);
//     v_rcp_f32 (1 ulp: 2^-23); the product (2^-24; the main pass tests the sign of one fma instead):
//     (1 + 2^-24)^3 (1 + 2^-23) - 1 < 2^-21.
//   reference s' = f32(<q, x_r>) / S: 2^-24 |<q/S, x_r>| <= 2^-24 ||q/S|| (B0 + B1).
//   Sum <= (2^-21 + 2^-24)(||q/S|| + ||rho||) B0 + 2^-24 ||q/S|| B1 < eps (||q/S|| + ||rho||) B0 + eps ||q/S|| B1:
//   the first is Delta's last term, the second is inside the (1 + eps) factor on the B1 term.  eps = 2^-20
//   holds at every d <= 2048 with a factor 1.7 to spare; no dim needs a wider one.
//
// Finish (the shared stage with FloatIP<KS>): one workgroup of 8 waves per query, the query slice in registers
// (lane l holds the 16-byte pieces l + 64 i of the query, i < NP = ceil(d / 256)).  A wave scores R candidate
// rows per round: lanes j < R each resolve one candidate (a fixed-trip binary search of the list prefix in
// LDS, then the list entry) for the NEXT round while this round's rows are in flight; the wave issues the
// R * NP global_load_dwordx4 of all R rows back to back (wave-uniform row base from v_readlane, consecutive
// lanes read consecutive pieces) and scores row i under a counted vmcnt wait while rows i + 1 .. R - 1 are
// still landing.  Score: flat_score_dim, one summation order for the finish and for the exact scan.
// Admission, retry and flags are the shared stage's; a round whose rows all fail the test against the k-th key touches
// no LDS.  R per dim keeps the row registers (4 R NP) near 96: 8 rows up to 512, 6 at 768, 4 at 1536, 3 at
// 2048; -DVRQ_G5F_R=n overrides it at every dim (the R = 1 A/B of DESIGN section 5 "K5mf").
#ifndef VRQ_G5F_R
#define VRQ_G5F_R 0
#endif

typedef float v4f __attribute__((ext_vector_type(4)));

template <int KS>
struct FShape {
  static constexpr int D = 32 * KS, PCS = D / 4;    // 16-byte pieces of a float row
  static constexpr int NP = (PCS + 63) / 64;        // piece rounds: lane l takes pieces l + 64 i
  static constexpr int REM = PCS - 64 * (NP - 1);   // lanes of the last round (32 at d = 384, else 64)
  static constexpr int R = VRQ_G5F_R > 0 ? VRQ_G5F_R : (KS <= 16 ? 8 : KS <= 24 ? 6 : KS <= 48 ? 4 : 3);
  static constexpr int OCC = KS <= 24 ? 2 : 1;      // finish workgroups per CU the register budget allows
  static constexpr int RPW = NP <= 1 ? 8 : NP <= 3 ? 4 : 2;  // corpus preparation: rows in flight per wave
};

template <int KS>
struct FSlice {
  v4f v[FShape<KS>::NP];
};

// this lane's pieces of one float row (zeros where the last round has no piece for the lane)
template <int KS>
__device__ __forceinline__ void fslice_load(FSlice<KS>& x, const float* __restrict__ row) {
  using F = FShape<KS>;
  const v4f* p = reinterpret_cast<const v4f*>(row) + lane_id();
#pragma unroll
  for (int i = 0; i < F::NP; ++i) {
    if (i < F::NP - 1 || F::REM == 64) {
      x.v[i] = p[64 * i];
    } else {
      x.v[i] = v4f{0.f, 0.f, 0.f, 0.f};
      if (lane_id() < F::REM) x.v[i] = p[64 * i];
    }
  }
}

// The float inner product of the finish and of the exact scan: (double)(float)(sum q_i x_i), every product
// exact in f64 (the fma rounds once, the sum), the lane's pieces in the order i = 0 .. NP - 1, then the wave
// butterfly.  Under the exactness condition of exact_scores.h the f64 sum is exact in every order and this
// is the one correct f32 rounding of the dot (K5d's and the oracle's bits); otherwise one of its two
// f32 neighbours.
template <int KS>
__device__ __forceinline__ double flat_score_dim(const FSlice<KS>& q, const FSlice<KS>& x) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < FShape<KS>::NP; ++i) {
    s = __builtin_fma((double)q.v[i].x, (double)x.v[i].x, s);
    s = __builtin_fma((double)q.v[i].y, (double)x.v[i].y, s);
    s = __builtin_fma((double)q.v[i].z, (double)x.v[i].z, s);
    s = __builtin_fma((double)q.v[i].w, (double)x.v[i].w, s);
  }
  return (double)(float)wave_sum_f64(s);
}

// ---------------------------------------------------------------------------------------------
// Corpus preparation at dim 32 KS (flat_ip_prepare_kernel's definitions): a wave takes RPW whole rows, all
// their loads in flight before the first max|x| reduction; the int8 image leaves as 16-byte stores (a quad
// of lanes hands its four packed dwords to its first lane).  Rows past n are the last row again (the
// maxima are idempotent; nothing is stored for them).
template <int KS>
__global__ __launch_bounds__(256) void k5mf_prepare_kernel(const float* __restrict__ xf, int64_t n,
                                                           int8_t* __restrict__ x8, double* __restrict__ inv_scale,
                                                           unsigned long long* __restrict__ bounds) {
  using F = FShape<KS>;
  constexpr int D = F::D, NP = F::NP, RPW = F::RPW;
  __shared__ double sb[2][4];
  const int w = threadIdx.x >> 6, l = lane_id();
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + w) * RPW;
  FSlice<KS> x[RPW];
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int64_t r = r0 + j < n ? r0 + j : n - 1;
    fslice_load(x[j], xf + r * D);
  }
  double ex = 0.0, es = 0.0;
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int64_t r = r0 + j < n ? r0 + j : n - 1;
    const bool store = r0 + j < n;
    float mxl = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
      mxl = fmaxf(fmaxf(mxl, fmaxf(fabsf(x[j].v[i].x), fabsf(x[j].v[i].y))),
                  fmaxf(fabsf(x[j].v[i].z), fabsf(x[j].v[i].w)));
    const float mx = (float)wave_allreduce64((double)mxl, [](double a, double b) { return fmax(a, b); });
    const bool live = mx >= 1e-30f;
    const double sc = live ? (double)mx / 127.0 : 0.0, inv = live ? 127.0 / (double)mx : 0.0;
    double b2 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const float xe[4] = {x[j].v[i].x, x[j].v[i].y, x[j].v[i].z, x[j].v[i].w};
      uint32_t pk = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double b = rint((double)xe[e] * inv);
        b = b > 127.0 ? 127.0 : (b < -127.0 ? -127.0 : b);
        const double rs = (double)xe[e] - sc * b;
        b2 += b * b;
        s2 += rs * rs;
        pk |= ((uint32_t)(int32_t)b & 0xffu) << (8 * e);
      }
      // quad_perm broadcasts of the quad's lanes 0..3: every lane of a quad holds its 16 bytes
      const uint32_t a0 = dpp_u32<0x00>(pk), a1 = dpp_u32<0x55>(pk), a2 = dpp_u32<0xAA>(pk), a3 = dpp_u32<0xFF>(pk);
      const int pc = 64 * i + l;
      if (store && (l & 3) == 0 && pc < F::PCS)
        *reinterpret_cast<int4*>(x8 + r * D + 4 * pc) = make_int4((int)a0, (int)a1, (int)a2, (int)a3);
    }
    b2 = wave_sum_f64(b2);  // exact (integers < 2^25)
    s2 = wave_sum_f64(s2);
    ex = fmax(ex, sc * sqrt(b2) * (1.0 + 1e-12));
    es = fmax(es, sqrt(s2) * (1.0 + 1e-12) + 1e-300);
    if (store && l == 0) inv_scale[r] = live ? inv : 1.0;
  }
  if (l == 0) {
    sb[0][w] = ex;
    sb[1][w] = es;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double* v = sb[threadIdx.x];
    const double m = fmax(fmax(v[0], v[1]), fmax(v[2], v[3]));
    atomicMax(bounds + threadIdx.x, (unsigned long long)__double_as_longlong(m));
  }
}

// ---------------------------------------------------------------------------------------------
// query prep: k5md_prep_kernel's piece (natural dim order), alpha = 1 / S, beta = 0, and the float Delta of
// the header from the corpus bounds
__global__ __launch_bounds__(256) void k5mf_prep_kernel(const float* __restrict__ qf, int nq, int nq_pad, int dim,
                                                        int8_t* __restrict__ qa, double* __restrict__ delta,
                                                        double* __restrict__ alpha, double* __restrict__ beta,
                                                        const double* __restrict__ bounds) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), l = lane_id();
  if (q >= nq_pad) return;
  int8_t* o = qa + (int64_t)q * dim;
  if (q >= nq) {  // padding queries: zero pieces (their thresholds never accept)
    for (int i = l; i < dim; i += WAVE) o[i] = 0;
    if (l == 0) {
      delta[q] = 0.0;
      alpha[q] = 0.0;
      beta[q] = 0.0;
    }
    return;
  }
  const float* qv = qf + (int64_t)q * dim;
  float mx = 0.f;
  for (int i = l; i < dim; i += WAVE) mx = fmaxf(mx, fabsf(qv[i]));
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, WAVE));
  const double invS = mx > 0.f ? 127.0 / (double)mx : 1.0;
  double r2 = 0.0, q2 = 0.0;
  for (int i = l; i < dim; i += WAVE) {
    const double x = (double)qv[i] * invS;
    double a = rint(x);  // |a| <= 127
    a = a > 127.0 ? 127.0 : (a < -127.0 ? -127.0 : a);
    const double rho = x - a;  // exact, |rho| <= 1/2
    r2 += rho * rho;
    q2 += (double)qv[i] * (double)qv[i];
    o[i] = (int8_t)a;
  }
  r2 = wave_sum_f64(r2);
  q2 = wave_sum_f64(q2);
  constexpr double SLACK = 1.0 / (1 << 20);  // the header's sum of roundings, < 2^-20
  if (l == 0) {
    const double qn = sqrt(q2) * invS, rn = sqrt(r2), b0 = bounds[0], b1 = bounds[1];
    delta[q] = (rn * b0 + qn * b1) * (1.0 + SLACK) + SLACK * (qn + rn) * b0;
    alpha[q] = invS;
    beta[q] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------
// K5mf's score: float rows by flat_score_dim, the query slice in registers, R rows per wave and round.
template <int KS>
struct FloatIP {
  const float* xf;
  static constexpr int OCC = FShape<KS>::OCC;
  struct Lds {};
  template <class Sh>
  __device__ __forceinline__ FSlice<KS> query(const float* __restrict__ qf, int q, Sh&) const {
    FSlice<KS> qs;
    fslice_load(qs, qf + (int64_t)q * FShape<KS>::D);
    return qs;
  }
  // The candidates of a batch are dealt to the waves in groups of R (row_at: per lane).
  template <class RowAt, class Admit>
  __device__ __forceinline__ void score_batch(const FSlice<KS>& qs, int64_t base, int64_t end, int64_t count,
                                              RowAt row_at, Admit admit) const {
    constexpr int D = FShape<KS>::D, R = FShape<KS>::R;
    const int l = lane_id(), w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // lane j < R: the row of candidate c0 + j (past the end: the last candidate again, so every address is a
    // row of the corpus; such a row is masked at admission)
    auto resolve = [&](int64_t c0) {
      uint32_t rv = 0;
      if (l < R) {
        const int64_t c = c0 + l;
        rv = row_at(c < count ? c : count - 1);
      }
      return rv;
    };
    const int nrounds = (int)((end - base + FIN_NW * R - 1) / (FIN_NW * R));
    int64_t c0 = base + (int64_t)w * R;
    uint32_t rv = resolve(c0);
    for (int t = 0; t < nrounds; ++t) {
      FSlice<KS> x[R];
      uint32_t rr[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        rr[j] = (uint32_t)__builtin_amdgcn_readlane((int)rv, j);
        fslice_load(x[j], xf + (int64_t)rr[j] * D);
      }
      const int64_t cn = c0 + FIN_NW * R;
      rv = resolve(cn);  // the next round's rows, resolved while this round's are in flight
      VRQ_SCHED_FENCE();
#pragma unroll
      for (int j = 0; j < R; ++j) admit(c0 + j < end && l == 0, desc_key_f64(flat_score_dim(qs, x[j])), rr[j]);
      c0 = cn;
    }
  }
};

// the operands of a K5mf call: the float rows for the finish, flat_ip_prepare's image of them for the passes
struct FloatOperands {
  const float* xf;
  const int8_t* x8;
  const double *inv_scale, *bounds;
  template <class... A>
  void prep(dim3 grid, hipStream_t s, A... a) const {
    hipLaunchKernelGGL(k5mf_prep_kernel, grid, dim3(256), 0, s, a..., bounds);
  }
  template <int KS, bool DENSE, class... A>
  void pass(dim3 grid, dim3 blk, hipStream_t s, A... a) const {
    hipLaunchKernelGGL((k5md_pass_kernel<KS, DENSE>), grid, blk, 0, s, x8, inv_scale, a...);
  }
  template <int KS>
  FloatIP<KS> family() const {
    return {xf};
  }
};

template <int KS>
static void launch_prepare(const float* xf, int64_t n, int8_t* x8, double* inv_scale, double* bounds, hipStream_t s) {
  const int64_t per = 4 * FShape<KS>::RPW;
  hipLaunchKernelGGL((k5mf_prepare_kernel<KS>), dim3((unsigned)((n + per - 1) / per)), dim3(256), 0, s, xf, n, x8,
                     inv_scale, reinterpret_cast<unsigned long long*>(bounds));
}

// "auto" of the float path, K5md's rule: per dim the smallest measured batch (nq = 1, 8, 64, 1024;
// profiles/flat_mfma_bench.jsonl) at which K5mf's slowest call beat K5d's fastest on the same rows, never
// nq = 1; 0 = no such batch measured, the dim stays on K5d
__host__ inline int min_batch_float(int dim) {
  switch (dim) {
    case 256: case 384: case 512: case 768: return 8;  // 1.19x-2.23x at nq = 8, 0.51x-0.78x at nq = 1
    case 1536: case 2048: return 64;                   // 0.52x / 0.41x at nq = 8, 3.3x / 2.3x at nq = 64
    default: return 0;
  }
}

// =============================================================================================
// K5mb: exhaustive binary (Phase-II) top-k, s = float64(q . (2 unpackbits(code) - 1)), on the matrix cores at
// the same six dims, behind vrq_binary_topk_dim_mfma.  K5's method for its binary mode: q/S = a + rho with
// one int8 piece a (S = max|q| / 127), u = <a, bits> against s' = (s + sum q) / (2S) = <q/S, bits>, so
// u - s' = -<rho, bits> lies in [-sum rho+, sum rho-] and Delta = max(sum rho+, sum rho-)(1 + eps) + eps ||q/S||_1.
// eps = 2^-20 holds up to d = 2048: u is an exact integer with |u| <= 127 * 2048 < 2^24, so the accumulators,
// the sample maxima (stored as f32) and the hit test (an integer compare) carry no rounding at all; what is
// left is the f64 rounding of s' = alpha s + beta and of the sums in prep, below 2^-40 ||q/S||_1.
// Select, the plan and the list layout are K5md's.
//
// The piece is stored with K5's k-permutation (ph2_pos) inside every 32-dim k-step, so the B fragment dword t
// of lane half h is (w >> (t + 4h)) & 0x01010101 of the little-endian code dword w of that k-step.
//
// Matrix pass (k5mb_pass_kernel<KS, DENSE>): K5md's work split per dim, A fragments of all of d in registers.
// The data path has no packed LDS ring and no LDS-DMA.  A 32-row packed tile is one contiguous run of 4 d
// bytes (128 KS); thread t of the workgroup loads its 16-byte piece t (and t + 64 W) straight into registers
// with one coalesced global_load_dwordx4, two tiles ahead of the MFMAs that consume it (a thread past the
// last piece loads the last piece again and writes nothing, so every wave issues the same number of loads and
// the wait before a tile's expansion is a counted one: the loads of the tile after it stay in flight).
// Piece p holds code dwords 4c .. 4c + 3 (k-steps 4c .. 4c + 3) of tile row rr, rr = p / (KS / 4),
// c = p % (KS / 4).  During tile t's MFMAs its lane expands them into the 8 fragments (4 k-steps x both lane
// halves) of tile t + 1 and writes each with one ds_write_b128 into the unpacked image
// [k-step][lane half * 32 + row][16 B] of a ring of 2 (32 d bytes per slot), one fragment per k-step.  The
// image is read back linearly (lane l reads 16 B at k-step * 1024 + 16 l), conflict-free at every dim.
// LDS at 2048: 2 x 64 KiB of ring + 16 KiB of hit stage.
//
// Thresholded pass: a tile's accumulators start at -ceil(thr) of their query (the first MFMA's C operand),
// clamped to +-2^30 for infinite or huge thresholds; a hit is acc >= 0.  Tile t-1's accumulators fold into one
// running integer max in tile t's MFMA shadow, and tile t-1's hit bits are re-derived from the still-live
// accumulators at the start of tile t+1 only when that max is non-negative.  Hits take K5md's per-wave LDS
// stage and lists.  The dense pass keeps the running integer max of u per (query, sample chunk, lane row).
//
// Finish and exact scan: one workgroup per query builds the query's nibble table (d / 4 nibbles x 16 f64) in
// LDS and scores one candidate row per THREAD with d / 4 lookups in nibble order (binary_score_dim, the one
// summation order of this path; phase2_nibbles' arithmetic at a run-time dim).
constexpr int BAB = 3;  // B fragments read BAB k-steps ahead into the ring of NR
static_assert(BAB < NR, "B ring");

template <int KS>
struct BShape {
  static constexpr int W = Shape<KS>::W, NT = W * 64;
  static constexpr int RB = 4 * KS;               // code bytes per row
  static constexpr int PPR = KS / 4;              // 16-byte pieces per row
  static constexpr int NPC = GRT * PPR;           // pieces per tile
  static constexpr int PL = (NPC + NT - 1) / NT;  // loads per lane and tile
  static constexpr int NF = 8 * PL;               // fragments a lane expands per tile, one per k-step
  static constexpr int UT = KS * 1024;            // unpacked tile: [k-step][lane][16 B]
  static_assert(KS % 4 == 0 && NF <= KS, "a piece stays inside a row; one fragment per k-step");
};

// prep: one wave per (padded) query, run-time dim.  qa[q] = the int8 piece in ph2_pos order inside every
// k-step; delta[q] = Delta_q; alpha = 1 / (2S), beta = sum q / (2S) (s' = alpha s + beta in u units).
__global__ __launch_bounds__(256) void k5mb_prep_kernel(const float* __restrict__ qf, int nq, int nq_pad, int dim,
                                                        int8_t* __restrict__ qa, double* __restrict__ delta,
                                                        double* __restrict__ alpha, double* __restrict__ beta) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), l = lane_id();
  if (q >= nq_pad) return;
  int8_t* o = qa + (int64_t)q * dim;
  if (q >= nq) {  // padding queries: zero pieces (their thresholds never accept)
    for (int i = l; i < dim; i += WAVE) o[i] = 0;
    if (l == 0) {
      delta[q] = 0.0;
      alpha[q] = 0.0;
      beta[q] = 0.0;
    }
    return;
  }
  const float* qv = qf + (int64_t)q * dim;
  float mx = 0.f;
  for (int i = l; i < dim; i += WAVE) mx = fmaxf(mx, fabsf(qv[i]));
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, WAVE));
  const double invS = mx > 0.f ? 127.0 / (double)mx : 1.0;  // an all-zero query: S = 1
  double rp = 0.0, rn = 0.0, q1 = 0.0, qs = 0.0;
  for (int i = l; i < dim; i += WAVE) {
    const double x = (double)qv[i] * invS;
    double a = rint(x);  // |a| <= 127
    a = a > 127.0 ? 127.0 : (a < -127.0 ? -127.0 : a);
    const double rho = x - a;  // exact, |rho| <= 1/2
    rp += rho > 0.0 ? rho : 0.0;
    rn += rho < 0.0 ? -rho : 0.0;
    q1 += fabs((double)qv[i]);
    qs += (double)qv[i];
    o[(i & ~31) + ph2_pos(i & 31)] = (int8_t)a;
  }
  rp = wave_sum_f64(rp);
  rn = wave_sum_f64(rn);
  q1 = wave_sum_f64(q1);
  qs = wave_sum_f64(qs);
  constexpr double SLACK = 1.0 / (1 << 20);
  if (l == 0) {
    delta[q] = fmax(rp, rn) * (1.0 + SLACK) + SLACK * q1 * invS;
    alpha[q] = 0.5 * invS;
    beta[q] = 0.5 * invS * qs;
  }
}

// The matrix pass.  DENSE = the sample pass (max of u over each lane row's rows of the chunk ->
// dv[q][chunk * 32 + lane row]) else the thresholded pass (u >= ceil(thr[q]) -> candidate lists); chunks,
// query blocks and qbflag as k5md_pass_kernel.
//
// G... is empty, or one `const uint32_t* rows` (K5gb, the gathered pass behind vrq_binary_topk_gather): the pass
// runs in virtual row space as K5g's does (n = the length of the list; chunks, tiles, the shifted last tile, the
// clamp of a short chunk and the staged hits are virtual rows v), and only the piece loads go through the list:
// piece i of a thread reads 16 bytes at codes + rows[v_i] * RB + 16 c_i, v_i = the virtual row of its tile row.
// A thread loads the list entry of each of its own pieces, PL four-byte loads per tile from the tile's one or
// two cache lines of the list; no cross-lane distribution, no LDS.  A piece load needs its entry in a register,
// so the entries run one tile ahead of the pieces, three ahead of the MFMAs: at the top of tile t the entries of
// tile t + 3 are requested FIRST, then the pieces of tile t + 2 go out with the entries requested in tile t - 1.
// In that order the entries a piece load waits for are older than everything that has to stay in flight (the
// pieces of tile t + 1 and the newest entries), so every wait stays a counted one: per tile, with PL = 2,
//   vmcnt(5), vmcnt(4)  entry 0 / 1 of tile t + 2 landed   (pieces of t + 1 and entries of t + 3 in flight)
//   vmcnt(5), vmcnt(4)  piece 0 / 1 of tile t + 1 landed   (entries of t + 3 and pieces of t + 2 in flight)
// against vmcnt(3), vmcnt(2) of the contiguous instance; with PL = 1 both are vmcnt(2) against vmcnt(1).  Past
// the last tile the index clamps to the last tile, so every address formed is a list entry and every wave
// issues the same number of loads.  The loads are plain C++ loads: the compiler counts the waits itself.
template <int KS, bool DENSE, class... G>
__global__ __launch_bounds__(Shape<KS>::W * 64, 1) void k5mb_pass_kernel(
    const uint8_t* __restrict__ codes, int64_t n, const int8_t* __restrict__ qa, int nq,
    const float* __restrict__ thr, uint32_t* __restrict__ cand, int32_t* __restrict__ ccnt, int capc,
    int64_t chunk_rows, int64_t chunk_stride, int nchunks, int nqb, float* __restrict__ dv, int64_t dv_stride,
    const int32_t* __restrict__ qbflag, G... gather) {
  using S = Shape<KS>;
  using B = BShape<KS>;
  constexpr bool GATHER = sizeof...(G) != 0;
  static_assert(sizeof...(G) <= 1, "one row list");
  constexpr int D = S::D, W = S::W, MB = S::MB, QW = S::QW, NE = S::NE, TPS = S::TPS, EOFF = S::EOFF;
  constexpr int RB = B::RB, PPR = B::PPR, NPC = B::NPC, PL = B::PL, NF = B::NF, UT = B::UT;
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * UT];
  // per-(query, this chunk) list lengths (one row per wave), then each wave's hit stage
  __shared__ int32_t lcnt[W * QW + (DENSE ? 0 : W * STG)];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l = lane_id(), r = l & 31, h = l >> 5;
  const int L = xcd_logical(blockIdx.x, gridDim.x);
  const int chunk = L / nqb, qb = L - chunk * nqb;
  if (chunk >= nchunks) return;
  if (qbflag && qbflag[qb] == 0) return;
  const int64_t row0 = (int64_t)chunk * chunk_stride;
  const int64_t row1 = (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  if (row0 >= row1) return;
  const int nrows = (int)(row1 - row0);
  const int ntiles = (nrows + GRT - 1) / GRT;
  const uint32_t sm0 = lds_addr(smem);

  // tile t covers chunk rows [tstart(t), tstart(t) + 32): the last tile of a ragged chunk is shifted back
  const bool tiny = nrows < GRT;
  auto tstart = [&](int t) { return tiny ? 0 : (t * GRT < nrows - GRT ? t * GRT : nrows - GRT); };
  auto lane_valid = [&](int t) { return tiny ? r < nrows : r >= t * GRT - tstart(t); };

  // this thread's pieces: global byte offset inside the tile (rows of a chunk shorter than 32 clamped, so every
  // load is in bounds) and the LDS byte offset of its first fragment in the unpacked image
  uint32_t goff[PL], uoff[PL];
  bool pv[PL];
  int grl[GATHER ? PL : 1];
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const int p = (int)threadIdx.x + B::NT * i, pc = p < NPC ? p : NPC - 1;
    const int rr = pc / PPR, c = pc % PPR, rl = tiny && rr > nrows - 1 ? nrows - 1 : rr;
    pv[i] = p < NPC;
    goff[i] = (uint32_t)(rl * RB + 16 * c);
    uoff[i] = (uint32_t)((4 * c * 64 + rr) * 16);
    if constexpr (GATHER) {  // the list supplies the row: tile row and byte in the row apart
      grl[i] = rl;
      goff[i] = (uint32_t)(16 * c);
    }
  }
  v4i pk[2][PL];  // the packed pieces of the tile being expanded / the tile after it
  auto load_tile = [&](int t, v4i (&dst)[PL]) {
    const uint8_t* base = codes + (row0 + tstart(t)) * RB;
#pragma unroll
    for (int i = 0; i < PL; ++i) dst[i] = *reinterpret_cast<const v4i*>(base + goff[i]);
  };
  // K5gb: ge[t & 1][i] = the list entry (physical row) of piece i of tile t, from its request until the piece
  // load that consumes it; tiles past the last are the last tile again
  const uint32_t* const rows = gather_rows(gather...);
  uint32_t ge[2][GATHER ? PL : 1];
  auto load_entries = [&](int t, uint32_t (&dst)[GATHER ? PL : 1]) {
    const uint32_t* base = rows + (row0 + tstart(t < ntiles ? t : ntiles - 1));
#pragma unroll
    for (int i = 0; i < PL; ++i) dst[GATHER ? i : 0] = base[grl[GATHER ? i : 0]];
  };
  auto load_gathered = [&](const uint32_t (&e)[GATHER ? PL : 1], v4i (&dst)[PL]) {
#pragma unroll
    for (int i = 0; i < PL; ++i)
      dst[i] = *reinterpret_cast<const v4i*>(codes + (int64_t)e[GATHER ? i : 0] * RB + goff[i]);
  };
  // fragment j = 8 i + 2 dw + hh of a tile: code dword dw of piece i, lane half hh
  auto expand = [&](auto J, const v4i (&src)[PL], uint32_t ub) {
    constexpr int j = decltype(J)::value, i = j >> 3, dw = (j >> 1) & 3, hh = j & 1;
    const uint32_t wd = (uint32_t)src[i][dw];
    v4i f;
    f.x = (int)((wd >> (4 * hh + 0)) & 0x01010101u);
    f.y = (int)((wd >> (4 * hh + 1)) & 0x01010101u);
    f.z = (int)((wd >> (4 * hh + 2)) & 0x01010101u);
    f.w = (int)((wd >> (4 * hh + 3)) & 0x01010101u);
    if (pv[i]) lds_write128_imm<dw * 1024 + hh * 512>(ub + uoff[i], f);
  };
  if constexpr (GATHER) {  // tile 0's and tile 1's entries (waited for here), their pieces, then tile 2's entries
    load_entries(0, ge[0]);
    load_entries(1, ge[1]);
    load_gathered(ge[0], pk[0]);
    load_gathered(ge[1], pk[1]);
    VRQ_SCHED_FENCE();
    load_entries(2, ge[0]);
  } else {
    load_tile(0, pk[0]);
    load_tile(ntiles > 1 ? 1 : 0, pk[1]);
  }

  // A fragments of this wave's M-blocks of 32 queries, every k-step -> accumulator file
  const int qbase = qb * S::QB + w * QW;
  v4i A[MB][KS];
#pragma unroll
  for (int j = 0; j < MB; ++j) {
    const int8_t* qp = qa + (int64_t)(qbase + 32 * j + r) * D + h * 16;
#pragma unroll
    for (int s = 0; s < KS; ++s) A[j][s] = *reinterpret_cast<const v4i*>(qp + s * 32);
  }
#pragma unroll
  for (int j = 0; j < MB; ++j)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+a"(A[j][s]));
  // test e of a lane: M-block e >> 4, accumulator register e & 15 -> query row of the wave
  auto qrow = [&](int e) { return 32 * (e >> 4) + ((e & 3) + 8 * ((e >> 2) & 3) + 4 * h); };
  v16i seed[MB] = {};  // thresholded pass: -ceil(thr) of each accumulator register's query
  if constexpr (!DENSE) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const float c = ceilf(thr[qbase + qrow(e)]);  // +-inf / huge thresholds: always / never a hit
      seed[e >> 4][e & 15] = c <= -1073741824.f ? 1073741824 : c >= 1073741824.f ? -1073741824 : -(int)c;
    }
  }

  const uint32_t lc0 = lds_addr(lcnt + w * QW);
  const uint32_t sg0 = lds_addr(lcnt + W * QW + (DENSE ? 0 : w * STG));  // this wave's hit stage
  int nst = 0;                                                         // staged entries (wave-uniform)
  if (!DENSE && l < QW) lcnt[w * QW + l] = 0;                          // visible after the first tile's barrier
  v16i acc[2][MB] = {};                                                // [tile parity][M-block]
  int imx[DENSE ? NE : 1];  // dense pass: running max of u per test (INT32_MIN: no row yet)
#pragma unroll
  for (int e = 0; e < (DENSE ? NE : 1); ++e) imx[e] = INT32_MIN;
  int imax = INT32_MIN;     // thresholded pass: max of the seeded accumulators of the tile being tested
  const int64_t qstride = (int64_t)nchunks * capc;

  auto to_list = [&](int ql, int cr) {  // as k5md_pass_kernel: a list past capc keeps counting (= overflow)
    int pos;
    lds_add_rtn32(pos, lc0 + (uint32_t)(ql * 4), 1);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pos)::"memory");
    if (pos < capc) cand[(int64_t)(qbase + ql) * qstride + (int64_t)chunk * capc + pos] = (uint32_t)(row0 + cr);
  };
  auto drain = [&]() {  // the staged entries -> lists (once per chunk, or when the stage is nearly full)
    for (int i0 = 0; i0 < nst; i0 += 64) {
      const int i = i0 + l;
      int e = 0;
      if (i < nst) lds_read32(e, sg0 + (uint32_t)(i * 4));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e)::"memory");
      if (i < nst) to_list((int)((uint32_t)e >> 26), e & 0x3ffffff);
    }
    nst = 0;
  };
  // the hits of tile tt, whose seeded accumulators are a: nothing to do unless the tile's max is non-negative
  auto flush = [&](int tt, const v16i (&a)[MB]) {
    const bool any = __ballot(imax >= 0) != 0;
    imax = INT32_MIN;
    if (!any) return;
    uint32_t m = 0;
    static_for<0, NE>([&](auto E) {
      constexpr int e = decltype(E)::value;
      m |= (a[e >> 4][e & 15] >= 0 ? 1u : 0u) << e;
    });
    if (!lane_valid(tt)) m = 0;
    if (__ballot(m != 0) == 0) return;
    const int lr = tstart(tt) + r;
    if (!__ballot((m & (m - 1)) != 0)) {
      // at most one hit per lane (the usual case): one staged entry per hit lane at its rank among them
      const uint64_t lanes = __ballot(m != 0);
      if (m) {
        int pos = nst + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(lanes >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lanes, 0));
        pos = pos < STG - 1 ? pos : STG - 1;  // (never binds: the stage drains above STG - 64)
        lds_write32(sg0 + (uint32_t)(pos * 4), (int)(((uint32_t)qrow(__builtin_ctz(m)) << 26) | (uint32_t)lr));
      }
      nst += __popcll(lanes);
      if (nst > STG - 64) drain();
    } else {
      for (int e = 0; e < NE; ++e)  // several hits in a lane: straight to the lists
        if ((m >> e) & 1u) to_list(qrow(e), lr);
    }
  };
  auto test = [&](const v16i (&a)[MB], int e, bool vp) {
    const int v = a[e >> 4][e & 15];
    if constexpr (DENSE)
      imx[e] = max(imx[e], vp ? v : INT32_MIN);
    else
      imax = max(imax, v);
  };

  // tile 0 -> slot 0 (tile t + 1 is expanded during tile t)
  static_for<0, NF>([&](auto J) { expand(J, pk[0], sm0); });

  auto tile = [&](auto PAR, auto FIRST, int t) {
    constexpr int p = decltype(PAR)::value;
    constexpr bool first = decltype(FIRST)::value;  // tile 0: no previous tile to test
    // every wave's fragments of tile t are written, and every wave is done reading the slot that tile t + 1's
    // fragments overwrite
    wait_lgkm0();
    barrier_all();
    if constexpr (!DENSE)
      if (t >= 2) flush(t - 2, acc[p]);  // (its accumulators are acc[p] until this tile's first MFMA)
    const bool vprev = lane_valid(t - 1);
    // pk[p] held tile t; pk[p ^ 1] holds tile t + 1
    if constexpr (GATHER) {
      load_entries(t + 3, ge[p ^ 1]);  // (ge[p ^ 1] held tile t + 1's, consumed in tile t - 1)
      VRQ_SCHED_FENCE();               // the request stays in front of the pieces: see the header
      load_gathered(ge[p], pk[p]);
    } else {
      load_tile(t + 2 < ntiles ? t + 2 : ntiles - 1, pk[p]);
    }
    const uint32_t badr = sm0 + (uint32_t)(p * UT + l * 16), ubn = sm0 + (uint32_t)((p ^ 1) * UT);
    v4i ring[NR];
    auto readB = [&](auto SS) {
      constexpr int s = decltype(SS)::value;
      lds_read128_off<s * 1024>(ring[s & (NR - 1)], badr);
    };
    static_for<0, BAB>([&](auto SS) { readB(SS); });
    VRQ_SCHED_FENCE();
    static_for<0, KS>([&](auto SS) {
      constexpr int s = decltype(SS)::value;
      if constexpr (s + BAB < KS) readB(std::integral_constant<int, s + BAB>{});
      // At most the B reads issued after B(s) stay outstanding.  A wave with a piece also has the fragment
      // writes of the k-steps in between in flight, which a wave without one never issues: the count holds
      // for both, and in the first it retires a read or two early (hence BAB = 3 reads ahead, not K5md's 2).
      asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(ring[s & (NR - 1)]) : "n"(s + BAB < KS ? BAB : KS - 1 - s) : "memory");
#pragma unroll
      for (int j = 0; j < MB; ++j)
        acc[p][j] = mfma_i8(A[j][s], ring[s & (NR - 1)], s == 0 ? seed[j] : acc[p][j]);
#pragma unroll
      for (int j = 0; j < MB; ++j) asm volatile("" : "+v"(acc[p][j]));
      if constexpr (s < NF) expand(SS, pk[p ^ 1], ubn);
      // tests / dense maxima of tile t-1
      if constexpr (!first && s >= EOFF && (s - EOFF) * TPS < NE) {
#pragma unroll
        for (int e = (s - EOFF) * TPS; e < (s - EOFF + 1) * TPS && e < NE; ++e) {
          test(acc[p ^ 1], e, vprev);
          // pin the test at this k-step (IR-level sinking would gather them behind the last MFMA)
          if constexpr (DENSE)
            asm volatile("" : "+v"(imx[e]));
          else
            asm volatile("" : "+v"(imax));
        }
      }
      VRQ_SCHED_FENCE();
    });
  };

  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using NOTFIRST = std::integral_constant<bool, false>;
  tile(I0{}, std::integral_constant<bool, true>{}, 0);
  int t = 1;
  for (; t + 1 < ntiles; t += 2) {
    tile(I1{}, NOTFIRST{}, t);
    tile(I0{}, NOTFIRST{}, t + 1);
  }
  if (t < ntiles) tile(I1{}, NOTFIRST{}, t);
  wait_lgkm0();
  // tile ntiles-2 (tested during the last tile), then the last tile itself
  const int pl = (ntiles - 1) & 1;
  if (!DENSE && ntiles >= 2) {
    if (pl)
      flush(ntiles - 2, acc[0]);
    else
      flush(ntiles - 2, acc[1]);
  }
  const bool vlast = lane_valid(ntiles - 1);
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    if (pl)
      test(acc[1], e, vlast);
    else
      test(acc[0], e, vlast);
  }
  if constexpr (DENSE) {  // the lane maxima of the chunk -> dv[q][chunk * 32 + r] (NaN: no row)
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int q = qbase + qrow(e);
      if (q < nq)
        dv[(int64_t)q * dv_stride + (int64_t)chunk * GRT + r] = imx[e] == INT32_MIN ? __builtin_nanf("") : (float)imx[e];
    }
  } else {
    if (pl)
      flush(ntiles - 1, acc[1]);
    else
      flush(ntiles - 1, acc[0]);
    drain();
    wait_lgkm0();
    if (l < QW && qbase + l < nq) ccnt[(int64_t)(qbase + l) * nchunks + chunk] = lcnt[w * QW + l];
  }
}

// ---------------------------------------------------------------------------------------------
// The binary score of one row for the query whose nibble table is tab (binary_table): tab[p * 16 + v] = the
// f64 sum over the 4 dims of nibble p (packbits MSB first) of (bit of v ? q : -q); the row's d / 4 table
// entries are added in nibble order.  One function for the finish and for the exact scan.
__device__ __forceinline__ void binary_table(const float* __restrict__ q, int dim, double* tab) {
  for (int e = threadIdx.x; e < dim * 4; e += blockDim.x) {
    const int p = e >> 4, v = e & 15;
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double x = (double)q[4 * p + b];
      t += ((v >> (3 - b)) & 1) ? x : -x;
    }
    tab[e] = t;
  }
}
__device__ __forceinline__ double binary_score_dim(const double* tab, const uint8_t* __restrict__ code_row, int dim) {
  const uint4* src = reinterpret_cast<const uint4*>(code_row);
  double s = 0.0;
  for (int i = 0; i < dim / 128; ++i) {
    const uint4 cw = src[i];
    const uint32_t wd[4] = {cw.x, cw.y, cw.z, cw.w};
    const double* t = tab + i * 512;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) {  // byte 16 i + 4 k + c: nibbles 2 b, 2 b + 1
        const uint32_t byte = (wd[k] >> (8 * c)) & 0xffu;
        s += t[(4 * k + c) * 32 + (byte >> 4)];
        s += t[(4 * k + c) * 32 + 16 + (byte & 15)];
      }
  }
  return s;
}

// K5mb's score: code rows by binary_score_dim, the query's nibble table in LDS, one row per thread.
struct Binary {
  const uint8_t* codes;
  int dim;
  static constexpr int OCC = 1;
  struct Lds {
    double tab[2048 * 4];
  };
  template <class Sh>
  __device__ __forceinline__ const double* query(const float* __restrict__ qf, int q, Sh& sh) const {
    binary_table(qf + (int64_t)q * dim, dim, sh.tab);
    return sh.tab;
  }
  template <class RowAt, class Admit>
  __device__ __forceinline__ void score_batch(const double* tab, int64_t base, int64_t end, int64_t, RowAt row_at,
                                              Admit admit) const {
    for (int64_t j = base + threadIdx.x; j < end; j += FIN_NT) {
      const uint32_t rr = row_at(j);
      admit(true, desc_key_f64(binary_score_dim(tab, codes + (int64_t)rr * (dim / 8), dim)), rr);
    }
  }
  template <class... A>
  void prep(dim3 grid, hipStream_t s, A... a) const {
    hipLaunchKernelGGL(k5mb_prep_kernel, grid, dim3(256), 0, s, a...);
  }
  template <int KS, bool DENSE, class... A>
  void pass(dim3 grid, dim3 blk, hipStream_t s, A... a) const {
    hipLaunchKernelGGL((k5mb_pass_kernel<KS, DENSE>), grid, blk, 0, s, codes, a...);
  }
  template <int KS>
  Binary family() const {
    return *this;
  }
};

// =============================================================================================
// The host driver of the three paths.  F = Int8Cos, FloatOperands or Binary supplies the prep-kernel launch,
// the pass-kernel launch and the finish family; the plan, the workspace, the stage flags and the sequence of
// launches are the same for all.
struct Call {
  int64_t n;  // rows the passes cover: the corpus's, or the length of `rows`
  const int8_t* qa;
  int nq;
  float* thr;
  uint32_t* cand;
  int32_t* cnt;
  float* dv;
  int32_t* qbf;
  hipStream_t s;
  const uint32_t* rows;  // K5g / K5gb: the allowed rows, ascending (NULL: every row)
};

template <int KS, class F>
static void launch_pass(const F& f, const Plan& p, const Call& c, int pass) {  // 0 sample, 1 main, 2 retry
  auto go = [&](auto... g) {
    const dim3 blk(Shape<KS>::W * 64);
    if (pass == 0)
      f.template pass<KS, true>(dim3(p.nsc * p.nqb), blk, c.s, c.n, c.qa, c.nq, (const float*)nullptr,
                                (uint32_t*)nullptr, (int32_t*)nullptr, 0, p.scr, p.sstride, p.nsc, p.nqb, c.dv,
                                p.scols, (const int32_t*)nullptr, g...);
    else
      f.template pass<KS, false>(dim3(p.nchunks * p.nqb), blk, c.s, c.n, c.qa, c.nq, (const float*)c.thr, c.cand,
                                 c.cnt, p.capc, p.chunk_rows, p.chunk_rows, p.nchunks, p.nqb, (float*)nullptr,
                                 (int64_t)0, pass == 2 ? (const int32_t*)c.qbf : (const int32_t*)nullptr, g...);
  };
  if (c.rows)
    go(c.rows);
  else if constexpr (KS != 32)  // (no contiguous KS = 32 instance: with_ks refuses the call)
    go();
}

template <class F>
static int launch_pass_dim(const F& f, int dim, const Plan& p, const Call& c, int pass) {
  const int rc = with_ks(dim, c.rows != nullptr, [&](auto KS) {
    launch_pass<decltype(KS)::value>(f, p, c, pass);
    return VRQ_OK;
  });
  if (rc != VRQ_OK) return rc;
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// rows != NULL (K5g, K5gb): n is the length of the list, and the call plans like an unfiltered one on n rows
template <class F>
static int run(const F& f, int64_t n, int dim, int64_t row_offset, const float* qf, int nq, int k, int flags,
               int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace, size_t workspace_bytes,
               hipStream_t s, const uint32_t* rows = nullptr) {
  Plan p;
  const int rc = plan_shape(n, dim, nq, k, &p, rows != nullptr);
  if (rc != VRQ_OK) return rc;
  if (workspace_bytes < p.bytes) return VRQ_EWORKSPACE;
  constexpr int ALL = VRQ_GEMM_STAGE_SAMPLE | VRQ_GEMM_STAGE_MAIN | VRQ_GEMM_STAGE_FINISH;
  const int st = (flags & ALL) ? (flags & ALL) : ALL;
  uint8_t* ws = (uint8_t*)workspace;
  int8_t* qa = (int8_t*)ws;
  double* delta = (double*)(ws + p.off_delta);
  double* alpha = (double*)(ws + p.off_alpha);
  double* beta = (double*)(ws + p.off_beta);
  int32_t* flag = (int32_t*)(ws + p.off_flag);
  const Call c{n, qa, nq, (float*)(ws + p.off_thr), (uint32_t*)(ws + p.off_cand), (int32_t*)(ws + p.off_cnt),
               (float*)(ws + p.off_dv), (int32_t*)(ws + p.off_qbf), s, rows};
  if (st & VRQ_GEMM_STAGE_SAMPLE) {
    f.prep(dim3((p.nq_pad + 3) / 4), s, qf, nq, p.nq_pad, dim, qa, delta, alpha, beta);
    VRQ_LAUNCH_CHECK();
    const int r0 = launch_pass_dim(f, dim, p, c, 0);
    if (r0 != VRQ_OK) return r0;
    hipLaunchKernelGGL(k5md_select_kernel, dim3(p.nq_pad), dim3(256), 0, s, (const float*)c.dv, p.scols, p.sstride,
                       p.nsc, n, k, (const double*)delta, c.thr, c.cnt, p.nchunks, nq, c.qbf, p.nqb);
    VRQ_LAUNCH_CHECK();
  }
  if (st & VRQ_GEMM_STAGE_MAIN) {
    const int r1 = launch_pass_dim(f, dim, p, c, 1);
    if (r1 != VRQ_OK) return r1;
  }
  if (st & VRQ_GEMM_STAGE_FINISH) {
    // finish -> retry main pass (query blocks with a retried query) -> finish of the retried queries ->
    // exact scan of the rest
    const bool skip = (flags & VRQ_GEMM_NO_FALLBACK) != 0;
    return with_ks(dim, rows != nullptr, [&](auto KS) {
      const auto fam = f.template family<decltype(KS)::value>();
      using Fam = std::remove_const_t<decltype(fam)>;
      auto stage = [&](auto... g) {
        auto finish = [&](auto RETRY) {
          hipLaunchKernelGGL((k5m_finish_kernel<Fam, decltype(RETRY)::value, decltype(g)...>), dim3(nq), dim3(FIN_NT),
                             0, s, fam, n, row_offset, qf, k, (const uint32_t*)c.cand, (const int32_t*)c.cnt,
                             p.nchunks, p.capc, p.qpb, out_count, out_rows, out_scores, flag, c.thr,
                             (const double*)alpha, (const double*)beta, (const double*)delta, c.qbf, g...);
        };
        finish(std::false_type{});
        VRQ_LAUNCH_CHECK();
        const int r2 = launch_pass_dim(f, dim, p, c, 2);
        if (r2 != VRQ_OK) return r2;
        finish(std::true_type{});
        VRQ_LAUNCH_CHECK();
        hipLaunchKernelGGL((k5m_fallback_kernel<Fam, decltype(g)...>), dim3(nq), dim3(FIN_NT), 0, s, fam, n,
                           row_offset, qf, k, out_count, out_rows, out_scores, (const int32_t*)flag, skip, g...);
        VRQ_LAUNCH_CHECK();
        return (int)VRQ_OK;
      };
      if (rows) return stage(rows);
      if constexpr (decltype(KS)::value != 32) return stage();
      return (int)VRQ_EUNSUPPORTED;
    });
  }
  return VRQ_OK;
}

// "auto" of the binary path, K5md's rule: per dim the smallest measured batch (nq = 1, 8, 64, 1024;
// profiles/binary_mfma_bench.jsonl) at which K5mb's slowest call beat K5d's fastest on the same codes;
// 0 = no such batch measured, the dim stays on K5d
__host__ inline int min_batch_binary(int dim) {
  switch (dim) {
    case 256: case 384: case 512: case 768: case 1536: case 2048:
      return 8;  // 3.1x-8.7x at nq = 8, 0.51x-0.77x at nq = 1
    default: return 0;
  }
}

// =============================================================================================
// K5g host side: the *_rows calls.  An empty list launches this alone.
__global__ __launch_bounds__(256) void k5g_empty_kernel(int nq, int k, int32_t* __restrict__ out_count,
                                                        int64_t* __restrict__ out_rows,
                                                        double* __restrict__ out_scores) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)nq * k) {
    out_rows[i] = -1;
    out_scores[i] = __builtin_nan("");
  }
  if (i < nq) out_count[i] = 0;
}

static int run_empty(int nq, int k, int32_t* out_count, int64_t* out_rows, double* out_scores, hipStream_t s) {
  const int64_t cells = (int64_t)nq * (k > 1 ? k : 1);
  hipLaunchKernelGGL(k5g_empty_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, nq, k, out_count,
                     out_rows, out_scores);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

// the plan of a gathered call over a list of m rows: plan_shape(m), an empty list planned as one row
__host__ inline int plan_rows(int64_t m, int dim, int nq, int k, Plan* p) {
  if (m < 0) return VRQ_EINVAL;
  return plan_shape(m > 0 ? m : 1, dim, nq, k, p, true);
}

// the bodies of the *_plan and *_prep_layout entries: rc = the plan's return code, passed through
static int plan_info(int rc, const Plan& p, int64_t* info) {
  if (rc != VRQ_OK) return rc;
  info[0] = p.chunk_rows;
  info[1] = p.nchunks;
  info[2] = p.capc;
  info[3] = p.nqb;
  info[4] = p.nsc;
  info[5] = p.scr;
  info[6] = (int64_t)p.bytes;
  info[7] = p.qpb;
  return VRQ_OK;
}

static int prep_layout_info(int rc, const Plan& p, int64_t* info) {
  if (rc != VRQ_OK) return rc;
  info[0] = (int64_t)p.off_delta;
  info[1] = (int64_t)p.off_alpha;
  info[2] = (int64_t)p.off_beta;
  info[3] = (int64_t)p.off_flag;
  info[4] = (int64_t)p.off_thr;
  info[5] = p.nq_pad;
  info[6] = (int64_t)p.off_cnt;
  info[7] = (int64_t)p.off_cand;
  return VRQ_OK;
}

constexpr int ROWS_FLAGS = VRQ_GEMM_STAGE_SAMPLE | VRQ_GEMM_STAGE_MAIN | VRQ_GEMM_STAGE_FINISH | VRQ_GEMM_NO_FALLBACK;

}  // namespace g5d
}  // namespace vrq

using namespace vrq;

extern "C" {

size_t vrq_gemm_topk_dim_mfma_workspace_size(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k) {
  if (mode != VRQ_GEMM_INT8_COSINE) return 0;  // (at 1024 too: the entry point serves no other mode)
  if (dim == 1024) return vrq_gemm_topk_workspace_size(mode, n, dim, nq, k);
  g5d::Plan p;
  return g5d::plan(mode, n, dim, nq, k, &p) == VRQ_OK ? p.bytes : 0;
}

int vrq_gemm_topk_dim_mfma_plan(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  if (mode != VRQ_GEMM_INT8_COSINE) return mode == VRQ_GEMM_FLOAT_IP ? VRQ_EINVAL : VRQ_EUNSUPPORTED;
  if (dim == 1024) return vrq_gemm_topk_plan(mode, n, dim, nq, k, info);
  g5d::Plan p;
  return g5d::plan_info(g5d::plan(mode, n, dim, nq, k, &p), p, info);
}

int vrq_gemm_topk_dim_mfma_prep_layout(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  if (dim == 1024) return VRQ_EUNSUPPORTED;  // K5's: vrq_gemm_topk_prep_layout / vrq_gemm_topk_layout
  g5d::Plan p;
  return g5d::prep_layout_info(g5d::plan(mode, n, dim, nq, k, &p), p, info);
}

int vrq_gemm_topk_dim_mfma(int32_t mode, const uint8_t* codes, const int8_t* x8, const double* norms, int64_t n,
                           int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k, int32_t flags,
                           int32_t* out_count, int64_t* out_rows, double* out_scores, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (mode == VRQ_GEMM_BINARY) return VRQ_EUNSUPPORTED;  // needs its own bit-expansion path off 1024
  if (mode != VRQ_GEMM_INT8_COSINE) return VRQ_EINVAL;
  if (dim == 1024)
    return vrq_gemm_topk(mode, codes, x8, norms, n, dim, row_offset, qf, nq, k, flags, out_count, out_rows, out_scores,
                         workspace, workspace_bytes, stream);
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(qf && out_count && out_rows && out_scores && workspace && x8 && norms && n > 0 && nq > 0 && k > 0);
  constexpr int OK = VRQ_GEMM_STAGE_SAMPLE | VRQ_GEMM_STAGE_MAIN | VRQ_GEMM_STAGE_FINISH | VRQ_GEMM_NO_FALLBACK;
  if (flags & ~OK) return VRQ_EUNSUPPORTED;
  return g5d::run(g5d::Int8Cos{x8, norms, dim}, n, dim, row_offset, qf, nq, k, flags, out_count, out_rows, out_scores,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

int vrq_gemm_topk_dim_engine(int32_t mode, int64_t n, int32_t dim, int32_t nq, int32_t k) {
  g5d::Plan p;
  if (dim == 1024 || g5d::plan(mode, n, dim, nq, k, &p) != VRQ_OK) return VRQ_GEMM_ENGINE_EXACT;
  const int mb = g5d::min_batch(dim);
  return mb > 0 && nq >= mb ? VRQ_GEMM_ENGINE_MFMA : VRQ_GEMM_ENGINE_EXACT;
}

int vrq_flat_ip_prepare_dim(const float* xf, int64_t n, int32_t dim, int8_t* x8, double* inv_scale, double* bounds,
                            void* stream) {
  if (dim == 1024) return vrq_flat_ip_prepare(xf, n, dim, x8, inv_scale, bounds, stream);
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(n >= 0 && bounds);
  if (n == 0) return VRQ_OK;
  VRQ_CHECK_ARG(xf && x8 && inv_scale);
  const hipStream_t s = (hipStream_t)stream;
  const int rc = g5d::with_ks(dim, false, [&](auto KS) {
    if constexpr (decltype(KS)::value != 32)  // (1024 is vrq_flat_ip_prepare's, above)
      g5d::launch_prepare<decltype(KS)::value>(xf, n, x8, inv_scale, bounds, s);
    return VRQ_OK;
  });
  if (rc != VRQ_OK) return rc;
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

size_t vrq_flat_ip_topk_dim_mfma_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t k) {
  if (dim == 1024) return vrq_gemm_topk_workspace_size(VRQ_GEMM_FLOAT_IP, n, dim, nq, k);
  g5d::Plan p;
  return g5d::plan_shape(n, dim, nq, k, &p) == VRQ_OK ? p.bytes : 0;
}

int vrq_flat_ip_topk_dim_mfma_plan(int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  if (dim == 1024) return vrq_gemm_topk_plan(VRQ_GEMM_FLOAT_IP, n, dim, nq, k, info);
  g5d::Plan p;
  return g5d::plan_info(g5d::plan_shape(n, dim, nq, k, &p), p, info);
}

int vrq_flat_ip_topk_dim_mfma_prep_layout(int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  if (dim == 1024) return VRQ_EUNSUPPORTED;  // K5's: vrq_gemm_topk_prep_layout / vrq_gemm_topk_layout
  g5d::Plan p;
  return g5d::prep_layout_info(g5d::plan_shape(n, dim, nq, k, &p), p, info);
}

int vrq_flat_ip_topk_dim_mfma(const float* xf, const int8_t* x8, const double* inv_scale, const double* bounds,
                              int64_t n, int32_t dim, int64_t row_offset, const float* qf, int32_t nq, int32_t k,
                              int32_t flags, int32_t* out_count, int64_t* out_rows, double* out_scores,
                              void* workspace, size_t workspace_bytes, void* stream) {
  constexpr int OK = VRQ_GEMM_STAGE_SAMPLE | VRQ_GEMM_STAGE_MAIN | VRQ_GEMM_STAGE_FINISH | VRQ_GEMM_NO_FALLBACK;
  if (flags & ~OK) return VRQ_EUNSUPPORTED;
  if (dim == 1024)
    return vrq_flat_ip_topk(xf, x8, inv_scale, bounds, n, dim, row_offset, qf, nq, k, flags, out_count, out_rows,
                            out_scores, workspace, workspace_bytes, stream);
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(xf && x8 && inv_scale && bounds && qf && out_count && out_rows && out_scores && workspace && n > 0 &&
                nq > 0 && k > 0);
  return g5d::run(g5d::FloatOperands{xf, x8, inv_scale, bounds}, n, dim, row_offset, qf, nq, k, flags, out_count,
                  out_rows, out_scores, workspace, workspace_bytes, (hipStream_t)stream);
}

int vrq_flat_ip_dim_engine(int64_t n, int32_t dim, int32_t nq, int32_t k) {
  g5d::Plan p;
  if (dim == 1024 || g5d::plan_shape(n, dim, nq, k, &p) != VRQ_OK) return VRQ_GEMM_ENGINE_EXACT;
  const int mb = g5d::min_batch_float(dim);
  return mb > 0 && nq > 1 && nq >= mb ? VRQ_GEMM_ENGINE_MFMA : VRQ_GEMM_ENGINE_EXACT;
}

size_t vrq_binary_topk_dim_mfma_workspace_size(int64_t n, int32_t dim, int32_t nq, int32_t k) {
  if (dim == 1024) return vrq_gemm_topk_workspace_size(VRQ_GEMM_BINARY, n, dim, nq, k);
  g5d::Plan p;
  return g5d::plan_shape(n, dim, nq, k, &p) == VRQ_OK ? p.bytes : 0;
}

int vrq_binary_topk_dim_mfma_plan(int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  if (dim == 1024) return vrq_gemm_topk_plan(VRQ_GEMM_BINARY, n, dim, nq, k, info);
  g5d::Plan p;
  return g5d::plan_info(g5d::plan_shape(n, dim, nq, k, &p), p, info);
}

int vrq_binary_topk_dim_mfma_prep_layout(int64_t n, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  if (dim == 1024) return VRQ_EUNSUPPORTED;  // K5's: vrq_gemm_topk_prep_layout / vrq_gemm_topk_layout
  g5d::Plan p;
  return g5d::prep_layout_info(g5d::plan_shape(n, dim, nq, k, &p), p, info);
}

int vrq_binary_topk_dim_mfma(const uint8_t* codes, int64_t n, int32_t dim, int64_t row_offset, const float* qf,
                             int32_t nq, int32_t k, int32_t flags, int32_t* out_count, int64_t* out_rows,
                             double* out_scores, void* workspace, size_t workspace_bytes, void* stream) {
  constexpr int OK = VRQ_GEMM_STAGE_SAMPLE | VRQ_GEMM_STAGE_MAIN | VRQ_GEMM_STAGE_FINISH | VRQ_GEMM_NO_FALLBACK;
  if (flags & ~OK) return VRQ_EUNSUPPORTED;
  if (dim == 1024)
    return vrq_gemm_topk(VRQ_GEMM_BINARY, codes, nullptr, nullptr, n, dim, row_offset, qf, nq, k, flags, out_count,
                         out_rows, out_scores, workspace, workspace_bytes, stream);
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(codes && qf && out_count && out_rows && out_scores && workspace && n > 0 && nq > 0 && k > 0);
  return g5d::run(g5d::Binary{codes, dim}, n, dim, row_offset, qf, nq, k, flags, out_count, out_rows, out_scores,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

size_t vrq_gemm_topk_rows_workspace_size(int32_t mode, int64_t m, int32_t dim, int32_t nq, int32_t k) {
  g5d::Plan p;
  return mode == VRQ_GEMM_INT8_COSINE && g5d::plan_rows(m, dim, nq, k, &p) == VRQ_OK ? p.bytes : 0;
}

int vrq_gemm_topk_rows_plan(int32_t mode, int64_t m, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  if (mode != VRQ_GEMM_INT8_COSINE) return mode == VRQ_GEMM_FLOAT_IP ? VRQ_EINVAL : VRQ_EUNSUPPORTED;
  g5d::Plan p;
  return g5d::plan_info(g5d::plan_rows(m, dim, nq, k, &p), p, info);
}

int vrq_gemm_topk_rows(int32_t mode, const uint8_t* codes, const int8_t* x8, const double* norms, int64_t n,
                       int32_t dim, int64_t row_offset, const uint32_t* rows, int64_t m, const float* qf, int32_t nq,
                       int32_t k, int32_t flags, int32_t* out_count, int64_t* out_rows, double* out_scores,
                       void* workspace, size_t workspace_bytes, void* stream) {
  (void)codes;
  if (mode == VRQ_GEMM_BINARY) return VRQ_EUNSUPPORTED;  // K5mb's gather has its own entry: vrq_binary_topk_gather
  if (mode != VRQ_GEMM_INT8_COSINE) return VRQ_EINVAL;
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  if (flags & ~g5d::ROWS_FLAGS) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(qf && out_count && out_rows && out_scores && n > 0 && nq > 0 && k > 0 && m >= 0 && m <= n);
  if (m == 0) return g5d::run_empty(nq, k, out_count, out_rows, out_scores, (hipStream_t)stream);
  VRQ_CHECK_ARG(rows && workspace && x8 && norms);
  return g5d::run(g5d::Int8Cos{x8, norms, dim}, m, dim, row_offset, qf, nq, k, flags, out_count, out_rows, out_scores,
                  workspace, workspace_bytes, (hipStream_t)stream, rows);
}

size_t vrq_flat_ip_topk_rows_workspace_size(int64_t m, int32_t dim, int32_t nq, int32_t k) {
  g5d::Plan p;
  return g5d::plan_rows(m, dim, nq, k, &p) == VRQ_OK ? p.bytes : 0;
}

int vrq_flat_ip_topk_rows_plan(int64_t m, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  g5d::Plan p;
  return g5d::plan_info(g5d::plan_rows(m, dim, nq, k, &p), p, info);
}

int vrq_flat_ip_topk_rows(const float* xf, const int8_t* x8, const double* inv_scale, const double* bounds, int64_t n,
                          int32_t dim, int64_t row_offset, const uint32_t* rows, int64_t m, const float* qf,
                          int32_t nq, int32_t k, int32_t flags, int32_t* out_count, int64_t* out_rows,
                          double* out_scores, void* workspace, size_t workspace_bytes, void* stream) {
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  if (flags & ~g5d::ROWS_FLAGS) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(qf && out_count && out_rows && out_scores && n > 0 && nq > 0 && k > 0 && m >= 0 && m <= n);
  if (m == 0) return g5d::run_empty(nq, k, out_count, out_rows, out_scores, (hipStream_t)stream);
  VRQ_CHECK_ARG(rows && workspace && xf && x8 && inv_scale && bounds);
  return g5d::run(g5d::FloatOperands{xf, x8, inv_scale, bounds}, m, dim, row_offset, qf, nq, k, flags, out_count,
                  out_rows, out_scores, workspace, workspace_bytes, (hipStream_t)stream, rows);
}

size_t vrq_binary_topk_gather_workspace_size(int64_t m, int32_t dim, int32_t nq, int32_t k) {
  g5d::Plan p;
  return g5d::plan_rows(m, dim, nq, k, &p) == VRQ_OK ? p.bytes : 0;
}

int vrq_binary_topk_gather_plan(int64_t m, int32_t dim, int32_t nq, int32_t k, int64_t* info) {
  if (!info) return VRQ_EINVAL;
  g5d::Plan p;
  return g5d::plan_info(g5d::plan_rows(m, dim, nq, k, &p), p, info);
}

int vrq_binary_topk_gather(const uint8_t* codes, int64_t n, int32_t dim, int64_t row_offset, const uint32_t* rows,
                           int64_t m, const float* qf, int32_t nq, int32_t k, int32_t flags, int32_t* out_count,
                           int64_t* out_rows, double* out_scores, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (!vrq_dim_supported(dim)) return VRQ_EUNSUPPORTED;
  if (flags & ~g5d::ROWS_FLAGS) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(qf && out_count && out_rows && out_scores && n > 0 && nq > 0 && k > 0 && m >= 0 && m <= n);
  if (m == 0) return g5d::run_empty(nq, k, out_count, out_rows, out_scores, (hipStream_t)stream);
  VRQ_CHECK_ARG(rows && workspace && codes);
  return g5d::run(g5d::Binary{codes, dim}, m, dim, row_offset, qf, nq, k, flags, out_count, out_rows, out_scores,
                  workspace, workspace_bytes, (hipStream_t)stream, rows);
}

int vrq_binary_topk_dim_engine(int64_t n, int32_t dim, int32_t nq, int32_t k) {
  g5d::Plan p;
  if (dim == 1024 || g5d::plan_shape(n, dim, nq, k, &p) != VRQ_OK) return VRQ_GEMM_ENGINE_EXACT;
  const int mb = g5d::min_batch_binary(dim);
  return mb > 0 && nq >= mb ? VRQ_GEMM_ENGINE_MFMA : VRQ_GEMM_ENGINE_EXACT;
}

}  // extern "C"
