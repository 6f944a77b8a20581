// mfma_hits.h -- what the matrix-core Phase-I kernels of every code size share around their MFMA loops
// (hamming_mfma.hip: K1m, K1s, K1r; hamming_mfma_dim.hip: K1rd): the launch shape constants, the layout of
// a staged hit entry, the pass modes, the dense sample pass's lane minima and the row-split kernels' hit stage.
#pragma once

#include "mfma_common.h"

namespace vrq {

constexpr int MWAVES = 4;   // waves per workgroup (one per SIMD; the row-split kernels: one chunk per wave)
constexpr int RT = 64;      // rows per tile (2 n-blocks of 32)
constexpr int STG = 512;    // per-wave staged hit entries (u32)

// Staged hit entry (u32): (v + bias) << 14 | query-in-wave << 7 | row in the tile or n-block, where
// v = dist - tau(q) in [-bias, -1] (tau = the threshold the pass ran with; the suffix kernel adds it back)
// and bias = dim + 1 (1025 at 1024 bits).  List keys carry the same field: (v + bias) << 40 | row.
constexpr int ENT_V_SHIFT = 14, ENT_Q_SHIFT = 7;

// MODE of a pass: MFMA_MAIN (thresholded pass), MFMA_SAMPLE (dense sample pass) or MFMA_RERUN (the exact
// re-run of failed query blocks: same code as MAIN, a separate symbol so profiles and traces tell the two
// launches apart).
enum { MFMA_MAIN = 0, MFMA_SAMPLE = 1, MFMA_RERUN = 2 };

// The dense sample pass keeps, per lane and accumulator register, the minimum of v = dist - pc(q)
// over the sample rows of its chunk that the lane holds (lane row ri of every n-block): 32 values
// per (query, chunk), each the distance of a DISTINCT sample row, written once per chunk as u16
// (v + BIAS, BIAS = the code's bits; 0xFFFF: the lane saw no row) to dv[q][col], col = chunk * 32 + ri.
// The order statistics sample_select_kernel takes over these minima are >= those over every sample
// distance: tau_p (K-th + 1) still has K distinct rows below it, and tau_s only admits more rows (the
// recheck proves it per query either way).
// The minima are kept in float: v = pc(r) - 2 acc is one v_fma_f32 and the fold one v_min_f32 per
// register (exact: integers far below 2^24), a row past the chunk end contributes +inf.
template <bool ON, int MB, int BIAS>
struct DenseMin {  // the sample pass's lane minima (ON); empty in the thresholded passes
  float v[MB][16];
  __device__ __forceinline__ DenseMin() {
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int g = 0; g < 16; ++g) v[m][g] = __builtin_inff();
  }
  // v = pc(r) - 2 <q, r> of the 16 registers of M-block m (a row past the chunk end: no value)
  __device__ __forceinline__ void fold(const v16f& a, int m, int pc, bool ok) {
    const float pcf = ok ? (float)pc : __builtin_inff();
#pragma unroll
    for (int g = 0; g < 16; ++g) v[m][g] = fminf(v[m][g], fmaf(-2.0f, a[g], pcf));
  }
  // -> dv[q][col] as u16 (v + BIAS; 0xFFFF: no row), col = chunk * 32 + lane row
  __device__ __forceinline__ void out(uint16_t* __restrict__ dv, int64_t dv_stride, int64_t col, int qbase, int h,
                                      int nq) const {
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int q = qbase + 32 * m + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (q < nq)
          dv[(int64_t)q * dv_stride + col] = v[m][g] == __builtin_inff() ? (uint16_t)0xFFFF : (uint16_t)((int)v[m][g] + BIAS);
      }
  }
};
template <int MB, int BIAS>
struct DenseMin<false, MB, BIAS> {
  __device__ __forceinline__ void fold(const v16f&, int, int, bool) {}
  __device__ __forceinline__ void out(uint16_t*, int64_t, int64_t, int, int, int) const {}
};

// The hit stage of the row-split kernels (K1r, its lean form, K1rd): the candidates of a 32-row n-block are
// staged per wave in LDS and appended synchronously to the per-(query, chunk) lists (hits are rare at the
// sizes these kernels serve).  BIAS = dim + 1 is the key bias, QPW the wave's queries.
template <int BIAS, int QPW>
struct HitStage {
  uint32_t stg0, lc0;     // LDS addresses of the wave's stage (STG + 1 entries) and of its list lengths
  uint64_t* cbase;        // the wave's lists: query ql -> cbase + ql * qstride + pos
  int64_t qstride;
  int capc;
  int l;                  // lane id
  int nst = 0;            // staged entries (wave-uniform)

  // hits of M-block m of the n-block (acc > hp = pc(r) / 2): one ballot per register.  Positions past STG
  // land in a spare slot and the flush marks the whole wave's lists overflowed (exact rescan).
  __device__ __forceinline__ void block_hits(const v16f& a, int m, int pc, float hp) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const uint64_t mask = __ballot(a[g] > hp);
      if (mask) {
        if ((mask >> l) & 1) {
          const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
          int lo = l;  // lane-dependent values of this rare path from an opaque lane id (no hoisting)
          asm volatile("" : "+v"(lo));
          const int ql = 32 * m + (g & 3) + 8 * (g >> 2) + 4 * (lo >> 5);
          // acc = <q,r> + (tau(q) - pc(q)) / 2, so pc(r) - 2 acc = dist - tau(q) in [-BIAS, -1]
          const int v = pc - (int)(2.0f * a[g]);
          const int pos = nst + below < STG ? nst + below : STG;
          lds_write32(stg0 + (uint32_t)(pos * 4), ((v + BIAS) << ENT_V_SHIFT) | (ql << ENT_Q_SHIFT) | (lo & 31));
        }
        nst += __popcll(mask);
      }
    }
  }
  // staged hits -> lists; base_row: the n-block's first row
  __device__ __forceinline__ void flush_all(int64_t base_row) {
    if (nst > STG) {  // staging overflowed: every list of the wave -> exact rescan
      for (int i = l; i < QPW; i += 64) lds_add32(lc0 + (uint32_t)(i * 4), capc + 1);
      nst = STG;
    }
    for (int i0 = 0; i0 < nst; i0 += 64) {
      const int i = i0 + l;
      int e = 0, pos = 0;
      if (i < nst) lds_read32(e, stg0 + (uint32_t)(i * 4));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e)::"memory");
      const int ql = (e >> ENT_Q_SHIFT) & 127;
      if (i < nst) lds_add_rtn32(pos, lc0 + (uint32_t)(ql * 4), 1);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pos)::"memory");
      if (i < nst && pos < capc)
        cbase[(int64_t)ql * qstride + pos] =
            ((uint64_t)(uint32_t)(e >> ENT_V_SHIFT) << KEY_ROW_BITS) | (uint64_t)(base_row + (e & 127));
    }
    nst = 0;
  }
};

}  // namespace vrq
