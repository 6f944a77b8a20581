// dequant_dot.h -- the rescoring score of ONE stored row for one query, one wave per (query, row):
// float(np.dot(query_float, doc_emb)) of the two-phase searches (e.g. VectorDBInt8Global.py:232-241,
// CohereVectorDBBinary.py:228-232), shared by the stand-alone rescoring (dequant.hip) and the fused
// two-phase finish (select_rescore.hip) so both produce bit-identical scores.  doc_emb is the
// dequantised row of the mode (deq_row / deq_elem, the reference's _dequantize_* bit for bit), the f32
// row itself (VRQ_RESCORE_F32) or the +-1 row a packed sign code unpacks to (VRQ_RESCORE_SIGNED_BINARY).
#pragma once

#include "vrq_internal.h"

namespace vrq {

struct DeqRow {
  int mode;
  double limit;
  float sf;   // float32 scale (INT8/INT16 global, INT8 local)
  double sd;  // float64 scale (INT4 modes)
  bool zero;  // local modes with min == max
};

__device__ __forceinline__ DeqRow deq_row(int mode, double limit, const double* minmax, int64_t r) {
  DeqRow d{mode, limit, 0.f, 0.0, false};
  switch (mode) {
    case VRQ_RESCORE_F32: break;
    case VRQ_ENC_INT8_GLOBAL: d.sf = (float)(limit / 127.0); break;
    case VRQ_ENC_INT16_GLOBAL: d.sf = (float)(limit / 32767.0); break;
    case VRQ_ENC_INT4_GLOBAL: d.sd = limit / 7.0; break;
    case VRQ_ENC_INT8_LOCAL: {
      const float mn = (float)minmax[2 * r], mx = (float)minmax[2 * r + 1];
      d.zero = mn == mx;
      d.sf = __fdiv_rn(fmaxf(fabsf(mn), fabsf(mx)), 127.0f);  // np.float32 / int -> float32
      break;
    }
    default: {  // VRQ_ENC_INT4_LOCAL
      const double mn = minmax[2 * r], mx = minmax[2 * r + 1];
      d.zero = mn == mx;
      d.sd = fmax(fabs(mn), fabs(mx)) / 7.0;
      break;
    }
  }
  return d;
}

// element i of row r (q = the mode's code array)
__device__ __forceinline__ float deq_elem(const DeqRow& d, const void* q, int64_t r, int dim, int i) {
  if (d.zero) return 0.f;
  switch (d.mode) {
    case VRQ_RESCORE_F32:
      return reinterpret_cast<const float*>(q)[r * dim + i];
    case VRQ_ENC_INT8_GLOBAL:
    case VRQ_ENC_INT8_LOCAL:
      return __fmul_rn((float)reinterpret_cast<const int8_t*>(q)[r * dim + i], d.sf);
    case VRQ_ENC_INT16_GLOBAL:
      return __fmul_rn((float)reinterpret_cast<const int16_t*>(q)[r * dim + i], d.sf);
    default: {
      const uint8_t b = reinterpret_cast<const uint8_t*>(q)[r * ((dim + 1) / 2) + (i >> 1)];
      const int nib = (i & 1) ? (b & 15) : (b >> 4);
      return (float)__dmul_rn((double)(nib - 8), d.sd);
    }
  }
}

// this lane's part of the dot for a mode known at compile time (the switch of deq_elem folds away and the
// unrolled loop keeps several row loads in flight); elements l, l + 64, ... added in that order
template <int MODE>
__device__ __forceinline__ double deq_lane_sum(DeqRow d, const float* __restrict__ qrow, int dim,
                                               const void* __restrict__ q, int64_t r) {
  d.mode = MODE;
  double s = 0.0;
#pragma unroll 4
  for (int i = lane_id(); i < dim; i += WAVE) s += (double)qrow[i] * (double)deq_elem(d, q, r, dim, i);
  return s;
}

// Score of row r (wave-uniform) for the query row qrow = f32[dim]; every lane of the wave calls it and
// every lane returns the score.  Lane l takes elements l, l + 64, ... in that order, then the wave
// butterfly: exact f32 x f32 products, f64 accumulation, one rounding to f32.
// VRQ_RESCORE_SIGNED_BINARY (dim a multiple of 128): q = u8[n, dim / 8] packed sign codes, element i =
// +1 if bit i (MSB first) is set, else -1.  Lane l loads bytes 16 l .. 16 l + 15 of the row (one 16-byte
// load; lanes past the row load nothing).  Elements 64 j .. 64 j + 63 are bytes 8 j .. 8 j + 7 = two dwords
// of lane j / 2, read by v_readlane (j is wave-uniform): lanes 0-31 take the first dword, lanes 32-63 the
// second, and within it element 64 j + l is byte (l / 8) % 4 (little-endian) at bit 7 - l % 8 -- the same
// shift at every j.
__device__ __forceinline__ double dequant_dot(int mode, const float* __restrict__ qrow, int dim,
                                              const void* __restrict__ q, const double* __restrict__ minmax,
                                              double limit, int64_t r) {
  const int l = lane_id();
  double s = 0.0;
  if (mode == VRQ_RESCORE_SIGNED_BINARY) {
    const int cb = dim / 8;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (16 * l < cb) w = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(q) + r * cb + 16 * l);
    const int sh = 8 * ((l >> 3) & 3) + 7 - (l & 7);
#pragma unroll 4
    for (int j = 0; j < dim / WAVE; ++j) {
      const int src = j >> 1;
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)((j & 1) ? w.z : w.x), src);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)((j & 1) ? w.w : w.y), src);
      const double x = (double)qrow[j * WAVE + l];
      s += (((l < 32 ? lo : hi) >> sh) & 1u) ? x : -x;
    }
  } else {
    const DeqRow d = deq_row(mode, limit, minmax, r);
    switch (mode) {
      case VRQ_RESCORE_F32: s = deq_lane_sum<VRQ_RESCORE_F32>(d, qrow, dim, q, r); break;
      case VRQ_ENC_INT8_GLOBAL: s = deq_lane_sum<VRQ_ENC_INT8_GLOBAL>(d, qrow, dim, q, r); break;
      case VRQ_ENC_INT16_GLOBAL: s = deq_lane_sum<VRQ_ENC_INT16_GLOBAL>(d, qrow, dim, q, r); break;
      case VRQ_ENC_INT4_GLOBAL: s = deq_lane_sum<VRQ_ENC_INT4_GLOBAL>(d, qrow, dim, q, r); break;
      case VRQ_ENC_INT8_LOCAL: s = deq_lane_sum<VRQ_ENC_INT8_LOCAL>(d, qrow, dim, q, r); break;
      default: s = deq_lane_sum<VRQ_ENC_INT4_LOCAL>(d, qrow, dim, q, r); break;
    }
  }
  s = wave_sum_f64(s);  // exact products, f64 accumulation, one rounding to f32 below
  return (double)(float)s;
}

}  // namespace vrq
