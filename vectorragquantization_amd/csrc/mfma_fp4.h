// mfma_fp4.h -- the FP4 matrix-core form of a Hamming distance, shared by the Phase-I matrix-core scans
// (hamming_mfma.hip for 128-byte codes, hamming_mfma_dim.hip for the other code sizes).
#pragma once

#include "mfma_common.h"

namespace vrq {

constexpr int FMT_FP4 = 4;                  // e2m1 operand format of the f8f6f4 MFMA

// 32 code bits -> one FP4 MFMA fragment lane: 32 e2m1 values.  Dword j, nibble i holds bit 4i + j
// (a fixed permutation of k applied identically to queries and rows, so every dot product is
// unchanged), encoded so that A x B = 1 per common set bit:
//   rows (B):    j = 0, 1, 2: w & (0x11111111 << j) -> codes 0x1 / 0x2 / 0x4 = 0.5 / 1 / 2;
//                j = 3: (w >> 1) & 0x44444444 -> 0x4 = 2           (5 VALU per 32 bits)
//   queries (A): 2 / 1 / 0.5 / 0.5 at the same positions (unpacked once per kernel)
__device__ __forceinline__ v4i unpack_row32(uint32_t w) {
  v4i r;
  r.x = (int)(w & 0x11111111u);
  r.y = (int)(w & 0x22222222u);
  r.z = (int)(w & 0x44444444u);
  r.w = (int)((w >> 1) & 0x44444444u);
  return r;
}
__device__ __forceinline__ v4i unpack_query32(uint32_t w) {
  v4i r;
  r.x = (int)((w << 2) & 0x44444444u);
  r.y = (int)(w & 0x22222222u);
  r.z = (int)((w >> 2) & 0x11111111u);
  r.w = (int)((w >> 3) & 0x11111111u);
  return r;
}

// Unscaled v_mfma_f32_32x32x64_f8f6f4 (scale operands 0 select the unscaled form, 32 cycles; the
// block-scaled form costs 33 on these operands, tools/probes/mfma_shape_probe.hip): 1 per common
// set bit (unpack_row32 x unpack_query32), so C + popcount(q & r) exactly (integers <= 1024 in f32).
// FP4 operands occupy 4 registers; the upper half of the 8-register operand is ignored.
__device__ __forceinline__ v16f mfma_fp4(const v4i& a, const v4i& b, const v16f& c) {
  const v8i a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0};
  const v8i b8 = {b.x, b.y, b.z, b.w, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, FMT_FP4, FMT_FP4, 0, 0, 0, 0);
}

// wave-uniform "any lane has a value > thr in these 16 registers", for thr >= 0: a signed-integer
// max3 tree over the float bit patterns (non-negative floats order like their bits; negative ones
// are below every non-negative pattern, and none of them can exceed thr >= 0), no canonicalisation
__device__ __forceinline__ bool any_above(const v16f& a, float thr) {
  const v16i b = __builtin_bit_cast(v16i, a);
  // tree of depth 3: five independent max3, then two, then one
  const int x0 = max(max(b[0], b[1]), b[2]), x1 = max(max(b[3], b[4]), b[5]), x2 = max(max(b[6], b[7]), b[8]);
  const int x3 = max(max(b[9], b[10]), b[11]), x4 = max(max(b[12], b[13]), b[14]);
  const int y0 = max(max(x0, x1), x2), y1 = max(max(x3, x4), b[15]);
  return __ballot(max(y0, y1) > __float_as_int(thr)) != 0;
}

}  // namespace vrq
