// wave_scan.h -- device helpers shared by the wavefront Phase-I scans: K1 (hamming_scan.hip, 128-byte
// codes) and K1d (search_dim.hip, the other code sizes).
#pragma once

#include "vrq_internal.h"

namespace vrq {

constexpr int LOCAL_BITS = 20;
constexpr uint32_t LOCAL_MASK = (1u << LOCAL_BITS) - 1;

// Wave-level bitonic sort (ascending) of the CAP u32 keys at buf[0..CAP);
// entries at index >= cnt are treated as +inf.  Result written back to buf.
template <int CAP>
__device__ __forceinline__ void wave_sort_keys(uint32_t* buf, int cnt) {
  constexpr int E = CAP / WAVE;
  int l = lane_id();
  // opaque lane id: keeps the network's lane masks from being hoisted into the scan
  // loop, where they would hold ~100 SGPRs live and push the resident query words out
  asm volatile("" : "+v"(l));
  uint32_t v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = e * WAVE + l;
    v[e] = (i < cnt) ? buf[i] : 0xffffffffu;
  }
#pragma unroll
  for (int size = 2; size <= CAP; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride >= WAVE) {
        const int es = stride / WAVE;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if ((e & es) == 0) {
            const int i = e * WAVE + l;
            const bool up = (i & size) == 0;
            const uint32_t a = v[e], b = v[e + es];
            const uint32_t mn = a < b ? a : b, mx = a < b ? b : a;
            v[e] = up ? mn : mx;
            v[e + es] = up ? mx : mn;
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int i = e * WAVE + l;
          const uint32_t p = shfl_xor_u32(v[e], stride);
          const bool up = (i & size) == 0;
          const bool lower = (l & stride) == 0;
          const uint32_t mn = v[e] < p ? v[e] : p, mx = v[e] < p ? p : v[e];
          v[e] = (lower == up) ? mn : mx;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) buf[e * WAVE + l] = v[e];
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef uint32_t v16u __attribute__((ext_vector_type(16)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const void*)p);
}

// d += popcount(q ^ r): v_xor_b32 (SGPR q) + v_bcnt_u32_b32 (bcnt accumulates).  The
// empty asm pins the accumulation order so LLVM does not re-associate the chain
// into bcnt(x,0) + v_add3 trees (+15 % VALU).
__device__ __forceinline__ void xor_bcnt(uint32_t& d, uint32_t q, uint32_t r) {
  d = __popc(q ^ r) + d;
  asm("" : "+v"(d));
}

template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {  // provably wave-uniform (SGPR) pointer
  const uint64_t u = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return (T*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ void lds_barrier() { asm volatile("s_barrier" ::: "memory"); }

}  // namespace vrq
