// mfma_common.h -- device helpers shared by the matrix-core kernels (hamming_mfma.hip,
// gemm_topk.hip): compile-time loops, raw barriers / counted waits, and inline-asm LDS accesses
// that the compiler cannot tie to an outstanding LDS-DMA (see the note below).
#pragma once

#include <type_traits>

#include "vrq_internal.h"

namespace vrq {

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

// compile-time loop: f(integral_constant<int, I>) for I in [I0, N) -- every index a constant,
// so register arrays indexed by it stay in registers (a #pragma unroll may give up)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

__device__ __forceinline__ void barrier_all() { asm volatile("s_barrier" ::: "memory"); }
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// LDS accesses inside the tile loop are inline asm: after a global_load_lds the compiler
// would otherwise put s_waitcnt vmcnt(0) before the next LDS access (it cannot tell the
// DMA's target apart), stalling every tile on the DMA just issued.  Loaded registers become
// valid at the matching wait, which takes them as "+v" operands so no use is hoisted above it.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const void*)p);
}
__device__ __forceinline__ void lds_read128(v4i& d, uint32_t a) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(d) : "v"(a) : "memory");
}
// the same read into a loop-carried register set: the destination is an in/out operand, so the read,
// its wait and the loop-carried value form one tied chain the register allocator keeps in one place
// (an output-only destination may be given other registers and copied into the carried ones before
// the wait retires the load -- tests/isa_check.py)
__device__ __forceinline__ void lds_read128_inplace(v4i& d, uint32_t a) {
  asm volatile("ds_read_b128 %0, %1" : "+v"(d) : "v"(a) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read128_imm(v4i& d, uint32_t a) {  // address + immediate offset
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(a), "n"(OFF) : "memory");
}
__device__ __forceinline__ void lds_read64(v2i& d, uint32_t a) {
  asm volatile("ds_read_b64 %0, %1" : "=v"(d) : "v"(a) : "memory");
}
__device__ __forceinline__ void lds_read32(int& d, uint32_t a) {
  asm volatile("ds_read_b32 %0, %1" : "=v"(d) : "v"(a) : "memory");
}
__device__ __forceinline__ void lds_read32_inplace(int& d, uint32_t a) {
  asm volatile("ds_read_b32 %0, %1" : "+v"(d) : "v"(a) : "memory");
}
__device__ __forceinline__ void lds_write128(uint32_t a, const v4i& v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(a), "v"(v) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read32_imm(int& d, uint32_t a) {
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(d) : "v"(a), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_write128_imm(uint32_t a, const v4i& v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(a), "v"(v), "n"(OFF) : "memory");
}
// (a ^ X) + s in one VALU instruction, for per-lane LDS addresses that differ from a kept one by an XOR
// swizzle term: volatile, so the sum is formed where it is used and no copy of it is held across a loop
template <int X>
__device__ __forceinline__ uint32_t xor_add(uint32_t a, uint32_t s) {
  uint32_t d;
  asm volatile("v_xad_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "n"(X), "s"(s));
  return d;
}
// The LDS read at the per-lane address (a ^ X) + s, address form and read in ONE statement: between two asm
// statements the compiler pads a register handed from one to the next with an idle state (s_nop 0), inside a
// statement nothing is padded, and a VALU result needs no wait state before a DS instruction takes it as its
// address.  t is the address register.  It is handed back because the compiler assumes of every asm output
// that the next vector instruction touching its register needs an idle state, looking back across asm
// statements: the caller keeps t live (asm_keep) past the next instruction that writes a fresh register, so
// that instruction is given another one.
template <int X>
__device__ __forceinline__ void lds_read64_xad(v2i& d, uint32_t& t, uint32_t a, uint32_t s) {
  asm volatile("v_xad_u32 %1, %2, %3, %4\n\tds_read_b64 %0, %1" : "=&v"(d), "=&v"(t) : "v"(a), "n"(X), "s"(s) : "memory");
}
// two reads, at (a ^ X0) + s and (a ^ X1) + s (the DS instruction takes its address when it issues, so the
// second address may overwrite the first)
template <int X0, int X1>
__device__ __forceinline__ void lds_read128x2_xad(v4i& d0, v4i& d1, uint32_t& t, uint32_t a, uint32_t s) {
  asm volatile("v_xad_u32 %2, %3, %4, %6\n\tds_read_b128 %0, %2\n\tv_xad_u32 %2, %3, %5, %6\n\tds_read_b128 %1, %2"
               : "=&v"(d0), "=&v"(d1), "=&v"(t)
               : "v"(a), "n"(X0), "n"(X1), "s"(s)
               : "memory");
}
__device__ __forceinline__ void asm_keep(uint32_t t) { asm volatile("" ::"v"(t)); }
// a use of a 16-register value at this point and nothing else (device pass only: the host pass checks asm
// operands against its own registers, takes no 512-bit "v" input and then drops the kernel without a word)
__device__ __forceinline__ void asm_use(const v16f& x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" ::"v"(x));
#endif
}
// A counted LDS wait and the FP4 MFMA (v_mfma_f32_32x32x64_f8f6f4 on e2m1 operands, 4 registers each) that
// consumes the awaited B fragment, as ONE statement.  A wait-only statement that names the fragment "+v" keeps
// its consumers below the wait, but the compiler takes it for a vector write that feeds the MFMA and pads the
// pair with s_nop 0; here the fragment is a plain input, nothing is padded, and the statement being volatile
// keeps its place among the other asm statements (the LDS reads, the waits).  The compiler does not know the
// statement is an MFMA, so the CALLER owns the hazards of `acc`: its next reader must be the next MFMA of the
// same accumulate chain (C = D whole: no wait state) or lie at least 12 issue slots behind an 8-pass MFMA.
// A in the accumulator file ("a"), B and the accumulators in VGPRs.
template <int N>
__device__ __forceinline__ void wait_lgkm_mfma_fp4(v16f& acc, const v4i& a, const v4i& b) {  // acc += A x B
  asm volatile("s_waitcnt lgkmcnt(%3)\n\tv_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %0 cbsz:4 blgp:4"
               : "+v"(acc)
               : "a"(a), "v"(b), "n"(N)
               : "memory");
}
template <int N>
__device__ __forceinline__ void wait_lgkm_mfma_fp4_seed(v16f& acc, const v4i& a, const v4i& b, const v16f& c) {
  asm volatile("s_waitcnt lgkmcnt(%4)\n\tv_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %3 cbsz:4 blgp:4"
               : "=&v"(acc)
               : "a"(a), "v"(b), "v"(c), "n"(N)
               : "memory");
}
template <int N>
__device__ __forceinline__ void wait_lgkm_mfma_fp4_zero(v16f& acc, const v4i& a, const v4i& b) {  // acc = A x B
  asm volatile("s_waitcnt lgkmcnt(%3)\n\tv_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, 0 cbsz:4 blgp:4"
               : "=&v"(acc)
               : "a"(a), "v"(b), "n"(N)
               : "memory");
}
// One 16-byte-per-lane LDS-DMA piece: M0 (the LDS destination of lane 0) is written in the statement that
// reads it -- the compiler reserves M0 and does not keep it across statements -- and an SALU write of M0
// needs ONE wait state before the LDS-DMA that reads it (the s_nop 0 the compiler also puts there; in the
// xor form the address VALU fills that state).  voff: per-lane byte offset from the wave-uniform base.
__device__ __forceinline__ void lds_dma16(const void* base, uint32_t voff, uint32_t lds_a, uint32_t lds_b) {
  asm volatile("s_add_i32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               ::"v"(voff), "s"(base), "s"(lds_a), "s"(lds_b)
               : "memory");
}
// the same at per-lane offset (voff ^ X) + add: t is the address register (handed back: see lds_read64_xad)
template <int X>
__device__ __forceinline__ void lds_dma16_xad(const void* base, uint32_t& t, uint32_t voff, uint32_t add,
                                              uint32_t lds_a, uint32_t lds_b) {
  asm volatile("s_add_i32 m0, %4, %5\n\tv_xad_u32 %0, %1, %6, %2\n\tglobal_load_lds_dwordx4 %0, %3"
               : "=&v"(t)
               : "v"(voff), "s"(add), "s"(base), "s"(lds_a), "s"(lds_b), "n"(X)
               : "memory");
}
__device__ __forceinline__ void lds_write32(uint32_t a, int v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_add32(uint32_t a, int v) {
  asm volatile("ds_add_u32 %0, %1" ::"v"(a), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_add_rtn32(int& d, uint32_t a, int v) {
  asm volatile("ds_add_rtn_u32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(v) : "memory");
}
#define VRQ_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)

}  // namespace vrq
