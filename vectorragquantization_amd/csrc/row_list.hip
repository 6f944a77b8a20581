// row_list.hip -- vrq_row_list: the allow-bitmap of the filtered calls (u64 [ceil(n / 64)], row r = bit r & 63 of
// word r >> 6) as the ascending list of its rows below n, u32 [m], with m as a device int64.  The list is what the
// gathered exhaustive passes (K5g, gemm_topk_dim.hip) read their tiles through; it is built once per filter.
//
// The order comes from popcount prefix sums, never from atomics, so the list is deterministic and ascending:
//   count   one word per thread: popcount -> exclusive prefix inside the wave (DPP-free: 6 shuffle steps) -> the
//           waves' totals through LDS -> the block's total to blocks[b];
//   scan    one workgroup walks blocks[] in strides of its size with a running carry: blocks[b] becomes the
//           exclusive prefix over the blocks, *out_m the total;
//   emit    the count kernel's prefixes again + blocks[b] = the list position of the thread's first row; the
//           thread writes its word's rows, lowest bit first.
// Bits at or past n in the last word are masked off in both kernels.  rows == NULL: count and scan only.
#include "vrq_internal.h"

namespace vrq {
namespace rowlist {

constexpr int NT = 256, NW = NT / WAVE;  // one word per thread: 16384 rows per workgroup

__device__ __forceinline__ uint64_t masked_word(const uint64_t* __restrict__ allow, int64_t wi, int64_t nwords,
                                                int64_t n) {
  if (wi >= nwords) return 0ull;
  uint64_t w = allow[wi];
  const int64_t left = n - wi * 64;  // rows of this word below n: 1 .. 64 except past the end
  if (left < 64) w &= (1ull << left) - 1ull;
  return w;
}

// exclusive prefix of c over the workgroup's threads (thread order) and the workgroup's total
__device__ __forceinline__ int block_prefix(int c, int& total, int* wsum) {
  const int l = lane_id(), w = threadIdx.x >> 6;
  int incl = c;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const int y = __shfl_up(incl, d, WAVE);
    if (l >= d) incl += y;
  }
  if (l == WAVE - 1) wsum[w] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    before += i < w ? wsum[i] : 0;
    total += wsum[i];
  }
  return before + incl - c;
}

__global__ __launch_bounds__(NT) void count_kernel(const uint64_t* __restrict__ allow, int64_t nwords, int64_t n,
                                                   int64_t* __restrict__ blocks) {
  __shared__ int wsum[NW];
  const uint64_t w = masked_word(allow, (int64_t)blockIdx.x * NT + threadIdx.x, nwords, n);
  int total;
  block_prefix(__popcll(w), total, wsum);
  if (threadIdx.x == 0) blocks[blockIdx.x] = total;
}

__global__ __launch_bounds__(NT) void scan_kernel(int64_t* __restrict__ blocks, int64_t nblocks,
                                                  int64_t* __restrict__ out_m) {
  __shared__ int wsum[NW];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nblocks; b0 += NT) {
    const int64_t b = b0 + threadIdx.x;
    const int c = b < nblocks ? (int)blocks[b] : 0;  // <= 16384 each, <= 2^22 per stride
    int total;
    const int ex = block_prefix(c, total, wsum);
    if (b < nblocks) blocks[b] = carry + ex;
    carry += total;
    __syncthreads();  // wsum is reused by the next stride
  }
  if (threadIdx.x == 0) *out_m = carry;
}

__global__ __launch_bounds__(NT) void emit_kernel(const uint64_t* __restrict__ allow, int64_t nwords, int64_t n,
                                                  const int64_t* __restrict__ blocks, uint32_t* __restrict__ rows,
                                                  int64_t rows_cap) {
  __shared__ int wsum[NW];
  const int64_t wi = (int64_t)blockIdx.x * NT + threadIdx.x;
  uint64_t w = masked_word(allow, wi, nwords, n);
  int total;
  int64_t pos = blocks[blockIdx.x] + block_prefix(__popcll(w), total, wsum);
  const uint32_t base = (uint32_t)(wi * 64);
  while (w) {
    if (pos < rows_cap) rows[pos] = base + (uint32_t)__builtin_ctzll(w);
    ++pos;
    w &= w - 1;
  }
}

__host__ inline int64_t blocks_of(int64_t n) { return ((n + 63) / 64 + NT - 1) / NT; }

}  // namespace rowlist
}  // namespace vrq

using namespace vrq;

extern "C" {

size_t vrq_row_list_workspace_size(int64_t n) {
  if (n < 1 || n >= (int64_t(1) << 32)) return 0;
  return ((size_t)rowlist::blocks_of(n) * sizeof(int64_t) + 255) & ~size_t(255);
}

int vrq_row_list(const uint64_t* allow, int64_t n, uint32_t* rows, int64_t rows_cap, int64_t* out_m, void* workspace,
                 size_t workspace_bytes, void* stream) {
  if (n < 1 || n >= (int64_t(1) << 32)) return VRQ_EUNSUPPORTED;
  VRQ_CHECK_ARG(allow && out_m && workspace && ((uintptr_t)allow & 7) == 0 && ((uintptr_t)workspace & 7) == 0 &&
                (!rows || rows_cap >= 0));
  if (workspace_bytes < vrq_row_list_workspace_size(n)) return VRQ_EWORKSPACE;
  const hipStream_t s = (hipStream_t)stream;
  const int64_t nwords = (n + 63) / 64, nb = rowlist::blocks_of(n);
  int64_t* blocks = (int64_t*)workspace;
  hipLaunchKernelGGL(rowlist::count_kernel, dim3((unsigned)nb), dim3(rowlist::NT), 0, s, allow, nwords, n, blocks);
  VRQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(rowlist::scan_kernel, dim3(1), dim3(rowlist::NT), 0, s, blocks, nb, out_m);
  VRQ_LAUNCH_CHECK();
  if (rows) {
    hipLaunchKernelGGL(rowlist::emit_kernel, dim3((unsigned)nb), dim3(rowlist::NT), 0, s, allow, nwords, n,
                       (const int64_t*)blocks, rows, rows_cap);
    VRQ_LAUNCH_CHECK();
  }
  return VRQ_OK;
}

}  // extern "C"
