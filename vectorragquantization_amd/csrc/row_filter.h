// row_filter.h -- the FILTER axis of the counting scan's kernels (hamming_count.hip, hamming_count_mfma.hip) and
// what its per-query value shares between them.
//
// FILTER_OFF: every row takes part.  FILTER_ONE: one bitmap for every query of the call (vrq_*_filtered, a
// vrq_*_batch call with a bitmap).  FILTER_SETS: `allow` holds nsets bitmaps of set_words u64 words each and
// query q is filtered by bitmap query_set[q] (vrq_*_perquery): -1 allows every row, any other id outside
// [0, nsets) allows none.  A set id is turned into a SetRef before any address is formed: an id that names no
// bitmap gets offset 0 and its loaded word is replaced, so every address a kernel forms lies in bitmap 0 .. nsets - 1.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace vrq {

constexpr int FILTER_OFF = 0, FILTER_ONE = 1, FILTER_SETS = 2;

struct SetRef {
  int64_t off;  // first word of the query's bitmap in `allow` (0 where all or none)
  bool all;     // unfiltered (set id -1)
  bool none;    // no row is allowed: an id that names no bitmap, or a query slot past nq
};

__device__ __forceinline__ SetRef set_ref(int sid, bool real, int nsets, int64_t set_words) {
  SetRef r;
  r.all = real && sid == -1;
  r.none = !real || sid < -1 || sid >= nsets;
  r.off = (r.all || r.none) ? 0 : (int64_t)sid * set_words;
  return r;
}

// Word idx of the bitmap at `off`: a scalar load through the constant address space (off and idx are
// wave-uniform, the bitmaps are read-only for the kernel's lifetime), like the single bitmap's word.
__device__ __forceinline__ uint64_t set_word(const uint64_t* allow, int64_t off, bool all, bool none, int idx) {
  typedef const __attribute__((address_space(4))) uint64_t* const_u64_ptr;
  const uint64_t w = ((const_u64_ptr)(uintptr_t)allow)[off + (int64_t)idx];
  return none ? 0ull : all ? ~0ull : w;
}

// The set id of query q, read at a wave-uniform address (a scalar load).
__device__ __forceinline__ int set_id_uniform(const int32_t* query_set, int q) {
  typedef const __attribute__((address_space(4))) int32_t* const_i32_ptr;
  return __builtin_amdgcn_readfirstlane(((const_i32_ptr)(uintptr_t)query_set)[q]);
}

// The sets of the up to 64 query slots of a K1hm wave, lane i holding slot i: the bitmap offsets stay in two
// VGPRs and reach the scalar unit by v_readlane, the two flags of every slot are ballots.
struct WaveSets {
  int32_t off_lo, off_hi;  // lane i: SetRef::off of slot i
  uint64_t all, none;      // bit i: SetRef::all / SetRef::none of slot i
  bool uniform;            // every real slot names the same set: slot 0's word serves the wave

  // q: the query of this lane's slot; real: the slot holds a query of the call
  __device__ __forceinline__ void init(const int32_t* query_set, int q, bool real, int nsets, int64_t set_words) {
    const int sid = real ? query_set[q] : -2;
    const SetRef r = set_ref(sid, real, nsets, set_words);
    off_lo = (int32_t)(uint32_t)r.off;
    off_hi = (int32_t)(r.off >> 32);
    all = __ballot(r.all);
    none = __ballot(r.none);
    const int sid0 = __builtin_amdgcn_readfirstlane(sid);  // slot 0 is real: the wave has a query
    uniform = __all(!real || sid == sid0);
  }
  // the word of slot s (wave-uniform) for bitmap word idx
  __device__ __forceinline__ uint64_t word(const uint64_t* allow, int s, int idx) const {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(off_lo, s);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(off_hi, s);
    return set_word(allow, (int64_t)(((uint64_t)hi << 32) | lo), (all >> s) & 1, (none >> s) & 1, idx);
  }
};

}  // namespace vrq
