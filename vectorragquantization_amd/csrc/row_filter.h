// row_filter.h -- the FILTER axis of the counting scan's kernels (hamming_count.hip, hamming_count_mfma.hip) and
// what its per-query value shares between them.
//
// FILTER_OFF: every row takes part.  FILTER_ONE: one bitmap for every query of the call (vrq_*_filtered, a
// vrq_*_batch call with a bitmap).  FILTER_SETS: `allow` holds nsets bitmaps of set_words u64 words each and
// query q is filtered by bitmap query_set[q] (vrq_*_perquery): -1 allows every row, any other id outside
// [0, nsets) allows none.  A set id is turned into a SetRef before any address is formed: an id that names no
// bitmap gets offset 0 and its loaded word is replaced, so every address a kernel forms lies in bitmap 0 .. nsets - 1.
//
// FILTER_ROWS (K1g; vrq_*_gather): the scan runs in the row space [0, m) of an ascending list `rows` u32 [m] and
// reads only the listed rows.  Chunks, tiles, histograms and prefixes count list positions; the list is
// consulted for the DMA source address of a tile piece and for the row field of an emitted key, nowhere else.
// RowSlab (below) is how the entries reach the lanes, on both engines.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace vrq {

constexpr int FILTER_OFF = 0, FILTER_ONE = 1, FILTER_SETS = 2, FILTER_ROWS = 3;

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

// The list entries of a wave's tiles (FILTER_ROWS): a wave-private LDS slab of SLOTS runs of 64 entries, the run
// of the wave's k-th tile in slot k % SLOTS.  A run is one coalesced 256-byte LDS-DMA (one wave instruction on
// the vm counter, entry of tile row i from lane i), requested two tiles before the tile's pieces are issued, so
// the ring's counted wait grows by exactly one: the order on the counter is T(i), E(i+2), T(i+1), E(i+3), and
// vmcnt(C + 1) retires T(i) and E(i+2) together.  A lane then takes the entry of each of its pieces (tile row
// (64 gi + l) / C) with one ds_read_b32 in front of the tile's own reads; the lgkmcnt(0) that retires those
// retires the entries, so the steady loop has no wait of its own for them.  Nothing of the list stays in VGPRs
// across a tile, which is what the 256-VGPR instances need, and one scheme serves both engines.  (An entry per
// lane in a register and ds_bpermute per piece would need the entries of four tiles in rotating registers while
// two of them are still in flight; per-piece vector loads, K5g's way, put C more instructions per tile on the
// vm counter.)  Every position is clamped to the chunk's last row, so every address comes from a list entry.
template <int SLOTS>
struct RowSlab {
  static_assert(SLOTS >= 4 && (SLOTS & (SLOTS - 1)) == 0, "two tiles of pieces and two runs are in flight");
  static constexpr int BYTES = SLOTS * 256;
  uint8_t* slab;
  const uint32_t* rows;
  int64_t row0, row1;  // the chunk's list positions
  int first, step;     // the wave's k-th tile is chunk tile first + k * step
  int l;

  // the run of the wave's k-th tile (k wave-uniform) -> slot k % SLOTS
  __device__ __forceinline__ void request(int k) const {
    int64_t v = row0 + (int64_t)(first + k * step) * 64 + l;
    v = v < row1 ? v : row1 - 1;
    __builtin_amdgcn_global_load_lds(rows + v, (__attribute__((address_space(3))) void*)(slab + (k & (SLOTS - 1)) * 256),
                                     4, 0, 0);
  }
  // entry of tile row r of the wave's k-th tile; valid after the caller's next lgkmcnt(0)
  __device__ __forceinline__ void entry(uint32_t& d, int k, int r) const {
    const uint32_t a = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const void*)slab) +
                       (uint32_t)((k & (SLOTS - 1)) * 256 + r * 4);
    asm volatile("ds_read_b32 %0, %1" : "=v"(d) : "v"(a) : "memory");
  }
  // the entries of the pieces lane l issues for the wave's k-th tile (C pieces per lane, piece gi of tile row
  // (64 gi + l) / C); valid after the caller's next lgkmcnt(0) and a pin()
  template <int C>
  __device__ __forceinline__ void piece_entries(int k, uint32_t (&pa)[C]) const {
#pragma unroll
    for (int gi = 0; gi < C; ++gi) entry(pa[gi], k, (gi * 64 + l) / C);
  }
  template <int C>
  static __device__ __forceinline__ void pin(uint32_t (&pa)[C]) {  // no use is hoisted above the wait before it
#pragma unroll
    for (int gi = 0; gi < C; ++gi) asm volatile("" : "+v"(pa[gi]));
  }
  // Fills the ring of a wave with ntw >= 1 tiles: leaves T(0), E(2), T(1), E(3) on the vm counter in that order,
  // which is the order every steady iteration i restores with issue_rows(i + 2) and request(i + 4).  Runs are
  // requested whether or not their tile exists (their positions are clamped), so the counted wait of an
  // iteration does not depend on how many tiles are left.
  template <class Ring>
  __device__ __forceinline__ void fill(const Ring& tr, int ntw) const {
    uint32_t pa[Ring::C];
    request(0);
    request(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    piece_entries(0, pa);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pin(pa);
    tr.issue_rows(0, pa);
    request(2);
    if (ntw > 1) {
      piece_entries(1, pa);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      pin(pa);
      tr.issue_rows(1, pa);
    }
    request(3);
  }
};

}  // namespace vrq
