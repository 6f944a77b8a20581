// hamming_count_mfma.hip -- K1hm: the count and emit stages of the counting scan (hamming_count.hip) on the
// matrix cores, for every code size, with and without the row bitmap.  The threshold stage and the large
// finish run unchanged on what these kernels leave: histograms u32 [query][chunk][dim + 1], and K-lists whose
// dist < T part and dist == T part are each in row order.
//
// The distance engine is K1rd's (hamming_mfma_dim.hip): the queries of a wave are resident as FP4 A fragments,
// each wave LDS-DMAs its own 64-row tiles into a two-slot ring in K1d's rotated image, every 32-bit piece of a
// row is unpacked straight into the B fragment of one k-step, and dist = pc(q) + pc(r) - 2 <q, r> is exact in
// f32.  Register g of lane half hh of an accumulator holds query (g & 3) + 8 (g >> 2) + 4 hh of the M-block,
// row lane & 31 of the n-block.  128-byte codes (C = 8 pieces, rotation shift 1 as in K1h) have an instance.
//
//  count  accumulators start at -pc(q) / 2, so dist = pc(r) - 2 acc.  Every live (query, row) pair adds 1 to
//         its LDS bin: no bound, no sample.  Bins are u16 pairs in a u32 -- the two queries that one register
//         holds in its two lane halves share a word, the low half adds 1 and the high half 65536 -- so 32
//         queries take (dim + 1) * 64 bytes; at 2048 dims that is 128 KiB + 64 B, which leaves no room for a
//         ring, so the M-block there is half populated (16 real queries, registers 0..7).  A workgroup adds its
//         bins into its own slab of the workspace (plain vector loads and stores; it alone owns the slab) after
//         every kCountFlushRows = 65 280 rows, so no u16 can pass 65 280 whatever the chunk length.
//  emit   one wave per (chunk, 32 MB queries) walks the chunk's n-blocks in row order.  Accumulators start at
//         (T(q) + 1 - pc(q)) / 2, so a row is in the list iff acc > pc(r) / 2: one max3 tree and one compare
//         per M-block.  On a hit, pc(r) - 2 acc = dist - T - 1 tells dist < T from dist == T; the ballot over
//         register g holds the 32 rows of one query in its low half and those of the query 4 further in its
//         high half, in row order, so a row's rank is the mbcnt within its own half plus the query's running
//         position (kept in LDS).  Positions follow hamming_emit_kernel's rule; no global atomics.
//
// Dead pairs never count and never hit: rows past the chunk's end, rows whose bitmap bit is clear, query
// slots past nq (zero A fragments; their seed never accepts in emit, their adds are masked in count).
// Every loop has a trip count fixed by the kernel arguments; no workgroup waits for another.
//
// Per-query sets (FILTER_SETS; row_filter.h).  Lane i of a wave keeps the bitmap offset of query slot i (WaveSets),
// read once at kernel entry; a slot's word of a tile is a scalar load at base + v_readlane(offset), on the lgkm
// counter like the single bitmap's word, so the ring's counted vm waits are untouched.  count: once per tile the
// words of the wave's slots are turned into a per-lane mask "which slots allow my row" for each n-block, so
// register g of M-block m tests bit slot_of(g, 0) of the mask shifted by 4 hh; the OR of the words plays the
// single word's part for the tile and n-block skips.  emit: the tile loop needs the OR of the words alone (the
// any_above pre-test keeps a per-row predicate); the (query, row) bit is applied in the rare hit path, before
// the ballots.  When every real slot of the wave names one set, a wave-uniform test at entry takes the
// single-word path with that set's word.
#include <limits.h>

#include "mfma_common.h"
#include "mfma_fp4.h"
#include "row_filter.h"
#include "vrq_internal.h"
#include "vrq_scan.h"

namespace vrq {

namespace {

// rows a count workgroup scans between two flushes of its u16 bins (1020 tiles: a multiple of 2 and 4 waves)
constexpr int kCountFlushRows = 65280;
static_assert(kCountFlushRows < 65536 && kCountFlushRows % 256 == 0, "u16 bins");

template <int KS>
struct CountCode {
  static constexpr int CB = 8 * KS, BINS = 64 * KS + 1, C = CB / 16, NPH = (C + 1) / 2, TILE = 64 * CB;
  // K1d's rotation (search_dim.hip), with K1h's shift for 128-byte rows
  static constexpr int SHIFT = C == 2 ? 3 : C == 4 ? 2 : C == 6 ? 4 : C == 8 ? 1 : C == 12 ? 2 : C == 16 ? 0 : -1;
  static_assert(C == 3 || SHIFT >= 0, "code size");
  static constexpr int NW = CB <= 128 ? 4 : 2;      // waves of a count workgroup
  static constexpr int QREAL = CB == 256 ? 16 : 32;  // real queries of a count M-block
  static constexpr int NG = QREAL / 2;               // accumulator registers that hold them
  __host__ __device__ static constexpr int rot(int r) { return SHIFT < 0 ? 0 : (r >> SHIFT) % C; }
  template <int MB>
  static constexpr int count_lds() { return MB * NG * BINS * 4 + NW * 2 * TILE; }
};

__device__ __forceinline__ int linear_block() {  // XCD-aware, bijective (K1h's)
  const int nb = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, slot = b >> 3, q8 = nb >> 3, r8 = nb & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// the bitmap word of tile `tile` of the chunk at row0: a scalar load through the constant address space
__device__ __forceinline__ uint64_t tile_allow_word(const uint64_t* allow, int64_t row0, int tile) {
  typedef const __attribute__((address_space(4))) uint64_t* const_u64_ptr;
  const int idx = __builtin_amdgcn_readfirstlane((int)(row0 >> 6) + tile);  // n < 2^32: below 2^26
  return ((const_u64_ptr)(uintptr_t)allow)[idx];
}

// A wave's distance engine: its tile ring, its resident queries and the MFMAs of one n-block.
template <int KS, int MB>
struct Engine {
  using Cd = CountCode<KS>;
  static constexpr int CB = Cd::CB, C = Cd::C, NPH = Cd::NPH, TILE = Cd::TILE;
  uint8_t* ring;  // two slots
  const uint8_t* codes;
  int64_t row0, row1;
  int l, h, ri;
  uint32_t raddr[2][NPH];  // piece j of this lane's half of row 32 nb + ri, in slot 0
  v4i A[MB][KS];

  __device__ __forceinline__ Engine(uint8_t* ring_, const uint8_t* codes_, int64_t r0, int64_t r1)
      : ring(ring_), codes(codes_), row0(r0), row1(r1), l(lane_id()) {
    h = l >> 5;
    ri = l & 31;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int j = 0; j < NPH; ++j) {
        const int r = 32 * nb + ri;
        const int c = C == 3 ? (j == 0 ? h : 2) : h * NPH + j;
        raddr[nb][j] = lds_addr(ring) + (uint32_t)((r * C + (c + Cd::rot(r)) % C) * 16);
      }
  }
  // A fragments of M-block m from query q (qok: a real query); returns pc(q) in both lane halves
  __device__ __forceinline__ int load_query(int m, const uint8_t* queries, int q, bool qok) {
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(queries + (int64_t)(qok ? q : 0) * CB);
    int pc = 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int di = C == 3 ? (s < 4 ? 4 * h + s : 8 + 2 * h + (s - 4)) : h * KS + s;
      const uint32_t wd = qok ? qp[di] : 0u;
      pc += __popc(wd);
      A[m][s] = unpack_query32(wd);
    }
    return pc + __shfl_xor(pc, 32, 64);
  }
  // tile `tile` of the chunk -> slot (C wave instructions on the vm counter); rows past row1 are clamped
  __device__ __forceinline__ void issue(int tile, int slot) const {
    uint8_t* buf = ring + slot * TILE;
    const int64_t tr0 = row0 + (int64_t)tile * 64;
#pragma unroll
    for (int gi = 0; gi < C; ++gi) {
      const int p = gi * 64 + l;
      const int r = p / C, cs = p % C;
      const int c = (cs + C - Cd::rot(r)) % C;
      int64_t row = tr0 + r;
      row = row < row1 ? row : row1 - 1;
      __builtin_amdgcn_global_load_lds(codes + row * CB + c * 16,
                                       (__attribute__((address_space(3))) void*)(buf + gi * 1024), 16, 0, 0);
    }
  }
  // both n-blocks of the tile in `slot` -> registers, retired before return
  __device__ __forceinline__ void read(int slot, v4i (&rb)[2][NPH]) const {
    const uint32_t boff = (uint32_t)(slot * TILE);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int j = 0; j < NPH; ++j) lds_read128(rb[nb][j], raddr[nb][j] + boff);
    wait_lgkm0();
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int j = 0; j < NPH; ++j) asm volatile("" : "+v"(rb[nb][j]));
  }
  // acc[m] = seed[m] + <q, r> for the n-block's rows; returns pc(r) of the lane's row
  __device__ __forceinline__ int block(const v4i (&rb)[NPH], const v16f (&seed)[MB], v16f (&acc)[MB]) const {
    int pcs = 0;
    static_for<0, KS>([&](auto S) {
      constexpr int s = decltype(S)::value;
      uint32_t wd;
      if constexpr (C == 3 && s >= 4)
        wd = (uint32_t)(h ? rb[1][s - 2] : rb[1][s - 4]);
      else
        wd = (uint32_t)rb[s >> 2][s & 3];
      const v4i bfrag = unpack_row32(wd);
      static_for<0, MB>([&](auto M) {
        constexpr int m = decltype(M)::value;
        if constexpr (s == 0)
          acc[m] = mfma_fp4(A[m][s], bfrag, seed[m]);
        else
          acc[m] = mfma_fp4(A[m][s], bfrag, acc[m]);
      });
      pcs += __popc(wd);
    });
    return pcs + __shfl_xor(pcs, 32, 64);
  }
};

// query slot (within its M-block) that register g of lane half hh holds
__device__ __forceinline__ int slot_of(int g, int hh) { return (g & 3) + 8 * (g >> 2) + 4 * hh; }

}  // namespace

// ---- count ----
template <int KS, int MB, int FILTER>
__global__ __launch_bounds__(64 * CountCode<KS>::NW) void hamming_count_mfma_kernel(
    const uint8_t* __restrict__ codes, int64_t n, const uint8_t* __restrict__ queries, int nq, int64_t chunk_rows,
    int nchunks, int nqb, uint32_t* __restrict__ hist_out, const uint64_t* __restrict__ allow, int nsets,
    int64_t set_words, const int32_t* __restrict__ query_set) {
  using Cd = CountCode<KS>;
  using Eng = Engine<KS, MB>;
  constexpr int C = Cd::C, NPH = Cd::NPH, NW = Cd::NW, BINS = Cd::BINS, QREAL = Cd::QREAL, NG = Cd::NG;
  constexpr int WORDS = MB * NG * BINS;
  static_assert(Cd::template count_lds<MB>() <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) uint8_t ring[NW * 2 * Cd::TILE];
  __shared__ uint32_t hist[WORDS];

  const int L = linear_block();
  const int chunk = L / nqb;
  const int qb = L - chunk * nqb;
  if (chunk >= nchunks) return;
  const int64_t row0 = (int64_t)chunk * chunk_rows;
  const int64_t row1 = (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  const int nrows = (int)(row1 - row0);
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = qb * (QREAL * MB);

  for (int i = tid; i < WORDS; i += 64 * NW) hist[i] = 0;

  Eng e(ring + w * 2 * Cd::TILE, codes, row0, row1);
  const int l = e.l, h = e.h, ri = e.ri;
  // resident queries; seeds -pc(q) / 2 per register, and the registers whose query is real (bit g)
  __shared__ int32_t pcq[NW][MB * 32];
  v16f seed[MB];
  uint32_t qlive[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int q = q0 + m * QREAL + ri;
    const bool qok = ri < QREAL && q < nq;
    const int pc = e.load_query(m, queries, q, qok);
    if (h == 0) pcq[w][m * 32 + ri] = qok ? pc : 0;
  }
  __syncthreads();  // the zeroed bins and pcq (no DMA in flight yet)
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    qlive[m] = 0;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int sl = slot_of(g, h);
      seed[m][g] = -0.5f * (float)pcq[w][m * 32 + sl];
      if (g < NG && q0 + m * QREAL + sl < nq) qlive[m] |= 1u << g;
    }
  }
  const uint32_t hist0 = lds_addr(hist);
  const int inc = h ? 0x10000 : 1;
  WaveSets sets;  // lane i: slot i & 31 of M-block i >> 5
  if constexpr (FILTER == FILTER_SETS) {
    const int q = q0 + (l >> 5) * QREAL + ri;
    sets.init(query_set, q, (l >> 5) < MB && ri < QREAL && q < nq, nsets, set_words);
  }

  const int ntiles = (nrows + 63) >> 6;
  constexpr int SEGT = kCountFlushRows / 64;  // tiles between flushes
  const int nseg = (ntiles + SEGT - 1) / SEGT;
  for (int seg = 0; seg < nseg; ++seg) {
    const int t0 = seg * SEGT;
    const int nts = ntiles - t0 < SEGT ? ntiles - t0 : SEGT;
    // this wave's tiles of the segment: t0 + w, t0 + w + NW, ...
    const int ntw = w < nts ? (nts - w + NW - 1) / NW : 0;
    if (ntw > 0) e.issue(t0 + w, 0);
    if (ntw > 1) e.issue(t0 + w + NW, 1);
    for (int i = 0; i < ntw; ++i) {
      if (i + 1 < ntw) wait_vm<C>(); else wait_vm<0>();
      const int tile = t0 + w + i * NW;
      v4i rb[2][NPH];
      e.read(i & 1, rb);
      if (i + 2 < ntw) e.issue(tile + 2 * NW, i & 1);  // (the slot's reads are retired)
      uint64_t word = ~0ull;
      if constexpr (FILTER == FILTER_ONE) {
        word = tile_allow_word(allow, row0, tile);
        if (word == 0) continue;  // no allowed row in this tile (wave-uniform; its loads were issued and waited)
      }
      // FILTER_SETS, mixed sets: bit s of smask[nb][m] says slot s of M-block m allows this lane's row of n-block nb
      uint32_t smask[2][MB];
      bool mixed = false;
      if constexpr (FILTER == FILTER_SETS) {
        const int idx = __builtin_amdgcn_readfirstlane((int)(row0 >> 6) + tile);
        mixed = !sets.uniform;
        if (mixed) {
          word = 0;
#pragma unroll
          for (int m = 0; m < MB; ++m) {
            smask[0][m] = smask[1][m] = 0;
#pragma unroll
            for (int sl = 0; sl < QREAL; ++sl) {
              const uint64_t ws = sets.word(allow, 32 * m + sl, idx);
              word |= ws;
              smask[0][m] |= (((uint32_t)ws >> ri) & 1u) << sl;
              smask[1][m] |= (((uint32_t)(ws >> 32) >> ri) & 1u) << sl;
            }
          }
        } else {
          word = sets.word(allow, 0, idx);
        }
        if (word == 0) continue;  // no allowed row of any resident query in this tile (wave-uniform)
      }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const uint32_t half = (uint32_t)(word >> (32 * nb));
        if (FILTER && half == 0) continue;  // (wave-uniform)
        if (tile * 64 + nb * 32 >= nrows) continue;  // the ragged last tile has no second n-block (wave-uniform)
        const bool rlive = tile * 64 + nb * 32 + ri < nrows && ((half >> ri) & 1);
        v16f acc[MB];
        const int prow = e.block(rb[nb], seed, acc);
        if (FILTER == FILTER_SETS && mixed) {
          if (rlive) {
            const float pr = (float)prow;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
              const uint32_t sm = smask[nb][m] >> (4 * h);  // (slots past nq are `none`: their bits are clear)
#pragma unroll
              for (int g = 0; g < NG; ++g)
                if ((sm >> slot_of(g, 0)) & 1) {
                  const int d = (int)(pr - 2.0f * acc[m][g]);
                  lds_add32(hist0 + (uint32_t)(((m * NG + g) * BINS + d) * 4), inc);
                }
            }
          }
          continue;
        }
        if (rlive) {
          const float pr = (float)prow;
#pragma unroll
          for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int g = 0; g < NG; ++g)
              if ((qlive[m] >> g) & 1) {
                const int d = (int)(pr - 2.0f * acc[m][g]);  // exact: integers <= dim
                lds_add32(hist0 + (uint32_t)(((m * NG + g) * BINS + d) * 4), inc);
              }
        }
      }
    }
    wait_vm<0>();
    wait_lgkm0();
    __syncthreads();  // every add of the segment is in the bins
    // the workgroup's own slab: bins of the first segment are stored, later ones added
    for (int i = tid; i < WORDS; i += 64 * NW) {
      const uint32_t v = hist[i];
      const int p = i / BINS, b = i - p * BINS;
      const int m = p / NG, g = p - m * NG;
      const int qlo = q0 + m * QREAL + slot_of(g, 0), qhi = qlo + 4;
      if (qlo < nq) {
        uint32_t* o = hist_out + ((int64_t)qlo * nchunks + chunk) * BINS + b;
        *o = seg == 0 ? (v & 0xffffu) : *o + (v & 0xffffu);
      }
      if (qhi < nq) {
        uint32_t* o = hist_out + ((int64_t)qhi * nchunks + chunk) * BINS + b;
        *o = seg == 0 ? (v >> 16) : *o + (v >> 16);
      }
      hist[i] = 0;
    }
    __syncthreads();
  }
}

// ---- emit ----
template <int KS, int MB, int FILTER>
__global__ __launch_bounds__(64) void hamming_emit_mfma_kernel(
    const uint8_t* __restrict__ codes, int64_t n, const uint8_t* __restrict__ queries, int nq, int K,
    int64_t chunk_rows, int nchunks, int nqb, const int32_t* __restrict__ tc, const int32_t* __restrict__ prefix,
    uint64_t* __restrict__ lists, const uint64_t* __restrict__ allow, int nsets, int64_t set_words,
    const int32_t* __restrict__ query_set) {
  using Cd = CountCode<KS>;
  using Eng = Engine<KS, MB>;
  constexpr int C = Cd::C, NPH = Cd::NPH, QPW = 32 * MB;
  __shared__ __attribute__((aligned(16))) uint8_t ring[2 * Cd::TILE];
  __shared__ int32_t Tq[QPW], ltpos[QPW], eqpos[QPW], tq[QPW];

  const int L = linear_block();
  const int chunk = L / nqb;
  const int qb = L - chunk * nqb;
  if (chunk >= nchunks) return;
  const int64_t row0 = (int64_t)chunk * chunk_rows;
  const int64_t row1 = (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  const int nrows = (int)(row1 - row0);
  const int q0 = qb * QPW;

  Eng e(ring, codes, row0, row1);
  const int l = e.l, h = e.h, ri = e.ri;
  // per query: T, the next dist < T position and the next dist == T position of this chunk
  bool any = false;
  for (int i = l; i < QPW; i += 64) {
    const int q = q0 + i;
    int T = 0, lp = 0, ep = 0;
    if (q < nq) {
      const int32_t* pq = prefix + ((int64_t)q * nchunks + chunk) * 4;
      T = tc[2 * q + 0];
      lp = pq[0];
      ep = tc[2 * q + 1] + pq[1];
      if (pq[2] > 0 || (pq[3] > 0 && ep < K)) any = true;
    }
    Tq[i] = T;
    ltpos[i] = lp;
    eqpos[i] = ep;
  }
  if (!__any(any)) return;  // this chunk holds no row of these queries' K-lists (wave-uniform)
  __syncthreads();
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int q = q0 + 32 * m + ri;
    const bool qok = q < nq;
    const int pc = e.load_query(m, queries, q, qok);
    if (h == 0) tq[32 * m + ri] = qok ? Tq[32 * m + ri] + 1 - pc : -0x40000000;  // padded slots never accept
  }
  __syncthreads();
  v16f seed[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int g = 0; g < 16; ++g) seed[m][g] = 0.5f * (float)tq[32 * m + slot_of(g, h)];
  __syncthreads();  // (every plain LDS access is done before the first DMA)
  const uint32_t T0 = lds_addr(Tq), lt0 = lds_addr(ltpos), eq0 = lds_addr(eqpos);
  WaveSets sets;  // lane i: query slot i
  if constexpr (FILTER == FILTER_SETS) sets.init(query_set, q0 + l, l < QPW && q0 + l < nq, nsets, set_words);

  const int ntiles = (nrows + 63) >> 6;
  e.issue(0, 0);
  if (ntiles > 1) e.issue(1, 1);
  for (int i = 0; i < ntiles; ++i) {
    if (i + 1 < ntiles) wait_vm<C>(); else wait_vm<0>();
    v4i rb[2][NPH];
    e.read(i & 1, rb);
    if (i + 2 < ntiles) e.issue(i + 2, i & 1);
    uint64_t word = ~0ull;
    if constexpr (FILTER == FILTER_ONE) {
      word = tile_allow_word(allow, row0, i);
      if (word == 0) continue;  // (wave-uniform, as in the count kernel)
    }
    int idx = 0;
    bool mixed = false;
    if constexpr (FILTER == FILTER_SETS) {
      idx = __builtin_amdgcn_readfirstlane((int)(row0 >> 6) + i);
      mixed = !sets.uniform;
      if (mixed) {  // the OR of the slots' words: the per-row predicate of the pre-test
        word = 0;
#pragma unroll
        for (int sl = 0; sl < QPW; ++sl) word |= sets.word(allow, sl, idx);
      } else {
        word = sets.word(allow, 0, idx);
      }
      if (word == 0) continue;
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const uint32_t half = (uint32_t)(word >> (32 * nb));
      if (FILTER && half == 0) continue;
      if (i * 64 + nb * 32 >= nrows) continue;
      const int local = i * 64 + nb * 32 + ri;
      const bool rlive = local < nrows && ((half >> ri) & 1);
      v16f acc[MB];
      const int prow = e.block(rb[nb], seed, acc);
      const int pc = rlive ? prow : 0x40000000;  // a dead row: no hit
      const float hp = 0.5f * (float)pc;
      static_for<0, MB>([&](auto M) {
        constexpr int m = decltype(M)::value;
        if (!any_above(acc[m], hp)) return;
        // rare: some row of this n-block is in some list of this M-block
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          bool hit = acc[m][g] > hp;
          if (!__ballot(hit)) continue;
          int lo = l;  // lane-dependent values of this rare path from an opaque lane id (no hoisting)
          asm volatile("" : "+v"(lo));
          const int ql = 32 * m + slot_of(g, lo >> 5);
          if (FILTER == FILTER_SETS && mixed) {  // the row's bit of the query's own word
            const uint64_t wlo = sets.word(allow, 32 * m + slot_of(g, 0), idx);
            const uint64_t whi = sets.word(allow, 32 * m + slot_of(g, 1), idx);
            const uint32_t wh = (uint32_t)(((lo >> 5) ? whi : wlo) >> (32 * nb));
            hit = hit && ((wh >> (lo & 31)) & 1);
          }
          // acc = <q, r> + (T + 1 - pc(q)) / 2, so pc(r) - 2 acc = dist - T - 1 in [-(dim + 1), -1]
          const int v = prow - (int)(2.0f * acc[m][g]);
          const bool lt = hit && v < -1, eq = hit && v == -1;
          const uint64_t mlt = __ballot(lt), meq = __ballot(eq);
          const uint32_t hlt = (lo >> 5) ? (uint32_t)(mlt >> 32) : (uint32_t)mlt;
          const uint32_t heq = (lo >> 5) ? (uint32_t)(meq >> 32) : (uint32_t)meq;
          const uint32_t below = (1u << (lo & 31)) - 1u;
          int T = 0, lp = 0, ep = 0;
          lds_read32(T, T0 + (uint32_t)(ql * 4));
          lds_read32(lp, lt0 + (uint32_t)(ql * 4));
          lds_read32(ep, eq0 + (uint32_t)(ql * 4));
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(T), "+v"(lp), "+v"(ep)::"memory");
          if (hit) {
            const int pos = lt ? lp + __popc(hlt & below) : ep + __popc(heq & below);
            if ((uint32_t)pos < (uint32_t)K)
              lists[(int64_t)(q0 + ql) * K + pos] =
                  ((uint64_t)(uint32_t)(v + T + 1) << KEY_ROW_BITS) | (uint64_t)(row0 + local);
          }
          if ((lo & 31) == 0) {  // one lane per half moves its query's positions on
            lds_add32(lt0 + (uint32_t)(ql * 4), __popc(hlt));
            lds_add32(eq0 + (uint32_t)(ql * 4), __popc(heq));
          }
          wait_lgkm0();
        }
      });
    }
  }
}

// ---------------------------------------------------------------------------
// host side: the tables the plan reads and the stages of one pass (the plan and the loop over passes and
// stages are the counting-scan route's, count_route.hip)
// ---------------------------------------------------------------------------
int large_mfma_qreal_of(int cb) { return cb == 256 ? 16 : 32; }
// M-blocks per wave: two where 64 queries' bins and four rings fit the LDS (up to 96 code bytes)
int large_mfma_mb_of(int cb, int qb) { return cb <= 96 && qb > 32 ? 2 : 1; }
int64_t large_mfma_flush_rows() { return kCountFlushRows; }

namespace {

template <int KS, int MB>
int count_launch(const CountPassArgs& a, hipStream_t s) {
  using Cd = CountCode<KS>;
  const int qpw = Cd::QREAL * MB, nqb = (a.nq + qpw - 1) / qpw;
  const dim3 grid((unsigned)(a.nchunks * nqb)), block(64 * Cd::NW);
  return filter_kind(a.filter, [&](auto F) -> int {
    hipLaunchKernelGGL((hamming_count_mfma_kernel<KS, MB, decltype(F)::value>), grid, block, 0, s, a.codes, a.n, a.q,
                       a.nq, a.chunk_rows, a.nchunks, nqb, a.hist, a.filter.allow, a.filter.nsets, a.filter.set_words,
                       a.filter.query_set);
    VRQ_LAUNCH_CHECK();
    return VRQ_OK;
  });
}

template <int KS, int MB>
int emit_launch(const CountPassArgs& a, hipStream_t s) {
  const int qpw = 32 * MB, nqb = (a.nq + qpw - 1) / qpw;
  const dim3 grid((unsigned)(a.nchunks * nqb)), block(64);
  return filter_kind(a.filter, [&](auto F) -> int {
    hipLaunchKernelGGL((hamming_emit_mfma_kernel<KS, MB, decltype(F)::value>), grid, block, 0, s, a.codes, a.n, a.q,
                       a.nq, a.K, a.chunk_rows, a.nchunks, nqb, a.tc, a.prefix, a.lists, a.filter.allow,
                       a.filter.nsets, a.filter.set_words, a.filter.query_set);
    VRQ_LAUNCH_CHECK();
    return VRQ_OK;
  });
}

int stage_launch(int cb, bool emit, const CountPassArgs& a, hipStream_t s) {
  return count_code_bytes(cb, [&](auto CB) -> int {
    constexpr int KS = decltype(CB)::value / 8;
    if (a.mb == 1) return emit ? emit_launch<KS, 1>(a, s) : count_launch<KS, 1>(a, s);
    if constexpr (KS <= 12)
      if (a.mb == 2) return emit ? emit_launch<KS, 2>(a, s) : count_launch<KS, 2>(a, s);
    return VRQ_EUNSUPPORTED;  // (a plan never asks for it)
  });
}

}  // namespace

int large_mfma_count_launch(int cb, const CountPassArgs& a, hipStream_t s) { return stage_launch(cb, false, a, s); }
int large_mfma_emit_launch(int cb, const CountPassArgs& a, hipStream_t s) { return stage_launch(cb, true, a, s); }

// The smallest batch at which AUTO takes K1hm, per code size; INT_MAX: forced only.  One entry serves the
// unfiltered and the filtered scan (it must hold for both), so the plan call needs no filter axis.
// From the A/B against K1h in the same run on the same buffers (tools/batch_bench.py, profiles/batch_bench.jsonl,
// the table in DESIGN section 5 "K1hm"; 1M rows, dims 384 / 1024 / 2048, nq 16 / 64 / 256 / 1024, K 1024 /
// 8192, allowed 1.0 / 0.1): K1hm's median scan time is below K1h's by more than the two legs' spread at every
// measured shape of 1024 and 2048 dims from 16 queries up; at 384 dims it loses at K = 8192 for every batch (its
// emit stage), so it stays forced only there.  The other code sizes were not measured: forced only.
int large_mfma_min_queries(int cb) {
  switch (cb) {
    case 32: return INT_MAX;
    case 48: return INT_MAX;
    case 64: return INT_MAX;
    case 96: return INT_MAX;
    case 128: return 16;
    case 192: return INT_MAX;
    case 256: return 16;
    default: return INT_MAX;
  }
}

}  // namespace vrq
