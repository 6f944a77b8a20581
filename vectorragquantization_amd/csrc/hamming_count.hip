// hamming_count.hip -- K1h: the counting Phase-I scan for K up to VRQ_K_LARGE_MAX (every code size).
//
// A Hamming distance is an integer in [0, dim], so the exact top-K by (dist asc, row asc) -- FAISS
// IndexBinaryFlat::search order -- is a counting problem with no per-query heap whose size depends on K:
//   count     one workgroup per (chunk of rows, group of queries) keeps an LDS histogram of dim + 1 bins per
//             resident query and writes it to the workspace at [query][chunk][dim + 1];
//   threshold one workgroup per query sums the chunk histograms, finds T with count(dist < T) < K <=
//             count(dist <= T) and c_lt = count(dist < T), and the exclusive prefix over chunks of the
//             dist < T and dist == T counts;
//   emit      the same scan again, one wave per (chunk, 4 queries) walking its chunk in row order: a row below
//             T goes to lt_prefix[chunk] + its rank in the chunk, a row at T to c_lt + eq_prefix[chunk] + its
//             rank while that is below K.  Ranks come from ballot + mbcnt, so every position is
//             deterministic and no global atomic is involved.
// The K-list of a query is then its dist < T rows in row order followed by its first K - c_lt rows at T in
// row order; the large finish (select_rescore.hip) sorts it.
//
// No bound on the counted distances.  Distances of unrelated codes pile up around dim / 2, and an upper bound
// B >= T from the K-th smallest distance of a row prefix (a first small launch of the same two kernels) would
// keep all but about K / prefix of the pairs away from the LDS atomics.  It was built and measured (DESIGN
// 5, K1h; profiles/large_k_bench_bound_ab.jsonl): at 1M rows the bounded count took 0.361 ms against 0.373 ms
// unbounded (1024 dims, 64 queries) and the same 0.012 ms at one query, while the bounding launches cost
// 0.02 - 0.40 ms.  The scan is bound by its distance arithmetic and its loads, not by the atomics, so every
// pair is counted.
//
// Rows stream HBM -> LDS by global_load_lds_dwordx4 into a wave-private two-slot ring with the rotated row
// layout of K1d (search_dim.hip); a tile is copied to registers before its slot is refilled, so two tiles are
// in flight while one is scored.  One row per lane, v_xor_b32 + v_bcnt_u32_b32 against wave-uniform query
// words (scalar loads).  Every loop has a host-fixed trip count; no workgroup waits for another.
#include "row_filter.h"
#include "vrq_internal.h"
#include "vrq_scan.h"
#include "wave_scan.h"

namespace vrq {

__host__ __device__ constexpr int large_rot_shift(int C) {  // (K1d's dim_rot_shift: see search_dim.hip)
  return C == 2 ? 3 : C == 4 ? 2 : C == 6 ? 4 : C == 8 ? 1 : C == 12 ? 2 : C == 16 ? 0 : -1;
}
__host__ __device__ constexpr int large_waves(int CB) { return CB <= 128 ? 4 : 2; }
// resident queries of a count workgroup: 64 KiB of histograms, 16 at the most
__host__ __device__ constexpr int large_qg(int CB) {
  return 65536 / ((CB * 8 + 1) * 4) > 16 ? 16 : 65536 / ((CB * 8 + 1) * 4);
}
constexpr int LARGE_QE = 4;  // queries per wave of the emit kernel

// The wave-private tile ring and the distance of the lane's row, shared by the count and the emit kernel.
template <int CB>
struct TileRing {
  static constexpr int C = CB / 16, W = CB / 4, TILE = 64 * CB, SHIFT = large_rot_shift(C);
  static_assert(CB % 16 == 0 && (C == 3 || SHIFT >= 0) && C < 32, "code size");
  uint8_t* base;  // this wave's two slots
  const uint8_t* codes;
  int64_t row0, row1;  // the chunk's rows
  int l;
  uint32_t raddr[C];

  __device__ __forceinline__ TileRing(uint8_t* b, const uint8_t* c, int64_t r0, int64_t r1)
      : base(b), codes(c), row0(r0), row1(r1), l(lane_id()) {
    const int rot = SHIFT < 0 ? 0 : (l >> SHIFT) % C;
#pragma unroll
    for (int c2 = 0; c2 < C; ++c2) raddr[c2] = lds_addr(base) + (uint32_t)((l * C + (c2 + rot) % C) * 16);
  }
  // tile `tile` of the chunk -> slot `slot` (C wave-instructions on the vm counter)
  __device__ __forceinline__ void issue(int tile, int slot) const {
    uint8_t* buf = base + slot * TILE;
    const int64_t tr0 = row0 + (int64_t)tile * 64;
#pragma unroll
    for (int gi = 0; gi < C; ++gi) {
      const int p = gi * 64 + l;  // LDS piece of the tile
      const int r = p / C, cs = p % C;
      const int rr = SHIFT < 0 ? 0 : (r >> SHIFT) % C;
      const int c = (cs + C - rr) % C;  // the piece that row r reads at slot cs
      int64_t row = tr0 + r;
      row = row < row1 ? row : row1 - 1;  // clamp the ragged last tile (lanes masked by the caller)
      __builtin_amdgcn_global_load_lds(codes + row * CB + c * 16,
                                       (__attribute__((address_space(3))) void*)(buf + gi * 1024), 16, 0, 0);
    }
  }
  // the lane's row of slot `slot` -> registers, retired before return
  __device__ __forceinline__ void read(int slot, v4u (&rv)[C]) const {
    const uint32_t boff = (uint32_t)(slot * TILE);
#pragma unroll
    for (int c = 0; c < C; ++c)
      asm volatile("ds_read_b128 %0, %1" : "=v"(rv[c]) : "v"(raddr[c] + boff) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rv[0]), "+v"(rv[1])::"memory");
#pragma unroll
    for (int c = 2; c < C; ++c) asm volatile("" : "+v"(rv[c]));
  }
  // Hamming distance of the lane's row to query `qi`.  The query words are read through the constant
  // address space at a wave-uniform address, which is what makes them scalar loads: a vector load here
  // would sit on the vm counter among the DMA pieces and drain the ring at every use.
  static __device__ __forceinline__ uint32_t distance(const v4u (&rv)[C], const uint8_t* queries, int qi) {
    typedef const __attribute__((address_space(4))) uint32_t* const_u32_ptr;
    const const_u32_ptr qp = (const_u32_ptr)(uintptr_t)(queries + (int64_t)qi * CB);
    uint32_t a0 = 0, a1 = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      xor_bcnt(a0, qp[4 * c + 0], rv[c].x);
      xor_bcnt(a1, qp[4 * c + 1], rv[c].y);
      xor_bcnt(a0, qp[4 * c + 2], rv[c].z);
      xor_bcnt(a1, qp[4 * c + 3], rv[c].w);
    }
    return a0 + a1;
  }
};

// XCD-aware, bijective block -> linear id, as K1 / K1d: the blocks of one XCD take the same chunk for
// successive query groups, so a chunk that several groups scan is re-read from that XCD's L2
__device__ __forceinline__ int xcd_linear_block() {
  const int nb = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, slot = b >> 3, q8 = nb >> 3, r8 = nb & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// The filtered instances (FILTER; vrq_*_filtered): `allow` holds one bit per row, bit r & 63 of the u64 word
// r >> 6.  Chunks start at multiples of 64 rows, so the filter of a 64-row tile is the one aligned word
// (row0 >> 6) + tile: a wave-uniform address, read like the query words through the constant address space
// (the bitmap is read-only for the kernel's lifetime).  That makes it a scalar load on the lgkm counter; a
// vector load would join the ring's DMA pieces on the vm counter and break the wait_vmcnt<C> accounting.
// A disallowed row is a dead lane of both passes, exactly like a row past the ragged last tile.  `allow` is
// the last kernel argument and the threshold's minimum is compiled into the filtered instance only, so the
// unfiltered count and emit instances are, instruction for instruction, what they were without the FILTER axis
// (the threshold's differs in the LDS offsets of its arrays alone).
//
// The per-query instances (FILTER_SETS; vrq_*_perquery, row_filter.h): every resident query has its own word of
// the tile, at its set's base + (row0 >> 6) + tile, still a scalar load at a wave-uniform address for the reason
// above.  The set ids are read once at kernel entry and kept as wave-uniform offsets; `live` is the row's bit
// of the query's own word, and a query whose word is zero skips its distance on a wave-uniform branch -- when
// that holds for every resident query the tile does nothing, but its loads were issued and waited for as in
// every other instance, so the ring's trip counts and wait counts are those of the unfiltered kernel.  When all
// real queries of the workgroup name one set (a batch sorted by set), a wave-uniform test at entry takes the
// single-word path with that set's word.  nsets, set_words and query_set follow `allow` as the last arguments.
__device__ __forceinline__ uint64_t allow_word(const uint64_t* allow, int64_t row0, int tile) {
  typedef const __attribute__((address_space(4))) uint64_t* const_u64_ptr;
  const int idx = __builtin_amdgcn_readfirstlane((int)(row0 >> 6) + tile);  // n < 2^32: below 2^26
  return ((const_u64_ptr)(uintptr_t)allow)[idx];
}

// ---- count: histogram of the distances per (query, chunk) over rows [0, n) ----
template <int CB, int FILTER>
__global__ __launch_bounds__(64 * large_waves(CB)) void hamming_count_kernel(
    const uint8_t* __restrict__ codes, int64_t n, const uint8_t* __restrict__ queries, int nq, int64_t chunk_rows,
    int nchunks, int nqg, uint32_t* __restrict__ hist_out, const uint64_t* __restrict__ allow, int nsets,
    int64_t set_words, const int32_t* __restrict__ query_set) {
  using Ring = TileRing<CB>;
  constexpr int C = Ring::C, NW = large_waves(CB), QG = large_qg(CB), BINS = CB * 8 + 1;
  __shared__ __attribute__((aligned(16))) uint8_t ring[NW * 2 * Ring::TILE];
  __shared__ uint32_t hist[QG * BINS];

  const int L = xcd_linear_block();
  const int chunk = L / nqg;
  const int qg = L - chunk * nqg;
  if (chunk >= nchunks) return;
  const int64_t row0 = (int64_t)chunk * chunk_rows;
  const int64_t row1 = (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  const int nrows = (int)(row1 - row0);
  const int tid = threadIdx.x, l = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int q0 = qg * QG;
  const int nqa = nq - q0 < QG ? nq - q0 : QG;

  for (int i = tid; i < nqa * BINS; i += 64 * NW) hist[i] = 0;
  __syncthreads();  // (no DMA in flight yet)

  // per-query sets: the bitmap offset of every resident query and its two flags (bit j of sall / snone)
  int64_t soff[FILTER == FILTER_SETS ? QG : 1];
  uint32_t sall = 0, snone = 0;
  bool uniform = true;
  if constexpr (FILTER == FILTER_SETS) {
    const int sid0 = set_id_uniform(query_set, q0);
#pragma unroll
    for (int j = 0; j < QG; ++j) {
      const bool real = j < nqa;
      const int sid = set_id_uniform(query_set, q0 + (real ? j : 0));
      const SetRef r = set_ref(sid, real, nsets, set_words);
      soff[j] = r.off;
      sall |= (uint32_t)r.all << j;
      snone |= (uint32_t)r.none << j;
      uniform = uniform && (!real || sid == sid0);
    }
  }

  // this wave's tiles: w, w + NW, ...
  const int ntiles = (nrows + 63) >> 6;
  const int ntw = w < ntiles ? (ntiles - w + NW - 1) / NW : 0;
  Ring tr(ring + w * 2 * Ring::TILE, codes, row0, row1);
  if (ntw > 0) tr.issue(w, 0);
  if (ntw > 1) tr.issue(w + NW, 1);
  for (int i = 0; i < ntw; ++i) {
    if (i + 1 < ntw) wait_vmcnt<C>(); else wait_vmcnt<0>();
    v4u rv[C];
    tr.read(i & 1, rv);
    if (i + 2 < ntw) tr.issue(w + (i + 2) * NW, i & 1);  // (the slot's reads are retired)
    bool live = (w + i * NW) * 64 + l < nrows;
    if constexpr (FILTER == FILTER_SETS) {
      const int idx = __builtin_amdgcn_readfirstlane((int)(row0 >> 6) + w + i * NW);
      if (!uniform) {  // mixed sets: a word per resident query (slots past nqa are `none`: word 0)
#pragma unroll
        for (int j = 0; j < QG; ++j) {
          const uint64_t wj = set_word(allow, soff[j], (sall >> j) & 1, (snone >> j) & 1, idx);
          if (wj == 0) continue;  // no allowed row of this query in the tile (wave-uniform)
          const uint32_t d = Ring::distance(rv, queries, q0 + j);
          if (live && ((wj >> l) & 1)) atomicAdd(&hist[j * BINS + d], 1u);
        }
        continue;
      }
      const uint64_t word = set_word(allow, soff[0], sall & 1, snone & 1, idx);
      if (word == 0) continue;
      live = live && ((word >> l) & 1);
    }
    if constexpr (FILTER == FILTER_ONE) {
      const uint64_t word = allow_word(allow, row0, w + i * NW);
      if (word == 0) continue;  // no allowed row in this tile (wave-uniform; its loads were issued and waited)
      live = live && ((word >> l) & 1);
    }
    for (int j = 0; j < nqa; ++j) {
      const uint32_t d = Ring::distance(rv, queries, q0 + j);
      if (live) atomicAdd(&hist[j * BINS + d], 1u);
    }
  }
  __syncthreads();  // (every DMA of this wave is retired)
  for (int i = tid; i < nqa * BINS; i += 64 * NW) {
    const int j = i / BINS, b = i - j * BINS;
    hist_out[((int64_t)(q0 + j) * nchunks + chunk) * BINS + b] = hist[i];
  }
}

// ---- threshold: one workgroup per query ----
constexpr int THR_THREADS = 1024;

// exclusive scan of one int per thread over the workgroup (LDS scratch of THR_THREADS ints); total in *tot
__device__ inline int thr_excl_scan(int v, int* tot, int32_t* scratch) {
  const int tid = threadIdx.x;
  __syncthreads();
  scratch[tid] = v;
  __syncthreads();
  for (int o = 1; o < THR_THREADS; o <<= 1) {
    const int y = tid >= o ? scratch[tid - o] : 0;
    __syncthreads();
    scratch[tid] += y;
    __syncthreads();
  }
  const int incl = scratch[tid];
  *tot = scratch[THR_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// hist u32 [nq][nchunks][bins].  want = min(K, n); a filtered scan (FILTER) lowers it to the total of the
// histograms, the number of allowed rows (an unfiltered scan's total is n).  Writes tc[q] = (T, c_lt), prefix[q][chunk] = (lt prefix,
// eq prefix, lt count, eq count) and the KEY_NONE padding of the K-list past `want`.
template <bool FILTER>
__global__ __launch_bounds__(THR_THREADS) void large_threshold_kernel(const uint32_t* __restrict__ hist, int nchunks,
                                                                      int bins, int want, int K,
                                                                      int32_t* __restrict__ tc,
                                                                      int32_t* __restrict__ prefix,
                                                                      uint64_t* __restrict__ lists) {
  constexpr int MAXBINS = 2049, SLICES = THR_THREADS / 256;
  __shared__ uint32_t tot[MAXBINS];
  __shared__ int32_t scratch[THR_THREADS];
  __shared__ int32_t ltc[kLargeMaxChunks], eqc[kLargeMaxChunks];
  __shared__ int32_t misc[2];
  const int q = blockIdx.x, tid = threadIdx.x;
  const uint32_t* hq = hist + (int64_t)q * nchunks * bins;
  for (int b = tid; b < bins; b += THR_THREADS) tot[b] = 0;
  if (tid == 0) {
    misc[0] = bins - 1;
    misc[1] = 0;
  }
  __syncthreads();
  // the sum over chunks of every bin: 256 threads across the bins (coalesced), SLICES slices of the chunks
  for (int b = tid % 256; b < bins; b += 256) {
    uint32_t s = 0;
    for (int c = tid / 256; c < nchunks; c += SLICES) s += hq[(int64_t)c * bins + b];
    if (s) atomicAdd(&tot[b], s);
  }
  __syncthreads();
  const int BPT = (bins + THR_THREADS - 1) / THR_THREADS;
  int local = 0;
  for (int b = 0; b < BPT; ++b) {
    const int i = tid * BPT + b;
    if (i < bins) local += (int)tot[i];
  }
  int all;
  int cum = thr_excl_scan(local, &all, scratch);
  if constexpr (FILTER) {
    if ((uint32_t)all < (uint32_t)want) want = all;  // fewer allowed rows than K
  }
  for (int b = 0; b < BPT; ++b) {
    const int i = tid * BPT + b;
    if (i >= bins) break;
    const int h = (int)tot[i];
    if (cum < want && cum + h >= want) {
      misc[0] = i;    // T
      misc[1] = cum;  // c_lt
    }
    cum += h;
  }
  __syncthreads();
  const int T = misc[0], c_lt = misc[1];
  if (tid == 0) {
    tc[2 * q + 0] = T;
    tc[2 * q + 1] = c_lt;
  }
  // per chunk: rows below T and rows at T (one wave per chunk)
  const int l = lane_id(), w = tid / WAVE;
  for (int c = w; c < nchunks; c += THR_THREADS / WAVE) {
    const uint32_t* hc = hq + (int64_t)c * bins;
    int s = 0;
    for (int b = l; b < T; b += WAVE) s += (int)hc[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
    if (l == 0) {
      ltc[c] = s;
      eqc[c] = (int)hc[T];
    }
  }
  __syncthreads();
  const int CPT = (nchunks + THR_THREADS - 1) / THR_THREADS;
  int sl = 0, se = 0;
  for (int b = 0; b < CPT; ++b) {
    const int c = tid * CPT + b;
    if (c < nchunks) {
      sl += ltc[c];
      se += eqc[c];
    }
  }
  int tl, te;
  int pl = thr_excl_scan(sl, &tl, scratch);
  int pe = thr_excl_scan(se, &te, scratch);
  int32_t* pq = prefix + (int64_t)q * nchunks * 4;
  for (int b = 0; b < CPT; ++b) {
    const int c = tid * CPT + b;
    if (c < nchunks) {
      pq[4 * c + 0] = pl;
      pq[4 * c + 1] = pe;
      pq[4 * c + 2] = ltc[c];
      pq[4 * c + 3] = eqc[c];
      pl += ltc[c];
      pe += eqc[c];
    }
  }
  for (int i = want + tid; i < K; i += THR_THREADS) lists[(int64_t)q * K + i] = KEY_NONE;
}

// ---- emit: one wave per (chunk, LARGE_QE queries), rows in order ----
template <int CB, int FILTER>
__global__ __launch_bounds__(64) void hamming_emit_kernel(const uint8_t* __restrict__ codes, int64_t n,
                                                          const uint8_t* __restrict__ queries, int nq, int K,
                                                          int64_t chunk_rows, int nchunks, int nqg,
                                                          const int32_t* __restrict__ tc,
                                                          const int32_t* __restrict__ prefix,
                                                          uint64_t* __restrict__ lists,
                                                          const uint64_t* __restrict__ allow, int nsets,
                                                          int64_t set_words,
                                                          const int32_t* __restrict__ query_set) {
  using Ring = TileRing<CB>;
  constexpr int C = Ring::C, QE = LARGE_QE;
  __shared__ __attribute__((aligned(16))) uint8_t ring[2 * Ring::TILE];

  const int L = xcd_linear_block();
  const int chunk = L / nqg;
  const int qg = L - chunk * nqg;
  if (chunk >= nchunks) return;
  const int64_t row0 = (int64_t)chunk * chunk_rows;
  const int64_t row1 = (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  const int nrows = (int)(row1 - row0);
  const int l = lane_id();
  const int q0 = qg * QE;
  const int nqa = nq - q0 < QE ? nq - q0 : QE;

  // per query: T, the next dist < T position and the next dist == T position of this chunk
  int32_t T[QE], ltpos[QE], eqpos[QE];
  bool any = false;
#pragma unroll
  for (int j = 0; j < QE; ++j) {
    const int q = q0 + (j < nqa ? j : 0);
    const int32_t* pq = prefix + ((int64_t)q * nchunks + chunk) * 4;
    T[j] = __builtin_amdgcn_readfirstlane(tc[2 * q + 0]);
    const int c_lt = __builtin_amdgcn_readfirstlane(tc[2 * q + 1]);
    ltpos[j] = __builtin_amdgcn_readfirstlane(pq[0]);
    eqpos[j] = c_lt + __builtin_amdgcn_readfirstlane(pq[1]);
    const int nlt = __builtin_amdgcn_readfirstlane(pq[2]), neq = __builtin_amdgcn_readfirstlane(pq[3]);
    if (j < nqa && (nlt > 0 || (neq > 0 && eqpos[j] < K))) any = true;
  }
  if (!any) return;  // this chunk holds no row of these queries' K-lists (wave-uniform)

  // per-query sets, as in the count kernel
  int64_t soff[QE];
  uint32_t sall = 0, snone = 0;
  bool uniform = true;
  if constexpr (FILTER == FILTER_SETS) {
    const int sid0 = set_id_uniform(query_set, q0);
#pragma unroll
    for (int j = 0; j < QE; ++j) {
      const bool real = j < nqa;
      const int sid = set_id_uniform(query_set, q0 + (real ? j : 0));
      const SetRef r = set_ref(sid, real, nsets, set_words);
      soff[j] = r.off;
      sall |= (uint32_t)r.all << j;
      snone |= (uint32_t)r.none << j;
      uniform = uniform && (!real || sid == sid0);
    }
  }

  const int ntiles = (nrows + 63) >> 6;
  Ring tr(ring, codes, row0, row1);
  tr.issue(0, 0);
  if (ntiles > 1) tr.issue(1, 1);
  for (int i = 0; i < ntiles; ++i) {
    if (i + 1 < ntiles) wait_vmcnt<C>(); else wait_vmcnt<0>();
    v4u rv[C];
    tr.read(i & 1, rv);
    if (i + 2 < ntiles) tr.issue(i + 2, i & 1);
    const int local = i * 64 + l;
    const bool inrows = local < nrows;
    bool live = inrows;
    uint64_t wq[QE];  // FILTER_SETS: the tile's word of every query (all-ones bits elsewhere)
#pragma unroll
    for (int j = 0; j < QE; ++j) wq[j] = ~0ull;
    if constexpr (FILTER == FILTER_SETS) {
      const int idx = __builtin_amdgcn_readfirstlane((int)(row0 >> 6) + i);
      uint64_t any_word = 0;
#pragma unroll
      for (int j = 0; j < QE; ++j) {
        const int js = uniform ? 0 : j;
        wq[j] = set_word(allow, soff[js], (sall >> js) & 1, (snone >> js) & 1, idx);
        any_word |= wq[j];
      }
      if (any_word == 0) continue;  // (wave-uniform: slots past nqa are `none`, or copies of slot 0)
    }
    if constexpr (FILTER == FILTER_ONE) {
      const uint64_t word = allow_word(allow, row0, i);
      if (word == 0) continue;  // (wave-uniform, as in the count kernel)
      live = live && ((word >> l) & 1);
    }
#pragma unroll
    for (int j = 0; j < QE; ++j) {
      if (j < nqa) {
        if constexpr (FILTER == FILTER_SETS) {
          if (wq[j] == 0) continue;  // no allowed row of this query in the tile (wave-uniform)
          live = inrows && ((wq[j] >> l) & 1);
        }
        const int32_t d = (int32_t)Ring::distance(rv, queries, q0 + j);
        const bool lt = live && d < T[j], eq = live && d == T[j];
        const uint64_t mlt = __ballot(lt), meq = __ballot(eq);
        if (mlt | meq) {
          const uint64_t key = ((uint64_t)(uint32_t)d << KEY_ROW_BITS) | (uint64_t)(row0 + local);
          uint64_t* o = lists + (int64_t)(q0 + j) * K;
          if (lt) {
            const int pos = ltpos[j] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mlt >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)mlt, 0u));
            if ((uint32_t)pos < (uint32_t)K) o[pos] = key;
          }
          if (eq) {
            const int pos = eqpos[j] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(meq >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)meq, 0u));
            if ((uint32_t)pos < (uint32_t)K) o[pos] = key;
          }
          ltpos[j] += __popcll(mlt);
          eqpos[j] += __popcll(meq);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host side: the tables the plan reads and the stages of one pass (the plan and the loop over passes and
// stages are the counting-scan route's, count_route.hip)
// ---------------------------------------------------------------------------
int large_qg_of(int cb) {
  return count_code_bytes(cb, [](auto CB) -> int { return large_qg(decltype(CB)::value); });
}

int large_waves_of(int cb) { return large_waves(cb); }

int large_count_launch(int cb, const CountPassArgs& a, hipStream_t s) {
  return count_code_bytes(cb, [&](auto CBc) -> int {
    constexpr int CB = decltype(CBc)::value;
    const int nqg = (a.nq + large_qg(CB) - 1) / large_qg(CB);
    const dim3 grid((unsigned)(a.nchunks * nqg)), block(64 * large_waves(CB));
    return filter_kind(a.filter, [&](auto F) -> int {
      hipLaunchKernelGGL((hamming_count_kernel<CB, decltype(F)::value>), grid, block, 0, s, a.codes, a.n, a.q, a.nq,
                         a.chunk_rows, a.nchunks, nqg, a.hist, a.filter.allow, a.filter.nsets, a.filter.set_words,
                         a.filter.query_set);
      VRQ_LAUNCH_CHECK();
      return VRQ_OK;
    });
  });
}

int large_emit_launch(int cb, const CountPassArgs& a, hipStream_t s) {
  return count_code_bytes(cb, [&](auto CBc) -> int {
    constexpr int CB = decltype(CBc)::value;
    const int nqg = (a.nq + LARGE_QE - 1) / LARGE_QE;
    const dim3 grid((unsigned)(a.nchunks * nqg)), block(64);
    return filter_kind(a.filter, [&](auto F) -> int {
      hipLaunchKernelGGL((hamming_emit_kernel<CB, decltype(F)::value>), grid, block, 0, s, a.codes, a.n, a.q, a.nq,
                         a.K, a.chunk_rows, a.nchunks, nqg, a.tc, a.prefix, a.lists, a.filter.allow, a.filter.nsets,
                         a.filter.set_words, a.filter.query_set);
      VRQ_LAUNCH_CHECK();
      return VRQ_OK;
    });
  });
}

int large_threshold_launch(const uint32_t* hist, int nq, int nchunks, int bins, int want, int K, bool filtered,
                           int32_t* tc, int32_t* prefix, uint64_t* lists, hipStream_t s) {
  if (filtered)
    hipLaunchKernelGGL(large_threshold_kernel<true>, dim3(nq), dim3(THR_THREADS), 0, s, hist, nchunks, bins, want,
                       K, tc, prefix, lists);
  else
    hipLaunchKernelGGL(large_threshold_kernel<false>, dim3(nq), dim3(THR_THREADS), 0, s, hist, nchunks, bins, want,
                       K, tc, prefix, lists);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

}  // namespace vrq
