// hamming_mfma_dim.hip -- K1rd: Phase I on the matrix cores for code sizes other than 128 bytes
// (32, 48, 64, 96, 192, 256 code bytes = embedding dims 256, 384, 512, 768, 1536, 2048).
//
// The scheme of K1r (hamming_mfma.hip), its lean form, with the k-loop length KS = code_bytes / 8 a
// template axis next to MODE (main / sample / re-run) and MB (32-query M-blocks per wave):
//  * each wave owns a contiguous chunk of rows and LDS-DMAs its own packed 64-row tiles (ring of NPR
//    tiles per wave, no workgroup barrier); the queries of its query block are resident as FP4 A
//    fragments in the accumulator file (4 KS MB registers), every 32-bit piece of a row is unpacked
//    straight into the B fragment of one k-step (5 VALU);
//  * dist = pc(q) + pc(r) - 2 <q, r> from the unscaled 32x32x64 FP4 MFMA, exact in f32 (<= 2048); the
//    accumulators start at (tau(q) - pc(q)) / 2, so a row is a hit iff acc > pc(r) / 2: a max3 tree and
//    one compare per M-block; the rare hit path stages dist - tau(q) per wave and appends to the
//    per-(query, chunk) lists, a list overflow marks capc + 1 (exact rescan in the suffix kernel);
//  * batches beyond one wave's 32 MB queries: the grid is chunk groups x query blocks, the query block
//    the fast index inside an XCD (K1d's block remap), so a chunk's re-reads come from that XCD's L2;
//    the corpus is read ceil(nq / (32 MB)) times;
//  * the dense sample pass is the same kernel in MODE = sample: 32 u16 lane minima of
//    dist - pc(q) + dim per (query, sample chunk).
//
// Assignment of a row's dwords to (k-step s, lane half h) -- the same for queries and rows, so every
// dot product is unchanged -- and the LDS image, per code size (C = 16-byte pieces per row):
//  * the tile image is K1d's: piece c of tile row r at 16-byte slot r C + (c + rot(r)) % C, the DMA
//    destination linear and its source address rotated (search_dim.hip); every ds_read_b128 in which
//    the lanes of one half read the same piece index of rows 32 nb + (lane & 31) is conflict-free over
//    its four 16-lane groups (K1d's enumeration: lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
//    are the same row sets here, for either half and either n-block);
//  * C even (32, 64, 96, 192, 256 bytes): half h takes pieces h C/2 .. h C/2 + C/2 - 1, k-step s is
//    dword h KS + s: C/2 whole ds_read_b128 per lane and n-block (96 bytes: 48-byte halves, three);
//  * C = 3 (48 bytes, 24-byte halves): half h takes piece h (k-steps 0..3) and dwords 2h, 2h+1 of piece
//    2 (k-steps 4, 5); both halves read piece 2 whole (an 8-byte read of half a slot at a 16-byte
//    stride is 2-way conflicted whatever the image: the 32 lanes of a ds_read_b64 group would all use
//    the same half of the 64 banks), two ds_read_b128 per lane and n-block.
//
// LDS-read discipline: the packed rows of the next n-block are read in place into the
// registers the k-steps just consumed, all of them are operands of the one wait after the n-block's
// hit test, and no read is in flight across the loop back-edge.
#include <limits.h>

#include "mfma_common.h"
#include "mfma_fp4.h"
#include "mfma_hits.h"
#include "vrq_internal.h"
#include "vrq_scan.h"

namespace vrq {

constexpr int AUX_NT = 2;   // cache policy of the row DMA when each row is read once per batch

template <int KSD>
struct DimCode {
  static constexpr int CB = 8 * KSD;        // code bytes
  static constexpr int DIMB = 64 * KSD;     // code bits
  static constexpr int C = CB / 16;         // 16-byte pieces per row = DMA instructions per tile
  static constexpr int NPH = (C + 1) / 2;   // ds_read_b128 per lane and n-block
  static constexpr int TILE = RT * CB;
  static constexpr int SHIFT = C == 2 ? 3 : C == 4 ? 2 : C == 6 ? 4 : C == 12 ? 2 : C == 16 ? 0 : -1;  // K1d's rot
  static_assert(C == 3 || SHIFT >= 0, "code size");
  __host__ __device__ static constexpr int rot(int r) { return SHIFT < 0 ? 0 : (r >> SHIFT) % C; }
};

template <int KSD, int MB>
struct RowsDimShape {
  using Cd = DimCode<KSD>;
  static constexpr int QPW = 32 * MB;
  static constexpr int NPR = Cd::CB <= 96 ? 3 : 2;  // packed ring depth per wave
  static constexpr int WSMEM = NPR * Cd::TILE + QPW * 8 + (STG + 1) * 4 + MB * 128;
  static constexpr int SMEM = MWAVES * WSMEM;
  // registers: A (4 KS MB, accumulator file) + accumulators and seeds (32 MB) + packed rows, their
  // addresses + ~64: two workgroups per CU (two waves per SIMD) when they fit 256
  static constexpr int REGS = 4 * KSD * MB + 32 * MB + 6 * Cd::NPH + 64;
  static constexpr int OCC = (REGS <= 256 && 2 * (SMEM + Cd::TILE) <= 160 * 1024) ? 2 : 1;
  static_assert(SMEM * OCC <= 160 * 1024, "LDS budget");
  static_assert(2 * Cd::C < 64, "vmcnt range");
};

// retire every LDS read; the N packed-row registers are its operands
template <int N>
__device__ __forceinline__ void wait_rows(v4i (&rb)[N]) {
  static_assert(N == 1 || N == 2 || N == 3 || N == 6 || N == 8, "pieces per lane");
  if constexpr (N == 1)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rb[0])::"memory");
  else if constexpr (N == 2)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rb[0]), "+v"(rb[1])::"memory");
  else if constexpr (N == 3)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rb[0]), "+v"(rb[1]), "+v"(rb[2])::"memory");
  else if constexpr (N == 6)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(rb[0]), "+v"(rb[1]), "+v"(rb[2]), "+v"(rb[3]), "+v"(rb[4]), "+v"(rb[5])::"memory");
  else
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(rb[0]), "+v"(rb[1]), "+v"(rb[2]), "+v"(rb[3]), "+v"(rb[4]), "+v"(rb[5]), "+v"(rb[6]),
                   "+v"(rb[7])::"memory");
}

template <int MODE, int KSD, int MB>
__global__ __launch_bounds__(MWAVES * 64, (RowsDimShape<KSD, MB>::OCC)) void hamming_mfma_rows_dim_kernel(
    const uint8_t* __restrict__ codes, int64_t n, const uint8_t* __restrict__ queries, int nq,
    const int32_t* __restrict__ tau, uint64_t* __restrict__ cand, int32_t* __restrict__ ccnt, int capc,
    int64_t chunk_rows, int64_t chunk_stride, int64_t tile_stride, int nchunks, int nqb,
    const int32_t* __restrict__ rerun, const int32_t* __restrict__ qbflag, uint16_t* __restrict__ dv,
    int64_t dv_stride) {
  constexpr bool DENSE = MODE == MFMA_SAMPLE;
  using Cd = DimCode<KSD>;
  using Sh = RowsDimShape<KSD, MB>;
  constexpr int CB = Cd::CB, C = Cd::C, NPH = Cd::NPH, TILE = Cd::TILE, DIMB = Cd::DIMB;
  constexpr int QPW = Sh::QPW, NPR = Sh::NPR;
  __shared__ __attribute__((aligned(16))) uint8_t smem[Sh::SMEM];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* pk = smem + w * (NPR * TILE);  // this wave's ring
  int32_t* wbase = reinterpret_cast<int32_t*>(smem + MWAVES * NPR * TILE);
  int32_t* lcnt = wbase + w * QPW;                          // this wave's list lengths
  int32_t* tq = wbase + MWAVES * QPW + w * QPW;             // tau'(q) = tau(q) - pc(q)
  int32_t* stg = wbase + 2 * MWAVES * QPW + w * (STG + 1);  // hit staging (+1 spare)
  float* sd = reinterpret_cast<float*>(wbase + 2 * MWAVES * QPW + MWAVES * (STG + 1)) + w * MB * 32;
  const int l = lane_id();
  const int h = l >> 5, ri = l & 31;
  // XCD-aware bijective remap; the query block is the fast index: the blocks of one chunk group run on
  // one XCD and re-read its rows from that XCD's L2
  const int nb = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, slot = b >> 3, q8 = nb >> 3, r8 = nb & 7;
  const int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
  const int cg = L / nqb;
  const int qb = L - cg * nqb;
  if (qbflag && qbflag[qb] == 0) return;  // re-run pass: only query blocks with a failed query
  const int chunk = cg * MWAVES + w;
  if (chunk >= nchunks) return;
  const int64_t row0 = (int64_t)chunk * chunk_stride;
  const bool strided = tile_stride != RT;
  const int64_t row1 = strided ? n : (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  if (row0 >= row1) return;
  const int nrows = strided ? (int)chunk_rows : (int)(row1 - row0);
  const int ntiles = (nrows + RT - 1) / RT;
  const int nblk = 2 * ntiles;  // 32-row n-blocks
  const bool once = nqb == 1;   // every row is read by one wave, once

  // LDS-DMA of packed tile t: instruction gi fills slots gi * 64 + lane; slot p = r C + cs holds piece
  // (cs - rot(r)) mod C of tile row r.  The last partial tile clamps each row to the chunk's last row.
  // The per-lane offsets are recomputed from an opaque lane id at every issue, so that no per-piece
  // 64-bit address stays live across the loop (2 C registers).
  auto issue = [&](int t) __attribute__((always_inline)) {
    int lo_ = l;
    asm volatile("" : "+v"(lo_));
    uint8_t* buf = pk + (t % NPR) * TILE;
    const int64_t tr0 = row0 + (int64_t)t * tile_stride;
    const bool whole = tr0 + RT <= row1;
#pragma unroll
    for (int gi = 0; gi < C; ++gi) {
      const int p = gi * 64 + lo_;
      const int r = p / C, cs = p % C;
      const int c16 = ((cs + C - Cd::rot(r)) % C) * 16;
      int64_t row = tr0 + r;
      if (!whole) row = row < row1 ? row : row1 - 1;
      const uint8_t* src = codes + row * CB + c16;
      uint8_t* dst = buf + gi * 1024;
      if (whole && once)
        __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, AUX_NT);
      else
        __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
  };
  for (int t = 0; t < NPR && t < ntiles; ++t) issue(t);

  // A fragments: k-step s, lane (ri, h) = this half's dword of query qbase + 32 m + ri
  const int qbase = qb * QPW;
  v4i A[MB][KSD];
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int q = qbase + 32 * m + ri;
    const bool qok = q < nq && (!rerun || rerun[q]);
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(queries + (int64_t)(qok ? q : 0) * CB);
    int pc = 0;
#pragma unroll
    for (int s = 0; s < KSD; ++s) {
      const int di = C == 3 ? (s < 4 ? 4 * h + s : 8 + 2 * h + (s - 4)) : h * KSD + s;
      const uint32_t wd = qok ? qp[di] : 0u;
      pc += __popc(wd);
      A[m][s] = unpack_query32(wd);
    }
    pc += __shfl_xor(pc, 32, 64);  // both halves of the query
    if (h == 0) tq[32 * m + ri] = DENSE ? 0 : qok ? tau[q] - pc : -0x40000000;  // padded queries never accept
  }
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int s = 0; s < KSD; ++s) asm volatile("" : "+a"(A[m][s]));
  for (int i = l; i < QPW; i += 64) lcnt[i] = 0;
  // seeds tau'/2: register g of lane half hh holds query (g & 3) + 8 (g >> 2) + 4 hh of the M-block
#pragma unroll
  for (int m = 0; m < MB; ++m)
    if (l < 32) {
      const int g = l & 15, hh = l >> 4;
      sd[m * 32 + l] = 0.5f * (float)tq[32 * m + (g & 3) + 8 * (g >> 2) + 4 * hh];
    }
  const uint32_t sd0 = lds_addr(sd) + (uint32_t)(h * 64), stg0 = lds_addr(stg);
  const uint32_t lc0 = lds_addr(lcnt), pk0 = lds_addr(pk);
  v16f seedv[MB];  // the C operand of every n-block's first MFMA
  if constexpr (!DENSE) {
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      v4i p0, p1, p2, p3;
      lds_read128(p0, sd0 + (uint32_t)(m * 128));
      lds_read128(p1, sd0 + (uint32_t)(m * 128 + 16));
      lds_read128(p2, sd0 + (uint32_t)(m * 128 + 32));
      lds_read128(p3, sd0 + (uint32_t)(m * 128 + 48));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3)::"memory");
      const v16i x = __builtin_shufflevector(__builtin_shufflevector(p0, p1, 0, 1, 2, 3, 4, 5, 6, 7),
                                             __builtin_shufflevector(p2, p3, 0, 1, 2, 3, 4, 5, 6, 7), 0, 1, 2, 3,
                                             4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
      seedv[m] = __builtin_bit_cast(v16f, x);
    }
  }
  // piece j of this lane's half of row 32 nb + ri: its byte offset in a packed tile.  Where rot(r + 32)
  // = rot(r) the second n-block's pieces lie 32 rows further; 96- and 192-byte rows keep both sets.
  constexpr bool SAME_ROT = Cd::SHIFT < 0 || (32 >> Cd::SHIFT) % C == 0;
  uint32_t raddr[SAME_ROT ? 1 : 2][NPH];
#pragma unroll
  for (int nbk = 0; nbk < (SAME_ROT ? 1 : 2); ++nbk)
#pragma unroll
    for (int j = 0; j < NPH; ++j) {
      const int r = 32 * nbk + ri;
      const int c = C == 3 ? (j == 0 ? h : 2) : h * NPH + j;
      raddr[nbk][j] = pk0 + (uint32_t)((r * C + (c + Cd::rot(r)) % C) * 16);
    }
  auto read_piece = [&](v4i& d, auto J, int blk) __attribute__((always_inline)) {
    constexpr int j = decltype(J)::value;
    uint32_t a;
    if constexpr (SAME_ROT)
      a = raddr[0][j] + (uint32_t)((blk & 1) * 32 * C * 16);
    else
      a = (blk & 1) ? raddr[SAME_ROT ? 0 : 1][j] : raddr[0][j];
    lds_read128_inplace(d, a + (uint32_t)(((blk >> 1) % NPR) * TILE));
  };
  // at most k tiles' DMA still in flight
  auto wait_tiles = [&](int k) __attribute__((always_inline)) {
    if (k <= 0) wait_vm<0>();
    else if (k == 1) wait_vm<C>();
    else wait_vm<2 * C>();
  };
  static_assert(NPR - 1 <= 2, "wait_tiles covers up to 2 tiles in flight");
  wait_tiles((ntiles < NPR ? ntiles : NPR) - 1);  // tile 0 landed
  v4i rb[NPH] = {};
  static_for<0, NPH>([&](auto J) { read_piece(rb[decltype(J)::value], J, 0); });
  wait_rows(rb);

  const int64_t qstride = (int64_t)nchunks * capc;
  uint64_t* const cbase = cand + ((int64_t)qbase * nchunks + chunk) * capc;  // + ql * qstride + pos
  // (the hit stage stays in these two lambdas, not HitStage of mfma_hits.h as in K1r: with the shared struct
  // every thresholded instance came out 39-40 instructions shorter and 0.8 % slower at nq = 1024 --
  // DESIGN section 6, profiles/threshold_merge_ab.jsonl)
  int nst = 0;
  auto flush_all = [&](int64_t base_row) __attribute__((always_inline)) {  // staged hits -> lists
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
  };
  auto block_hits = [&](const v16f& a, int m, int pc, float hp) __attribute__((always_inline)) {
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
          // acc = <q,r> + (tau(q) - pc(q)) / 2, so pc(r) - 2 acc = dist - tau(q) in [-(dim + 1), -1]
          const int v = pc - (int)(2.0f * a[g]);
          const int pos = nst + below < STG ? nst + below : STG;
          lds_write32(stg0 + (uint32_t)(pos * 4), ((v + DIMB + 1) << ENT_V_SHIFT) | (ql << ENT_Q_SHIFT) | (lo & 31));
        }
        nst += __popcll(mask);
      }
    }
  };
  DenseMin<DENSE, MB, DIMB> dmin;
  v16f acc[MB];
  for (int blk = 0; blk < nblk; ++blk) {
    // entering the second n-block of tile t: the next n-block's rows come from tile t + 1, which must
    // have landed (the wave's own DMA: no barrier)
    if ((blk & 1) && blk + 1 < nblk) {
      const int t1 = (blk + 1) >> 1;
      const int last = t1 + NPR - 1 < ntiles ? t1 + NPR - 1 : ntiles - 1;  // last tile issued so far
      wait_tiles(last - t1);
    }
    const int nx = blk + 1 < nblk ? blk + 1 : blk;
    int pcs = 0;
    static_for<0, KSD>([&](auto S) {
      constexpr int s = decltype(S)::value;
      uint32_t wd;
      if constexpr (C == 3 && s >= 4)
        wd = (uint32_t)(h ? rb[1][s - 2] : rb[1][s - 4]);
      else
        wd = (uint32_t)rb[s >> 2][s & 3];
      const v4i bfrag = unpack_row32(wd);
      static_for<0, MB>([&](auto M) {
        constexpr int m = decltype(M)::value;
        if constexpr (s == 0 && DENSE)
          acc[m] = mfma_fp4(A[m][s], bfrag, v16f{});
        else if constexpr (s == 0)
          acc[m] = mfma_fp4(A[m][s], bfrag, seedv[m]);
        else
          acc[m] = mfma_fp4(A[m][s], bfrag, acc[m]);
        asm volatile("" : "+v"(acc[m]));
      });
      VRQ_SCHED_FENCE();
      pcs += __popc(wd);
      // the register of k-steps 4j .. 4j+3 takes the next n-block's piece once its last k-step has
      // consumed it (unconditional: the last n-block re-reads its own rows, unused)
      if constexpr ((s & 3) == 3 || s == KSD - 1)
        read_piece(rb[s >> 2], std::integral_constant<int, (s >> 2)>{}, nx);
      VRQ_SCHED_FENCE();
    });
    // epilogue of this n-block (its rows: local lr)
    const auto pp = __builtin_amdgcn_permlane32_swap((uint32_t)pcs, (uint32_t)pcs, false, false);
    const int prow = (int)(pp[0] + pp[1]);  // row popcount (both lane halves)
    const int lr = blk * 32 + ri;
    if constexpr (DENSE) {
      static_for<0, MB>([&](auto M) { dmin.fold(acc[decltype(M)::value], decltype(M)::value, prow, lr < nrows); });
    } else {
      const int pc = lr < nrows ? prow : 0x40000000;  // past the end: no hit
      const float hp = 0.5f * (float)pc;
      const int hpb = __float_as_int(hp);
      uint64_t hitm[MB];
      uint64_t any = 0;
      static_for<0, MB>([&](auto M) {
        constexpr int m = decltype(M)::value;
        const v16i bb = __builtin_bit_cast(v16i, acc[m]);
        const int x0 = max(max(bb[0], bb[1]), bb[2]), x1 = max(max(bb[3], bb[4]), bb[5]);
        const int x2 = max(max(bb[6], bb[7]), bb[8]), x3 = max(max(bb[9], bb[10]), bb[11]);
        const int x4 = max(max(bb[12], bb[13]), bb[14]);
        hitm[m] = __ballot(max(max(max(x0, x1), x2), max(max(x3, x4), bb[15])) > hpb);
        any |= hitm[m];
      });
      if (any) {  // rare
        static_for<0, MB>([&](auto M) {
          constexpr int m = decltype(M)::value;
          if (hitm[m]) block_hits(acc[m], m, pc, hp);
        });
        if (nst) flush_all(row0 + (int64_t)blk * 32);
      }
    }
    wait_rows(rb);  // the next n-block's rows landed (every destination named)
    // after n-block 2t every read from tile t is retired: its ring slot takes the DMA of tile t + NPR
    // (issued before the wait for tile t + 1 at the top of n-block 2t + 1, which counts it)
    if (!(blk & 1) && (blk >> 1) + NPR < ntiles) issue((blk >> 1) + NPR);
  }
  wait_lgkm0();
  if constexpr (DENSE)
    dmin.out(dv, dv_stride, (int64_t)chunk * 32 + ri, qbase, h, nq);
  else
    for (int i = l; i < QPW; i += 64) {
      const int q = qbase + i;
      if (q < nq && (!rerun || rerun[q])) ccnt[(int64_t)q * nchunks + chunk] = lcnt[i];
    }
}

namespace {

// M-blocks per wave of the thresholded pass: the widest instance the batch fills, MB <= 2 at 192 and 256
// bytes (A alone is 96 / 128 registers per M-block there)
constexpr int mb_of(int cb, int nq) { return nq <= 32 ? 1 : (nq <= 64 || cb >= 192) ? 2 : 4; }

template <int KSD, int MB>
constexpr int occ_of() { return RowsDimShape<KSD, MB>::OCC; }
template <int KSD>
constexpr int occ_ks(int mb) {
  if constexpr (KSD >= 24)
    return mb == 1 ? occ_of<KSD, 1>() : occ_of<KSD, 2>();
  else
    return mb == 1 ? occ_of<KSD, 1>() : mb == 2 ? occ_of<KSD, 2>() : occ_of<KSD, 4>();
}
int occ_cb(int cb, int mb) {
  switch (cb) {
    case 32: return occ_ks<4>(mb);
    case 48: return occ_ks<6>(mb);
    case 64: return occ_ks<8>(mb);
    case 96: return occ_ks<12>(mb);
    case 192: return occ_ks<24>(mb);
    default: return occ_ks<32>(mb);
  }
}

struct PassArgs {
  const uint8_t* codes;
  int64_t n;
  const uint8_t* q;
  int nq;
  const int32_t* tau;
  uint64_t* cand;
  int32_t* ccnt;
  int capc;
  int64_t chunk_rows, chunk_stride, tile_stride;
  int nchunks, nqb;
  const int32_t* rerun;
  const int32_t* qbflag;
  uint16_t* dv;
  int64_t dv_stride;
};

template <int MODE, int KSD, int MB>
int launch_pass(const PassArgs& a, hipStream_t s) {
  const dim3 g((unsigned)((a.nchunks + MWAVES - 1) / MWAVES * a.nqb)), blk(MWAVES * 64);
  hipLaunchKernelGGL((hamming_mfma_rows_dim_kernel<MODE, KSD, MB>), g, blk, 0, s, a.codes, a.n, a.q, a.nq, a.tau,
                     a.cand, a.ccnt, a.capc, a.chunk_rows, a.chunk_stride, a.tile_stride, a.nchunks, a.nqb, a.rerun,
                     a.qbflag, a.dv, a.dv_stride);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}
template <int MODE, int KSD>
int launch_mb(const PassArgs& a, int mb, hipStream_t s) {
  if (mb == 1) return launch_pass<MODE, KSD, 1>(a, s);
  if (mb == 2) return launch_pass<MODE, KSD, 2>(a, s);
  // the dense pass and the 192- / 256-byte codes have no MB = 4 instance: a plan never asks for one
  if constexpr (MODE != MFMA_SAMPLE && KSD < 24)
    if (mb == 4) return launch_pass<MODE, KSD, 4>(a, s);
  return VRQ_EUNSUPPORTED;
}
template <int MODE>
int launch_cb(const PassArgs& a, int cb, int mb, hipStream_t s) {
  switch (cb) {
    case 32: return launch_mb<MODE, 4>(a, mb, s);
    case 48: return launch_mb<MODE, 6>(a, mb, s);
    case 64: return launch_mb<MODE, 8>(a, mb, s);
    case 96: return launch_mb<MODE, 12>(a, mb, s);
    case 192: return launch_mb<MODE, 24>(a, mb, s);
    case 256: return launch_mb<MODE, 32>(a, mb, s);
    default: return VRQ_EUNSUPPORTED;
  }
}

}  // namespace

// The smallest batch at which K1rd is the default, per code size, from the A/B against the forced
// wavefront scan in the same run on the same buffers (profiles/dim_mfma_bench.jsonl, the table in DESIGN
// section 5 "K1rd": 10M rows, nq = 1, 8, 64, 128, 1024, Phase I only and full).  K1rd is faster at every
// point of it -- 1.9x to 2.5x at nq = 1, 2.3x to 3.5x at nq = 8, 4.7x to 21x from 64 queries up, against the
// slower of the two yardstick runs, whose spread is at most 5.1 % -- so every code size takes it from one
// query.
int mfma_dim_min_queries(int cb) {
  switch (cb) {
    case 32: return 1;
    case 48: return 1;
    case 64: return 1;
    case 96: return 1;
    case 192: return 1;
    case 256: return 1;
    default: return INT_MAX;
  }
}

int mfma_dim_plan(int64_t n, int cb, int nq, int K, MfmaPlan* p) {
  if (!dim_code_bytes_supported(cb)) return VRQ_EUNSUPPORTED;
  if (nq < 1 || K < 1 || K > kMfmaMaxK || n < RT) return VRQ_EUNSUPPORTED;
  p->rows = 1;
  p->swap = 0;
  p->rows_sample = 1;
  p->mb = mb_of(cb, nq);
  p->qpb = 32 * p->mb;
  p->nqb = (nq + p->qpb - 1) / p->qpb;
  // the dense pass runs min(mb, 2) M-blocks per wave (an MB = 4 instance would spill in its epilogue)
  const int mbs = p->mb < 2 ? p->mb : 2;
  p->nqb_s = (nq + 32 * mbs - 1) / (32 * mbs);
  // sample: as mfma_plan -- S = n / 32 rows clamped to [kMfmaMinSample, kMfmaMaxSample], in 64-row tiles
  // spread evenly over the corpus, one sample chunk per wave of a grid that fills the device once
  int64_t S = n / kMfmaSampleDiv;
  if (S > kMfmaMaxSample) S = kMfmaMaxSample;
  if (S < kMfmaMinSample) S = kMfmaMinSample;
  int64_t tiles = S / RT > 0 ? S / RT : 1;
  if (tiles > n / RT) tiles = n / RT;
  int64_t nsc = 256 * MWAVES * occ_cb(cb, mbs) / p->nqb_s;
  if (nsc < 8) nsc = 8;  // >= 256 lane minima per query (>= 2K)
  if (nsc > tiles) nsc = tiles;
  // T whole tiles per chunk, rounded up and the chunk count reduced to fit (fewer than T tiles of the
  // sample are dropped; rounding T down would drop up to half of them when nsc does not divide tiles)
  int64_t T = (tiles + nsc - 1) / nsc;
  if (tiles / T >= 8 || tiles / T == nsc)
    nsc = tiles / T;
  else
    T = tiles / nsc;
  tiles = nsc * T;
  const int64_t ts = tiles > 1 ? (n - RT) / (tiles - 1) : RT;
  p->sample_chunk_rows = T * RT;
  p->sample_chunks = (int)nsc;
  p->sample_stride = T * ts;
  p->sample_tile_stride = ts;
  p->sample = tiles * RT;
  p->dvcols = nsc * 32;
  // thresholded pass: one chunk per wave, the grid (chunks x query blocks) fills the device once at the
  // instance's occupancy
  int64_t want = 256 * MWAVES * occ_cb(cb, p->mb) / p->nqb;
  if (want < MWAVES) want = MWAVES;
  int64_t cr = (n + want - 1) / want;
  cr = (cr + RT - 1) / RT * RT;
  p->chunk_rows = cr;
  p->nchunks = (int)((n + cr - 1) / cr);
  mfma_plan_lists(p, n, nq, K);
  return VRQ_OK;
}

bool mfma_dim_use(int64_t n, int cb, int nq, int K, int flags) {
  if (!dim_code_bytes_supported(cb) || (flags & VRQ_SEARCH_SCAN_VALU)) return false;
  const bool ok = K <= kMfmaMaxK && n >= kMfmaMinRows;
  if (flags & VRQ_SEARCH_SCAN_MFMA) return ok;
  return ok && nq >= mfma_dim_min_queries(cb);
}

int mfma_dim_scan_launch(const MfmaPlan& p, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                         uint8_t* ws, hipStream_t s, int flags) {
  constexpr int ALL = VRQ_SCAN_STAGE_PREFIX | VRQ_SCAN_STAGE_MATRIX | VRQ_SCAN_STAGE_RECHECK | VRQ_SCAN_STAGE_SUFFIX;
  const int st = (flags & ALL) ? (flags & ALL) : ALL;
  const MfmaWorkspace w(p, ws, nq);
  const bool sampled = p.j < K;
  if (!p.rows || !p.rows_sample) return VRQ_EINVAL;  // not a K1rd plan
  if (st & VRQ_SCAN_STAGE_PREFIX) {  // dense sample pass + per-query thresholds
    const PassArgs a{codes, n, q, nq, nullptr, nullptr, nullptr, 0, p.sample_chunk_rows, p.sample_stride,
                     p.sample_tile_stride, p.sample_chunks, p.nqb_s, nullptr, nullptr, w.dv, p.dvcols};
    const int rc = launch_cb<MFMA_SAMPLE>(a, cb, p.mb < 2 ? p.mb : 2, s);
    if (rc != VRQ_OK) return rc;
    const int rc2 = mfma_sample_select_launch(p, w, q, cb, nq, K, s);
    if (rc2 != VRQ_OK) return rc2;
  }
  if (st & VRQ_SCAN_STAGE_MATRIX) {
    const PassArgs a{codes, n, q, nq, sampled ? w.tau_s : w.tau_p, w.cand, w.ccnt, p.capc, p.chunk_rows, p.chunk_rows,
                     (int64_t)RT, p.nchunks, p.nqb, nullptr, nullptr, nullptr, 0};
    const int rc = launch_cb<MFMA_MAIN>(a, cb, p.mb, s);
    if (rc != VRQ_OK) return rc;
  }
  if ((st & VRQ_SCAN_STAGE_RECHECK) && sampled) {
    // prove C >= K per query; re-run the query blocks holding a failed query with tau_p
    int rc = mfma_sample_check_launch(p, w, nq, K, s);
    if (rc != VRQ_OK) return rc;
    const PassArgs a{codes, n, q, nq, w.tau_p, w.cand, w.ccnt, p.capc, p.chunk_rows, p.chunk_rows,
                     (int64_t)RT, p.nchunks, p.nqb, w.rerun, w.qbflag, nullptr, 0};
    rc = launch_cb<MFMA_RERUN>(a, cb, p.mb, s);
    if (rc != VRQ_OK) return rc;
  }
  // candidates of the whole corpus -> one sorted K-list per query
  if (st & VRQ_SCAN_STAGE_SUFFIX) return mfma_suffix_launch(p, w, codes, n, cb, q, nq, K, s);
  return VRQ_OK;
}

}  // namespace vrq
