// search_dim.hip -- K1d: the Phase-I exhaustive Hamming scan for code sizes other than 128 bytes
// (embedding dims 256, 384, 512, 768, 1536, 2048 = 32, 48, 64, 96, 192, 256 code bytes).
//
// Same contract as K1 (hamming_scan.hip): FAISS IndexBinaryFlat::search order (dist asc, row asc); a wave
// scans one contiguous chunk of rows and emits the exact top-K of its chunk as dist << 40 | row keys in
// the [nq][nchunks][K] layout that K2's exact merge takes.  Same machinery: rows stream HBM -> LDS by
// global_load_lds_dwordx4, one row per lane, v_xor_b32 + v_bcnt_u32_b32 against wave-uniform query words,
// ballot-compacted 32-bit keys (dist << 20 | chunk row) under the running K-th key, wave bitonic cut.
//
// What differs from K1:
//  * one wave per workgroup with a wave-private 3-slot LDS ring, so no workgroup barrier: the wave's own
//    vmcnt covers its DMA pieces, and a slot is refilled only after the wave retired its reads of it.
//    (A 64-row tile is CB/16 = 2, 3, 4, 6, 12 or 16 DMA instructions; 3 and 6 do not split over 4 or 8
//    waves.)  Blocks of one XCD take the same chunk for successive query groups, so a chunk that several
//    query groups scan is re-read from that XCD's L2.
//  * two queries per wave up to 96 code bytes, one at 192 and 256: a 2048-bit query is 64 SGPRs and two
//    of them exceed the 102 a wave has.
//  * LDS layout per width.  ds_read_b128 serves four 16-lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}
//    and the same + 32), a group is conflict-free iff its lanes' 16-byte slots differ mod 16.  Lane l
//    reads piece c of its row at slot l*C + (c + rot(l)) % C, the DMA source address is pre-rotated the
//    same way (linear LDS destination):
//        C = 3  (48 B):  rot = 0       -- the odd stride is conflict-free as it is
//        C = 2  (32 B):  rot = l >> 3      C = 4  (64 B):  rot = l >> 2
//        C = 6  (96 B):  rot = l >> 4      C = 12 (192 B): rot = l >> 2      C = 16 (256 B): rot = l
//    Unrotated, 96-byte rows are 2-way and 192-byte rows 4-way conflicted; each rot above leaves every
//    group of every piece index on 16 distinct slots (enumerated over the four lane groups).
//  * dist <= 2048 = 2^11: the largest key (2048 << 20 | 0xfffff) stays below the all-ones sentinel.
#include "vrq_internal.h"
#include "vrq_scan.h"
#include "wave_scan.h"

namespace vrq {

__host__ __device__ constexpr int dim_rot_shift(int C) {
  return C == 2 ? 3 : C == 4 ? 2 : C == 6 ? 4 : C == 12 ? 2 : C == 16 ? 0 : -1;
}

template <int CB, int CAP>
__global__ __launch_bounds__(64) void hamming_scan_dim_kernel(const uint8_t* __restrict__ codes, int64_t n,
                                                              const uint8_t* __restrict__ queries, int nq, int K,
                                                              int64_t chunk_rows, int nchunks, int nqg,
                                                              uint64_t* __restrict__ out) {
  constexpr int C = CB / 16;         // 16-byte pieces per row = LDS-DMA wave-instructions per 64-row tile
  constexpr int W = CB / 4;          // dwords per code
  constexpr int QG = CB <= 96 ? 2 : 1;
  constexpr int TILE = 64 * CB;
  constexpr int NBUF = 3;
  constexpr int SHIFT = dim_rot_shift(C);
  static_assert(CB % 16 == 0 && (C == 3 || SHIFT >= 0), "code size");
  static_assert(CAP % WAVE == 0 && 2 * C < 64, "cap / vmcnt range");
  __shared__ __attribute__((aligned(16))) uint8_t smem[NBUF * TILE + QG * CAP * 4];
  uint32_t* cand = reinterpret_cast<uint32_t*>(smem + NBUF * TILE);

  // XCD-aware, bijective block -> linear id, as K1
  const int nb = gridDim.x, b = blockIdx.x;
  const int xcd = b & 7, slot = b >> 3, q8 = nb >> 3, r8 = nb & 7;
  const int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
  const int chunk = L / nqg;
  const int qg = L - chunk * nqg;
  if (chunk >= nchunks) return;
  const int64_t row0 = (int64_t)chunk * chunk_rows;
  const int64_t row1 = (row0 + chunk_rows < n) ? row0 + chunk_rows : n;
  const int nrows = (int)(row1 - row0);
  const int l = lane_id();
  const int qw0 = qg * QG;  // first query of this wave (< nq: nqg = ceil(nq / QG))
  const int nqa = nq - qw0 < QG ? nq - qw0 : QG;

  // query words: wave-uniform loads (scalar cache -> SGPRs); an absent second query re-reads the first
  uint32_t qw[QG][W];
#pragma unroll
  for (int j = 0; j < QG; ++j) {
    const uint32_t* qp =
        reinterpret_cast<const uint32_t*>(uniform_ptr(queries + (int64_t)(qw0 + (j < nqa ? j : 0)) * CB));
#pragma unroll
    for (int i = 0; i < W; ++i) qw[j][i] = __builtin_amdgcn_readfirstlane(qp[i]);  // pinned to an SGPR
  }

  int cnt[QG];
  uint32_t tau[QG];
#pragma unroll
  for (int j = 0; j < QG; ++j) {
    cnt[j] = 0;
    tau[j] = 0xffffffffu;
  }

  const int rot = SHIFT < 0 ? 0 : (l >> SHIFT) % C;
  uint32_t raddr[C];  // this lane's row pieces in slot 0 of the ring
#pragma unroll
  for (int c = 0; c < C; ++c) raddr[c] = lds_addr(smem) + (uint32_t)((l * C + (c + rot) % C) * 16);

  const int ntiles = (nrows + 63) >> 6;
  auto issue = [&](int t) __attribute__((always_inline)) {
    uint8_t* buf = smem + (t % NBUF) * TILE;
    const int64_t tr0 = row0 + (int64_t)t * 64;
#pragma unroll
    for (int gi = 0; gi < C; ++gi) {
      const int p = gi * 64 + l;  // LDS slot of the tile
      const int r = p / C, cs = p % C;
      const int rr = SHIFT < 0 ? 0 : (r >> SHIFT) % C;
      const int c = (cs + C - rr) % C;  // the piece that row r reads at slot cs
      int64_t row = tr0 + r;
      row = row < row1 ? row : row1 - 1;  // clamp the ragged last tile (lanes masked below)
      __builtin_amdgcn_global_load_lds(codes + row * CB + c * 16,
                                       (__attribute__((address_space(3))) void*)(buf + gi * 1024), 16, 0, 0);
    }
  };
  auto read_tile = [&](int t, v4u (&rv)[C]) __attribute__((always_inline)) {
    const uint32_t boff = (uint32_t)((t % NBUF) * TILE);
#pragma unroll
    for (int c = 0; c < C; ++c)
      asm volatile("ds_read_b128 %0, %1" : "=v"(rv[c]) : "v"(raddr[c] + boff) : "memory");
  };
  // retire the tile's reads; every piece is re-defined after the wait, so no use can move above it
  auto wait_tile = [&](v4u (&rv)[C]) __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rv[0]), "+v"(rv[1])::"memory");
#pragma unroll
    for (int c = 2; c < C; ++c) asm volatile("" : "+v"(rv[c]));
  };
  auto distances = [&](const v4u (&rv)[C], uint32_t& da, uint32_t& db) __attribute__((always_inline)) {
    uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      xor_bcnt(a0, qw[0][4 * c + 0], rv[c].x);
      if (QG == 2) xor_bcnt(b0, qw[QG - 1][4 * c + 0], rv[c].x);
      xor_bcnt(a1, qw[0][4 * c + 1], rv[c].y);
      if (QG == 2) xor_bcnt(b1, qw[QG - 1][4 * c + 1], rv[c].y);
      xor_bcnt(a0, qw[0][4 * c + 2], rv[c].z);
      if (QG == 2) xor_bcnt(b0, qw[QG - 1][4 * c + 2], rv[c].z);
      xor_bcnt(a1, qw[0][4 * c + 3], rv[c].w);
      if (QG == 2) xor_bcnt(b1, qw[QG - 1][4 * c + 3], rv[c].w);
    }
    da = a0 + a1;
    db = b0 + b1;
  };
  auto accept = [&](int j, uint32_t key) __attribute__((always_inline)) {
    bool acc = key < tau[j];
    uint64_t mask = __ballot(acc);
    if (mask) {
      int nnew = __popcll(mask);
      uint32_t* cj = cand + j * CAP;
      if (cnt[j] + nnew > CAP) {
        wave_sort_keys<CAP>(cj, cnt[j]);
        cnt[j] = cnt[j] < K ? cnt[j] : K;
        if (cnt[j] >= K) tau[j] = __builtin_amdgcn_readfirstlane(cj[K - 1]);
        acc = key < tau[j];
        mask = __ballot(acc);
        nnew = __popcll(mask);
      }
      if (acc) {
        const int pos = cnt[j] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        cj[pos] = key;
      }
      cnt[j] += nnew;
    }
  };
  auto score_tile = [&](int t, const v4u (&rv)[C]) __attribute__((always_inline)) {
    const int local = t * 64 + l;
    uint32_t da, db;
    distances(rv, da, db);
    accept(0, local < nrows ? ((da << LOCAL_BITS) | (uint32_t)local) : 0xffffffffu);
    if (QG == 2 && nqa > 1) accept(QG - 1, local < nrows ? ((db << LOCAL_BITS) | (uint32_t)local) : 0xffffffffu);
  };

  // Software pipeline over the 3-slot ring: while tile t is scored from VGPRs (set A), tile t+1 is read
  // LDS -> VGPRs (set B) and tiles t+2, t+3 are in flight HBM -> LDS; tile t+3 goes to tile t's slot, whose
  // reads this wave retired at the end of the previous step.  (As in K1, the next tile's LDS reads are
  // issued and retired on every path, the last step's included, where they read a stale slot nothing uses.)
  for (int t = 0; t < 3 && t < ntiles; ++t) issue(t);
  if (ntiles > 2)
    wait_vmcnt<2 * C>();
  else if (ntiles > 1)
    wait_vmcnt<C>();
  else
    wait_vmcnt<0>();
  v4u rA[C], rB[C];
  read_tile(0, rA);
  wait_tile(rA);
  for (int t = 0; t < ntiles; t += 2) {
    if (t + 1 < ntiles) {
      if (t + 2 < ntiles) wait_vmcnt<C>(); else wait_vmcnt<0>();
    }
    read_tile(t + 1, rB);
    if (t + 3 < ntiles) issue(t + 3);
    score_tile(t, rA);
    wait_tile(rB);
    if (t + 1 >= ntiles) break;
    if (t + 2 < ntiles) {
      if (t + 3 < ntiles) wait_vmcnt<C>(); else wait_vmcnt<0>();
    }
    read_tile(t + 2, rA);
    if (t + 4 < ntiles) issue(t + 4);
    score_tile(t + 1, rB);
    wait_tile(rA);
  }

  // chunk done: exact top-K per query -> global keys (dist << 40 | shard row), padded.
#pragma unroll
  for (int j = 0; j < QG; ++j) {
    if (j >= nqa) break;
    uint32_t* cj = cand + j * CAP;
    wave_sort_keys<CAP>(cj, cnt[j]);
    const int m = cnt[j] < K ? cnt[j] : K;
    uint64_t* o = out + ((int64_t)(qw0 + j) * nchunks + chunk) * K;
    for (int i = l; i < K; i += WAVE) {
      uint64_t gk = KEY_NONE;
      if (i < m) {
        const uint32_t key = cj[i];
        gk = ((uint64_t)(key >> LOCAL_BITS) << KEY_ROW_BITS) | (uint64_t)(row0 + (key & LOCAL_MASK));
      }
      o[i] = gk;
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool dim_code_bytes_supported(int cb) {
  return cb == 32 || cb == 48 || cb == 64 || cb == 96 || cb == 192 || cb == 256;
}

int dim_scan_queries_per_wave(int cb) { return cb <= 96 ? 2 : 1; }

template <int CB, int CAP>
static int launch_t(const ScanPlan& p, const uint8_t* codes, int64_t n, const uint8_t* q, int nq, int K,
                    uint64_t* lists, hipStream_t s) {
  hipLaunchKernelGGL((hamming_scan_dim_kernel<CB, CAP>), dim3(p.nchunks * p.nqg), dim3(64), 0, s, codes, n, q, nq, K,
                     p.chunk_rows, p.nchunks, p.nqg, lists);
  VRQ_LAUNCH_CHECK();
  return VRQ_OK;
}

template <int CB>
static int launch_c(const ScanPlan& p, const uint8_t* codes, int64_t n, const uint8_t* q, int nq, int K,
                    uint64_t* lists, hipStream_t s) {
  switch (p.cap) {
    case 256: return launch_t<CB, 256>(p, codes, n, q, nq, K, lists, s);
    case 512: return launch_t<CB, 512>(p, codes, n, q, nq, K, lists, s);
    case 1024: return launch_t<CB, 1024>(p, codes, n, q, nq, K, lists, s);
    case 2048: return launch_t<CB, 2048>(p, codes, n, q, nq, K, lists, s);
    default: return VRQ_EUNSUPPORTED;
  }
}

int dim_scan_launch(const ScanPlan& p, const uint8_t* codes, int64_t n, int cb, const uint8_t* q, int nq, int K,
                    uint64_t* lists, hipStream_t s) {
  if (p.wpg != 1 || p.qg != dim_scan_queries_per_wave(cb)) return VRQ_EINVAL;  // not a K1d plan
  switch (cb) {
    case 32: return launch_c<32>(p, codes, n, q, nq, K, lists, s);
    case 48: return launch_c<48>(p, codes, n, q, nq, K, lists, s);
    case 64: return launch_c<64>(p, codes, n, q, nq, K, lists, s);
    case 96: return launch_c<96>(p, codes, n, q, nq, K, lists, s);
    case 192: return launch_c<192>(p, codes, n, q, nq, K, lists, s);
    case 256: return launch_c<256>(p, codes, n, q, nq, K, lists, s);
    default: return VRQ_EUNSUPPORTED;
  }
}

}  // namespace vrq
