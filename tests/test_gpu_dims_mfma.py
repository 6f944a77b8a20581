"""GPU checks of K1rd, the matrix-core Phase-I scan at the embedding dims other than 1024
(hamming_mfma_dim.hip): FAISS IndexBinaryFlat semantics (CohereEnhancedVectorDB.py:267-268 -- dist
ascending, then row ascending, strict-< admission), bit for bit.

* every entry of every per-(query, chunk) candidate list after PREFIX + MATRIX + RECHECK, and every list
  against the exact set of rows it must hold (true distances from an exact fp32 GEMM of the bit matrices);
* every u16 lane minimum of the dense sample pass;
* the top-K against the C restatement of hammings_knn_hc and against the forced wavefront scan;
* the exact-fallback paths at 384 bits (odd k-step count, 48-byte rows) and 2048 bits (the widest);
* the full three-phase search and the Python classes.

n = 300 007 (ragged; one wave's chunk is 2-5 tiles, so the DMA ring wraps and the last tile is partial);
there the sample is 65 536 rows and K = 100 gives a sampled order j < K, so the tau_s path is live.
"""
import numpy as np
import pytest
import torch

from tests.conftest import oracle_knn
from tests.test_gpu_lists import KEY_ROW_BITS, _al, _bits, _dist

pytestmark = pytest.mark.gpu

DIMS = (256, 384, 512, 768, 1536, 2048)
N = 300_007
INT_MAX = 2**31 - 1
# the documented default table (DESIGN section 5 "K1rd"; tests/test_dims_mfma_capi.py pins it on the host)
MIN_QUERIES = {256: 1, 384: 1, 512: 1, 768: 1, 1536: 1, 2048: 1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    return torch.device("cuda", 0)


def _nat():
    from vectorragquantization_amd import _native
    return _native


_CORPUS = {}


def _corpus(d, nq, dev, n=N):
    """Uniform random codes (one corpus per dim, shared) and nq queries: corpus rows with d/16 .. d/4 bits
    flipped, every seventh one uniform random (far from everything)."""
    from vectorragquantization_amd import synth
    if (d, n) not in _CORPUS:
        _CORPUS[(d, n)] = synth.random_codes(n, d // 8, device=dev, seed=500 + d)
    codes = _CORPUS[(d, n)]
    qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4), seed=600 + d + nq)
    g = torch.Generator(device=dev)
    g.manual_seed(700 + d + nq)
    qb[::7] = torch.randint(0, 256, qb[::7].shape, generator=g, device=dev, dtype=torch.uint8)
    return codes, qb


def _plan(n, d, nq, K, flags=None):
    Nn = _nat()
    info = np.zeros(12, np.int64)
    Nn.check(Nn.load().vrq_scan_plan(n, d, nq, K, Nn.VRQ_SEARCH_SCAN_MFMA if flags is None else flags,
                                     info.ctypes.data), "plan")
    return info


def _mb(d, nq):
    return 1 if nq <= 32 else 2 if nq <= 64 or d >= 1536 else 4


def _scan_stages(codes, qb, d, K, stages):
    Nn = _nat()
    lib = Nn.load()
    n, nq = codes.shape[0], qb.shape[0]
    flags = Nn.VRQ_SEARCH_PHASE1_ONLY | Nn.VRQ_SEARCH_SCAN_MFMA
    info = _plan(n, d, nq, K)
    ws = torch.zeros((int(info[11]),), dtype=torch.uint8, device=codes.device)
    st = Nn.stream_handle(codes.device)
    for stage in stages:
        Nn.check(lib.vrq_search3_dim_scan(Nn.ptr(codes), n, d, Nn.ptr(qb), nq, K, flags | stage, Nn.ptr(ws),
                                          ws.numel(), st), "scan stage")
    torch.cuda.synchronize()
    return info, ws


def _workspace_views(info, ws, nq):
    nch, capc, off_cand, off_cnt, off_tau = (int(info[i]) for i in (3, 4, 5, 6, 7))
    cnt = ws[off_cnt:off_cnt + 4 * nq * nch].view(torch.int32).view(nq, nch)
    cand = ws[off_cand:off_cand + 8 * nq * nch * capc].view(torch.int64).view(nq, nch, capc)
    qa = _al(4 * nq)
    tau_s = ws[off_tau:off_tau + 4 * nq].view(torch.int32).long()
    tau_p = ws[off_tau + qa:off_tau + qa + 4 * nq].view(torch.int32).long()
    rerun = ws[off_tau + 2 * qa:off_tau + 2 * qa + 4 * nq].view(torch.int32)
    return cnt, cand, tau_s, tau_p, rerun


# ----------------------------------------------------------------------------- 1. every list entry
@pytest.mark.parametrize("nq", (1, 40, 128, 129, 300))
@pytest.mark.parametrize("d", DIMS)
def test_candidate_lists_exact(dev, d, nq):
    """After PREFIX + MATRIX + RECHECK every (query, chunk) list holds exactly the rows of its chunk with
    dist < tau(q), each once, with the true distance in the key; no list overflows on uniform data.

    nq -> instance (MB = M-blocks per wave; query blocks of 32 MB queries), asserted through info[0:2]:
      1: MB 1;  40: MB 2;  128: MB 4, one block (1536 / 2048 bits: MB 2, two blocks);
      129: MB 4, a second block of one query (MB 2: three blocks, the third of one query);
      300: MB 4, three blocks, the third ragged (MB 2: five blocks, the fifth of 44 queries).
    Together they reach every compiled (code size, MB) instance in main mode."""
    K = 100
    codes, qb = _corpus(d, nq, dev)
    n = codes.shape[0]
    Nn = _nat()
    info, ws = _scan_stages(codes, qb, d, K, (Nn.VRQ_SCAN_STAGE_PREFIX, Nn.VRQ_SCAN_STAGE_MATRIX,
                                              Nn.VRQ_SCAN_STAGE_RECHECK))
    assert (int(info[0]), int(info[1])) == (3, _mb(d, nq))
    cr, nch, capc, j = (int(info[i]) for i in (2, 3, 4, 9))
    assert j < K, "the sampled threshold must be live at this size"
    cnt, cand, tau_s, tau_p, rerun = _workspace_views(info, ws, nq)
    tau = torch.where(rerun != 0, tau_p, tau_s)
    assert (cnt >= 0).all(), "negative list length"
    assert not (cnt > capc).any(), "a list overflowed on uniform data"
    D = _dist(codes, qb)
    live = torch.arange(capc, device=dev)[None, None, :] < cnt[:, :, None]
    qs = torch.arange(nq, device=dev)[:, None, None].expand(nq, nch, capc)[live]
    chs = torch.arange(nch, device=dev)[None, :, None].expand(nq, nch, capc)[live]
    keys = cand[live]
    rows = keys & ((1 << KEY_ROW_BITS) - 1)
    assert ((rows >= chs * cr) & (rows < torch.clamp(chs * cr + cr, max=n))).all(), "row outside its chunk"
    d_gpu = (keys >> KEY_ROW_BITS) - (d + 1) + tau[qs]
    d_true = D[qs, rows].long()
    bad = torch.nonzero(d_gpu != d_true).flatten()
    assert bad.numel() == 0, (f"{bad.numel()} of {keys.numel()} listed distances wrong; first: q {int(qs[bad[0]])} "
                              f"row {int(rows[bad[0]])} gpu {int(d_gpu[bad[0]])} true {int(d_true[bad[0]])}")
    assert (d_true < tau[qs]).all()
    listed = torch.sort(qs * n + rows).values
    tq, tr = torch.nonzero(D < tau[:, None].to(torch.int16), as_tuple=True)
    want = tq * n + tr
    assert torch.equal(listed, want), f"{listed.numel()} listed vs {want.numel()} rows below the thresholds"
    assert (cnt.sum(1) >= K).all(), "tau_s admitted fewer than K rows and the query did not re-run"


# ----------------------------------------------------------------------------- 2. dense sample pass
@pytest.mark.parametrize("nq", (8, 128, 300))
@pytest.mark.parametrize("d", DIMS)
def test_sample_lane_minima_exact(dev, d, nq):
    """Every u16 lane minimum equals min(dist - pc(q)) + dim over the sample rows that lane holds."""
    Nn = _nat()
    K = 100
    codes, qb = _corpus(d, nq, dev)
    n = codes.shape[0]
    sp = np.zeros(6, np.int64)
    Nn.check(Nn.load().vrq_scan_sample_plan(n, d, nq, K, Nn.VRQ_SEARCH_SCAN_MFMA, sp.ctypes.data), "sample plan")
    rows_sample, nsc, scr, sstride, ts, cols = (int(x) for x in sp)
    assert rows_sample == 1 and sstride == (scr // 64) * ts and cols == 32 * nsc
    _, ws = _scan_stages(codes, qb, d, K, (Nn.VRQ_SCAN_STAGE_PREFIX,))
    dv = ws[:2 * nq * cols].view(torch.int16).view(nq, cols).int() & 0xFFFF
    T = scr // 64
    srows = (torch.arange(nsc * T, device=dev)[:, None] * ts + torch.arange(64, device=dev)[None, :]).reshape(-1)
    assert int(srows.max()) < n
    D = _dist(codes[srows], qb)
    pcq = _bits(qb).sum(1).int()
    want = D.view(nq, nsc, T, 2, 32).amin(dim=(2, 3)).int() - pcq[:, None, None] + d
    assert torch.equal(dv, want.view(nq, cols))


# ----------------------------------------------------------------------------- 3. top-K
def _phase1(codes, qb, d, K, flags, row_offset=0):
    """vrq_search3_dim_scan + vrq_search3_dim_finish, Phase I only -> (count, dist, rows) as numpy."""
    Nn = _nat()
    lib = Nn.load()
    dev_ = codes.device
    n, nq = codes.shape[0], qb.shape[0]
    flags |= Nn.VRQ_SEARCH_PHASE1_ONLY
    ws = torch.empty((max(8, lib.vrq_search3_dim_workspace_size(n, d, nq, K)),), dtype=torch.uint8, device=dev_)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev_)
    rows = torch.empty((nq, K), dtype=torch.int64, device=dev_)
    dist = torch.empty((nq, K), dtype=torch.int32, device=dev_)
    st = Nn.stream_handle(dev_)
    Nn.check(lib.vrq_search3_dim_scan(Nn.ptr(codes), n, d, Nn.ptr(qb), nq, K, flags, Nn.ptr(ws), ws.numel(), st),
             "scan")
    Nn.check(lib.vrq_search3_dim_finish(Nn.ptr(codes), 0, 0, 0, n, d, row_offset, 0, nq, K, K, K, flags, Nn.ptr(cnt),
                                        Nn.ptr(rows), Nn.ptr(dist), 0, 0, Nn.ptr(ws), ws.numel(), st), "finish")
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), dist.cpu().numpy(), rows.cpu().numpy()


def _hamming_topk(codes, qb, K, row_offset):
    Nn = _nat()
    lib = Nn.load()
    n, cb, nq = codes.shape[0], codes.shape[1], qb.shape[0]
    ws = torch.empty((max(8, lib.vrq_hamming_topk_workspace_size(n, cb, nq, K)),), dtype=torch.uint8,
                     device=codes.device)
    rows = torch.empty((nq, K), dtype=torch.int64, device=codes.device)
    dist = torch.empty((nq, K), dtype=torch.int32, device=codes.device)
    Nn.check(lib.vrq_hamming_topk(Nn.ptr(codes), n, cb, row_offset, Nn.ptr(qb), nq, K, Nn.ptr(dist), Nn.ptr(rows),
                                  Nn.ptr(ws), ws.numel(), Nn.stream_handle(codes.device)), "hamming_topk")
    torch.cuda.synchronize()
    return dist.cpu().numpy(), rows.cpu().numpy()


_ORACLE = {}


@pytest.mark.parametrize("nq", (1, 64, 300))
@pytest.mark.parametrize("d", DIMS)
def test_topk_vs_faiss_restatement(dev, oracle_lib, d, nq):
    """Rows and distances of the forced matrix-core scan equal the C restatement (one reference per
    (dim, batch) at K = 128; its prefixes are the smaller K's) and the forced wavefront scan, bit for bit;
    vrq_hamming_topk (whichever scan it chooses by shape) returns the same."""
    Nn = _nat()
    codes, qb = _corpus(d, nq, dev)
    off = 7_000_000_000
    assert Nn.load().vrq_scan_kind(N, d, nq, 128, Nn.VRQ_SEARCH_SCAN_MFMA, None) == Nn.VRQ_SCAN_KIND_MFMA
    if (d, nq) not in _ORACLE:
        _ORACLE[(d, nq)] = oracle_knn(oracle_lib, codes.cpu().numpy(), qb.cpu().numpy(), 128, threads=16)
    D0, I0 = _ORACLE[(d, nq)]
    for K in (1, 100, 128):
        c, D1, I1 = _phase1(codes, qb, d, K, Nn.VRQ_SEARCH_SCAN_MFMA, off)
        assert np.array_equal(c, np.full(nq, K))
        assert np.array_equal(D1, D0[:, :K]) and np.array_equal(I1, I0[:, :K] + off)
        cv, Dv, Iv = _phase1(codes, qb, d, K, Nn.VRQ_SEARCH_SCAN_VALU, off)
        assert np.array_equal(cv, c) and np.array_equal(Dv, D1) and np.array_equal(Iv, I1)
        Dh, Ih = _hamming_topk(codes, qb, K, off)
        assert np.array_equal(Dh, D1) and np.array_equal(Ih, I1)


# ----------------------------------------------------------------------------- 4. edge paths
EDGE_DIMS = (384, 2048)
NQ_EDGE = 140   # 384 bits: MB 4, a second query block of 12; 2048 bits: MB 2, three blocks


def _paths(codes_t, qb_t, d, K):
    """Which fallback paths a query took (PREFIX + MATRIX + RECHECK, read from the workspace):
    -> (some list overflowed [nq], re-ran with tau_p [nq])."""
    Nn = _nat()
    info, ws = _scan_stages(codes_t, qb_t, d, K, (Nn.VRQ_SCAN_STAGE_PREFIX, Nn.VRQ_SCAN_STAGE_MATRIX,
                                                  Nn.VRQ_SCAN_STAGE_RECHECK))
    cnt, _, _, _, rerun = _workspace_views(info, ws, qb_t.shape[0])
    return (cnt > int(info[4])).any(dim=1).cpu().numpy(), (rerun != 0).cpu().numpy()


def _flip(rng, rows, nflip, lo=0, hi=None):
    """Copies of `rows` (u8[m, cb]) with exactly nflip distinct bits in [lo, hi) flipped each."""
    m, cb = rows.shape
    hi = cb * 8 if hi is None else hi
    out = np.empty((m, cb), np.uint8)
    out[...] = rows
    pos = lo + rng.integers(0, hi - lo, (m, nflip))
    while nflip > 1:                                     # distinct positions per row
        bad = (np.diff(np.sort(pos, axis=1), axis=1) == 0).any(axis=1)
        if not bad.any():
            break
        pos[bad] = lo + rng.integers(0, hi - lo, (int(bad.sum()), nflip))
    flat = out.reshape(-1)
    base = np.arange(m, dtype=np.int64) * cb
    for c in range(nflip):                               # one position per row per step: unique indices
        flat[base + (pos[:, c] >> 3)] ^= (0x80 >> (pos[:, c] & 7)).astype(np.uint8)
    return out


def _check(oracle_lib, codes, qb, K, dist, rows, row_offset=0):
    D0, I0 = oracle_knn(oracle_lib, codes, qb, K, threads=16)
    assert np.array_equal(D0, dist)
    assert np.array_equal(I0 + row_offset, rows)
    return D0, I0


def _run_edge(oracle_lib, dev, d, codes, qb, K, row_offset=0):
    """The forced matrix-core scan against the C restatement, every query."""
    Nn = _nat()
    codes_t, qb_t = torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev)
    c, D1, I1 = _phase1(codes_t, qb_t, d, K, Nn.VRQ_SEARCH_SCAN_MFMA, row_offset)
    assert np.array_equal(c, np.full(qb.shape[0], K))
    _check(oracle_lib, codes, qb, K, D1, I1, row_offset)
    return D1, I1


@pytest.mark.parametrize("d", EDGE_DIMS)
def test_heavy_ties(dev, oracle_lib, d):
    """Every row is one of 25 codes, stored in runs of 700 equal rows (a run covers whole chunks, so the
    chunks of a query's nearest code hold more hits than a list does -- with the codes scattered row by
    row a chunk of this corpus would hold ~13): every query has overflowed lists and is rescanned exactly,
    and the K-list is the first rows of each distance in row order (plus a row offset)."""
    rng = np.random.default_rng(11 + d)
    cb = d // 8
    base = rng.integers(0, 256, (25, cb), dtype=np.uint8)
    codes = np.repeat(base[rng.integers(0, 25, N // 700 + 1)], 700, axis=0)[:N]
    qb = np.concatenate([base[:4], _flip(rng, base[4:8], 40), rng.integers(0, 256, (NQ_EDGE - 8, cb), dtype=np.uint8)])
    ovf, _ = _paths(torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev), d, 100)
    assert ovf.all(), "every query's lists must overflow on an all-ties corpus"
    for K in (1, 100, 128):
        _run_edge(oracle_lib, dev, d, codes, qb, K, row_offset=5_000_000)


@pytest.mark.parametrize("d", EDGE_DIMS)
def test_candidate_overflow_exact_rescan(dev, oracle_lib, d):
    """40 000 rows at distance exactly 3 from query 0 (50 of them exact copies): far more rows beat its
    threshold than its lists hold, so the corpus is rescanned exactly and the answer is the 50 copies plus
    the FIRST 50 dist-3 rows in row order.  Queries 2 and 135 (a later query block) repeat query 0 (a row
    of the region itself sees too few rows below its sampled threshold to overflow a list at this size)."""
    rng = np.random.default_rng(9 + d)
    cb, K, R0, R = d // 8, 100, 130_000, 40_000
    codes = rng.integers(0, 256, (N, cb), dtype=np.uint8)
    qb = rng.integers(0, 256, (NQ_EDGE, cb), dtype=np.uint8)
    region = _flip(rng, np.broadcast_to(qb[:1], (R, cb)), 3)
    region[rng.choice(R, 50, replace=False)] = qb[0]
    codes[R0:R0 + R] = region
    qb[2] = qb[0]
    qb[135] = qb[0]
    ovf, _ = _paths(torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev), d, K)
    assert ovf[[0, 2, 135]].all() and not ovf[[1, 3]].any()
    D1, _ = _run_edge(oracle_lib, dev, d, codes, qb, K)
    assert (D1[0] == 0).sum() == 50 and (D1[0] == 3).sum() == 50


@pytest.mark.parametrize("d", EDGE_DIMS)
def test_hit_staging_overflow(dev, oracle_lib, d):
    """A 30 000-row region clustered around one code (6 bits of its first half flipped), every query of the
    first query block near it (4 bits of the second half flipped: exactly 10 bits from every row of the
    region, so each of its 32-row blocks gives that wave 32 x its queries hits, more than the 512 entries
    its LDS stage holds) and six such queries in a later query block: their lists are marked overflowed and
    rescanned exactly while the other queries keep the fast path."""
    rng = np.random.default_rng(17 + d)
    cb, K, R0, R = d // 8, 100, 200_000, 30_000
    qpb = 32 * _mb(d, NQ_EDGE)
    base = rng.integers(0, 256, (1, cb), dtype=np.uint8)
    codes = rng.integers(0, 256, (N, cb), dtype=np.uint8)
    codes[R0:R0 + R] = _flip(rng, np.broadcast_to(base, (R, cb)), 6, 0, d // 2)
    qb = rng.integers(0, 256, (NQ_EDGE, cb), dtype=np.uint8)
    planted = np.concatenate([np.arange(qpb), np.arange(NQ_EDGE - 8, NQ_EDGE - 2)])
    qb[planted] = _flip(rng, np.broadcast_to(base, (planted.size, cb)), 4, d // 2, d)
    ovf, _ = _paths(torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev), d, K)
    assert ovf[planted].all() and ovf.sum() <= planted.size + 8
    _, I1 = _run_edge(oracle_lib, dev, d, codes, qb, K)
    assert (I1[planted] >= R0).all() and (I1[planted] < R0 + R).all()


def _sample_rows(n, d, nq, K):
    Nn = _nat()
    info = np.zeros(8, np.int64)
    Nn.check(Nn.load().vrq_scan_sample_plan(n, d, nq, K, Nn.VRQ_SEARCH_SCAN_MFMA, info.ctypes.data), "sample plan")
    chunks, crows, ts = int(info[1]), int(info[2]), int(info[4])
    tiles = chunks * (crows // 64)
    return (np.arange(tiles, dtype=np.int64)[:, None] * ts + np.arange(64)[None, :]).reshape(-1)


@pytest.mark.parametrize("d", EDGE_DIMS)
def test_sampled_threshold_rerun(dev, oracle_lib, d):
    """Queries 0 and 135 (the first and a later query block) get 70 near copies on sample rows and 40 more
    at dist 30 off the sample: tau_s = d'_(j) + 1 falls among the near copies, the check finds fewer than
    K admitted rows, and the query block's re-run with tau_p must recover the first 30 dist-30 rows in row
    order."""
    rng = np.random.default_rng(23 + d)
    cb, K, nq = d // 8, 100, NQ_EDGE
    info = _plan(N, d, nq, K)
    assert int(info[9]) < K, "the plan must take the sampled threshold"
    codes = rng.integers(0, 256, (N, cb), dtype=np.uint8)
    qb = _flip(rng, codes[rng.integers(0, N, nq)], 50)
    samp = _sample_rows(N, d, nq, K)
    assert samp.max() < N and np.unique(samp).size == samp.size
    insamp = np.zeros(N, bool)
    insamp[samp] = True
    planted = [0, 135]
    near_all = rng.choice(samp, 140, replace=False)
    far_all = rng.integers(0, N, 400)
    far_all = rng.permutation(np.unique(far_all[~insamp[far_all]]))[:80]
    assert far_all.size == 80
    for i, q in enumerate(planted):
        near = near_all[70 * i:70 * (i + 1)]
        codes[near] = _flip(rng, np.repeat(qb[q:q + 1], 70, axis=0), int(rng.integers(5, 21)))
        far = far_all[40 * i:40 * (i + 1)]
        codes[far] = _flip(rng, np.repeat(qb[q:q + 1], 40, axis=0), 30)
    _, rerun = _paths(torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev), d, K)
    assert rerun[planted].all(), "the planted queries must fail tau_s and re-run with tau_p"
    D1, _ = _run_edge(oracle_lib, dev, d, codes, qb, K)
    assert (D1[0] == 30).sum() == 30 and (D1[135] == 30).sum() == 30


@pytest.mark.parametrize("d", EDGE_DIMS)
def test_cluster_ordered_corpus(dev, oracle_lib, d):
    """300 clusters of 1000 contiguous near-copies: a query's whole neighbourhood sits in few chunks and in
    few lane rows of the sample (looser thresholds).  The result must still be exactly the FAISS order."""
    rng = np.random.default_rng(4242 + d)
    cb, ncl, per = d // 8, 300, 1000
    centres = rng.integers(0, 256, (ncl, cb), dtype=np.uint8)
    codes = np.empty((N, cb), np.uint8)
    m = ncl * per
    codes[:m] = np.repeat(centres, per, axis=0)
    codes[m:] = rng.integers(0, 256, (N - m, cb), dtype=np.uint8)
    flips = rng.integers(0, 256, (m, cb), dtype=np.uint8)
    for _ in range(3):                                    # bit density 1/16
        flips &= rng.integers(0, 256, (m, cb), dtype=np.uint8)
    codes[:m] ^= flips
    qb = _flip(rng, centres[rng.integers(0, ncl, NQ_EDGE)], 12)
    _run_edge(oracle_lib, dev, d, codes, qb, 100)


@pytest.mark.parametrize("d", (1536, 2048))
def test_distances_above_1027(dev, oracle_lib, d):
    """Every row is >= 1028 bits from every query: nothing may fall off a 1 028-bin histogram (sample
    selection, suffix merge, exact rescan and the finish's merge all size theirs by the dim)."""
    rng = np.random.default_rng(31 + d)
    cb, n, nq = d // 8, 70_001, 70
    base = rng.integers(0, 256, (1, cb), dtype=np.uint8)
    codes = _flip(rng, np.broadcast_to(base, (n, cb)), 1)
    extra = rng.integers(0, 256, (n, cb), dtype=np.uint8)
    for _ in range(3):
        extra &= rng.integers(0, 256, (n, cb), dtype=np.uint8)
    codes ^= extra                                        # ~ d/16 + 1 bits from base
    qb = _flip(rng, np.broadcast_to(~base, (nq, cb)), 20)
    codes[5000:5300] = codes[5000]                        # 300 identical rows: ties beyond a list's capacity
    D1, _ = _run_edge(oracle_lib, dev, d, codes, qb, 100)
    assert D1.min() >= 1028


# ----------------------------------------------------------------------------- 5. full three-phase
@pytest.mark.parametrize("d", (384, 1536, 2048))
def test_three_phase_equals_wavefront_scan(dev, oracle_lib, d):
    """n = 70 001 (just above the row minimum), k / oversamples 10 / 10 / 3: all five outputs with the matrix
    scan (the default choice where the measured table takes it for this batch, and forced through the
    stage-able pair) equal those of the forced wavefront scan bit for bit; Phase I equals the oracle's."""
    from vectorragquantization_amd import synth
    from vectorragquantization_amd.enhanced import search3
    from vectorragquantization_amd.quant import int8_row_norms
    Nn = _nat()
    lib = Nn.load()
    n, k, K, K3 = 70_001, 10, 100, 30
    nq = 48 if MIN_QUERIES[d] == INT_MAX else max(48, MIN_QUERIES[d])
    g = torch.Generator(device=dev)
    g.manual_seed(900 + d)
    codes = synth.random_codes(n, d // 8, device=dev, seed=800 + d)
    qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 8), seed=801 + d)
    x8 = torch.randint(-127, 128, (n, d), generator=g, device=dev, dtype=torch.int8)
    x8[4242] = 0                                          # zero norm -> -inf cosine
    norms = int8_row_norms(x8)
    qf = (torch.round(torch.randn((nq, d), generator=g, device=dev) * 4096) / 65536).float()
    assert lib.vrq_scan_kind(n, d, nq, K, Nn.VRQ_SEARCH_SCAN_MFMA, None) == Nn.VRQ_SCAN_KIND_MFMA
    default_is_matrix = lib.vrq_scan_kind(n, d, nq, K, 0, None) == Nn.VRQ_SCAN_KIND_MFMA
    assert default_is_matrix == (nq >= MIN_QUERIES[d])
    ref = [o.cpu().numpy() for o in search3(codes, x8, norms, qf, qb, k, K, K3, Nn.VRQ_SEARCH_SCAN_VALU)]
    dflt = [o.cpu().numpy() for o in search3(codes, x8, norms, qf, qb, k, K, K3, 0)]
    # forced through the stage-able pair
    ws = torch.empty((lib.vrq_search3_dim_workspace_size(n, d, nq, K),), dtype=torch.uint8, device=dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, k), dtype=torch.int64, device=dev)
    dist = torch.empty((nq, k), dtype=torch.int32, device=dev)
    s2 = torch.empty((nq, k), dtype=torch.float64, device=dev)
    s3 = torch.empty((nq, k), dtype=torch.float64, device=dev)
    st, fl = Nn.stream_handle(dev), Nn.VRQ_SEARCH_SCAN_MFMA
    Nn.check(lib.vrq_search3_dim_scan(Nn.ptr(codes), n, d, Nn.ptr(qb), nq, K, fl, Nn.ptr(ws), ws.numel(), st), "scan")
    Nn.check(lib.vrq_search3_dim_finish(Nn.ptr(codes), Nn.ptr(x8), Nn.ptr(norms), 0, n, d, 0, Nn.ptr(qf), nq, k, K, K3,
                                        fl, Nn.ptr(cnt), Nn.ptr(rows), Nn.ptr(dist), Nn.ptr(s2), Nn.ptr(s3),
                                        Nn.ptr(ws), ws.numel(), st), "finish")
    torch.cuda.synchronize()
    forced = [o.cpu().numpy() for o in (cnt, rows, dist, s2, s3)]
    for a, b, c in zip(ref, dflt, forced):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
    c1, D1, I1 = _phase1(codes, qb, d, K, Nn.VRQ_SEARCH_SCAN_MFMA)
    assert np.array_equal(c1, np.full(nq, K))
    _check(oracle_lib, codes.cpu().numpy(), qb.cpu().numpy(), K, D1, I1)


# ----------------------------------------------------------------------------- 6. Python surface
def test_binary_index_1536_batched(dev, oracle_lib):
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    rng = np.random.default_rng(9)
    n, nq = 70_001, 130
    codes = rng.integers(0, 256, (n, 192), dtype=np.uint8)
    ids = rng.permutation(1_000_000)[:n].astype(np.int64)
    a = BinaryIndexIDMap2(1536, dev)
    for s in range(0, n, 30_000):
        a.add_with_ids(codes[s:s + 30_000], ids[s:s + 30_000])
    q = _flip(rng, codes[rng.integers(0, n, nq)], 100)
    for k in (10, 100):
        Da, La = a.search(q, k)
        D0, I0 = oracle_knn(oracle_lib, codes, q, k, threads=16)
        assert np.array_equal(np.asarray(Da), D0) and np.array_equal(np.asarray(La), ids[I0])


def test_enhanced_search3_384_equals_wavefront_scan(dev):
    """enhanced.search3 (what CohereEnhancedVectorDB.search_vectors runs on its buffers) at 384 dims and
    >= 65 536 rows returns what the forced wavefront scan returns."""
    from vectorragquantization_amd import synth
    from vectorragquantization_amd.enhanced import search3
    from vectorragquantization_amd.quant import int8_row_norms
    Nn = _nat()
    d, n, nq = 384, 66_000, 200
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    codes = synth.random_codes(n, d // 8, device=dev, seed=78)
    qb, _ = synth.flip_queries(codes, nq, flips=(20, 60), seed=79)
    x8 = torch.randint(-127, 128, (n, d), generator=g, device=dev, dtype=torch.int8)
    norms = int8_row_norms(x8)
    qf = (torch.round(torch.randn((nq, d), generator=g, device=dev) * 4096) / 65536).float()
    a = search3(codes, x8, norms, qf, qb, 10, 100, 30, 0)
    b = search3(codes, x8, norms, qf, qb, 10, 100, 30, Nn.VRQ_SEARCH_SCAN_VALU)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
