"""Edge paths of K1s (hamming_mfma_swap_kernel<2, 8>), the kernel of every large-batch pass of at most 2^32
(query, row) pairs -- config 2's headline -- against the FAISS restatement and against the exact lists.

The inputs come from tests/k1s_cases.py (their preconditions are checked without a GPU in
tests/test_k1s_cases.py); the chunk geometry comes from vrq_scan_plan.  Every case asserts that the plan
runs K1s, that the whole top-K (all queries, distances and rows) equals the oracle's bit for bit, and the
property it is there for:

* geometry matrix: idle waves (fewer than 8 row sets per chunk), a chunk and a row set of a single row, a
  workgroup of a single query, an all-padding query block of a pair, three row sets per wave; K = 1 and
  K = 128 with a row offset;
* dense patches: 16 queries of one block x 16 rows of one row block at distance <= 10, i.e. 256 hits in
  one 32x32 accumulator and 8 per lane (the one-ballot-per-register path of block_hits), placed so that
  every row-in-set and query-in-block position, every wave, the set after the switch and the partial last
  set are decoded; check_scan_lists proves every entry's row and distance;
* a stage flood in a LATE query block: the earlier blocks' staged hits (planted witnesses in every
  flooded row set) must survive, and only the flooded block and the later ones may be marked;
* a two-valued corpus: thresholds, keys and lane minima at both ends of their ranges.
"""
import numpy as np
import pytest
import torch

from tests import k1s_cases as C
from tests.conftest import oracle_knn
from tests.test_gpu_lists import _dist, check_scan_lists, scan_paths

pytestmark = pytest.mark.gpu

K = 100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plan(n, nq, K_=K, k1s=True):
    """vrq_scan_plan -> (kind, M-blocks, chunk rows, chunks, capc)."""
    from vectorragquantization_amd import _native as N
    info = np.zeros(12, np.int64)
    N.check(N.load().vrq_scan_plan(n, 1024, nq, K_, N.VRQ_SEARCH_SCAN_MFMA, info.ctypes.data), "plan")
    if k1s:
        assert (int(info[0]), int(info[1])) == (2, 4), "shape does not run K1s"
    return tuple(int(x) for x in info[:5])


def _phase1(codes_t, qb_t, K_, row_offset=0):
    """vrq_search3 PHASE1_ONLY on the matrix-core scan -> (count, dist, rows)."""
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd.enhanced import search3
    dev = codes_t.device
    nq = qb_t.shape[0]
    x8 = torch.empty((1, 1024), dtype=torch.int8, device=dev)
    norms = torch.empty((1,), dtype=torch.float64, device=dev)
    qf = torch.zeros((nq, 1024), dtype=torch.float32, device=dev)
    cnt, rows, dist, _, _ = search3(codes_t, x8, norms, qf, qb_t, K_, K_, K_,
                                    N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_MFMA, row_offset)
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), dist.cpu().numpy(), rows.cpu().numpy()


def _assert_topk(oracle_lib, codes, qb, codes_t, qb_t, K_, row_offset=0):
    D0, I0 = oracle_knn(oracle_lib, codes, qb, K_, threads=16)
    c, D1, I1 = _phase1(codes_t, qb_t, K_, row_offset)
    assert np.array_equal(c, np.full(qb.shape[0], K_))
    assert np.array_equal(D0, D1)
    assert np.array_equal(I0 + row_offset, I1)
    return D0, I0


# (nq, n, the property the shape is there for, from the plan's chunk rows cr and chunks nch)
GEOMETRY = [
    (512, 65_536, lambda nq, n, cr, nch: cr // C.SRS == 4),                       # waves 4..7 idle
    (513, 65_665, lambda nq, n, cr, nch: nq - C.SQPB == 1 and n - (nch - 1) * cr == 1),
    (545, 65_537, lambda nq, n, cr, nch: (n - (nch - 1) * cr) % C.SRS == 1),      # last row set: 1 row
    (577, 66_241, lambda nq, n, cr, nch: C.blocks_run(nq, 1) == (4, 3) and n - (nch - 1) * cr == 1),
    (1025, 65_536, lambda nq, n, cr, nch: (nq + C.SQPB - 1) // C.SQPB == 3 and nq - 2 * C.SQPB == 1),
    (2048, 65_599, lambda nq, n, cr, nch: cr // C.SRS == 17),                     # wave 0 owns sets 0, 8, 16
]


@pytest.mark.parametrize("nq,n,prop", GEOMETRY, ids=[f"{g[0]}x{g[1]}" for g in GEOMETRY])
def test_k1s_geometry(dev, oracle_lib, nq, n, prop):
    _, _, cr, nch, _ = _plan(n, nq)
    assert prop(nq, n, cr, nch), f"chunks of {cr} rows x {nch} do not give the shape this case is there for"
    codes, qb = C.geometry_case(n, nq, cr, 7000 + nq)
    codes_t, qb_t = _t(codes, dev), _t(qb, dev)
    D0, I0 = _assert_topk(oracle_lib, codes, qb, codes_t, qb_t, K)
    assert (D0[0, 0], I0[0, 0]) == (0, n - 1) and D0[nq - 1, 0] == 0
    check_scan_lists(codes_t, qb_t, K)


@pytest.mark.parametrize("K_", [1, 128])
def test_k1s_k_bounds_row_offset(dev, oracle_lib, K_):
    n, nq = 70_001, 1024
    _, _, cr, _, _ = _plan(n, nq, K_)
    codes, qb = C.geometry_case(n, nq, cr, 7100 + K_)
    _assert_topk(oracle_lib, codes, qb, _t(codes, dev), _t(qb, dev), K_, row_offset=5_000_000)


def test_k1s_dense_patches(dev, oracle_lib):
    """256 hits in one accumulator, 8 per lane, at every decoded position (see the module docstring)."""
    n, nq = 66_241, 577
    _, _, cr, nch, capc = _plan(n, nq)
    codes, qb, patches = C.patch_case(n, nq, cr, 7200)
    codes_t, qb_t = _t(codes, dev), _t(qb, dev)
    D = _dist(codes_t, qb_t).cpu().numpy()
    hit = D < C.standin_tau(D, K)[:, None]
    assert max(int(C.stage_load(hit, wg).max()) for wg in range(2)) <= C.STG, "a patch would overflow the stage"
    assert int(C.list_load(hit, cr).max()) <= capc, "a patch would overflow a list"
    for qs, rows in patches:
        assert (D[np.ix_(qs, rows)] <= 10).all()
    ovf, rerun, _, _ = scan_paths(codes_t, qb_t, K)
    print(f"dense patches: {int(ovf.sum())} of {nq} queries overflowed, {int(rerun.sum())} re-ran")
    _assert_topk(oracle_lib, codes, qb, codes_t, qb_t, K)
    check_scan_lists(codes_t, qb_t, K)


def test_k1s_late_block_stage_overflow(dev, oracle_lib):
    """The flood overflows the stage in block 14 of workgroup 0 and block 9 of workgroup 1, in every row set
    of the suffix: those blocks and the later ones of their workgroups are marked, nothing else is, and
    the hits the earlier blocks staged before the flood (the witnesses) are all in their lists."""
    n, nq = 70_001, 1024
    _, _, cr, nch, capc = _plan(n, nq)
    codes, qb, wit = C.flood_case(n, nq, 7300)
    codes_t, qb_t = _t(codes, dev), _t(qb, dev)
    fq, may = C.flood_queries(), C.flood_may_mark(nq)
    D = _dist(codes_t, qb_t).cpu().numpy()
    flood_rows = np.setdiff1d(np.arange(C.FLOOD_S, n), [r for _, r in wit])
    assert (D[np.ix_(fq, flood_rows)] == 10).all()
    hit = D < C.standin_tau(D, K)[:, None]
    back = hit.copy()
    back[fq] = False
    suffix_sets = np.arange(C.FLOOD_S // C.SRS, (n + C.SRS - 1) // C.SRS)
    for wg in range(2):
        flood = C.stage_load(hit, wg) - C.stage_load(back, wg)
        assert (flood[suffix_sets[:-1]] > C.STG).all(), "the flood must overflow the stage in every full suffix set"
        assert int(C.stage_load(back, wg).max()) < C.STG, "the background alone must not overflow the stage"
    wq, wr = np.array(wit).T
    assert hit[wq, wr].all() and not np.isin(wq, may).any()
    ovf, rerun, _, _ = scan_paths(codes_t, qb_t, K)
    marked = np.flatnonzero(ovf)
    print(f"late-block flood: {marked.size} of {nq} queries overflowed ({int(ovf[:512].sum())} in workgroup 0, "
          f"{int(ovf[512:].sum())} in workgroup 1), {int(rerun.sum())} re-ran")
    assert np.isin(marked, may).all(), f"queries outside the flooded blocks' tails are marked: {np.setdiff1d(marked, may)}"
    assert ovf[fq].all(), "every flood query must be marked"
    assert int(ovf[:512].sum()) <= 64 and int(ovf[512:].sum()) <= 224
    check_scan_lists(codes_t, qb_t, K, allow_overflow=True)
    _assert_topk(oracle_lib, codes, qb, codes_t, qb_t, K)


# K1r MB = 1, the lean MB = 2, MB = 4; K1m MB = 2; K1s: every instance sees the extreme seeds and thresholds
@pytest.mark.parametrize("nq", [8, 40, 100, 200, 600])
def test_two_valued_corpus(dev, oracle_lib, nq):
    """All rows zero but 50 all-ones rows.  For the all-ones query the K-th distance is 1024, so tau = 1025
    and v = dist - tau takes both ends of its range (-1025 for the ones rows, -1 for the zero rows); the
    sample's u16 lane minima reach 0 (ones query, ones row) and 2048 (zeros query, ones row).  Every
    query's threshold admits every row at its nearer value, so every list that can overflow does: chunks
    hold more rows than a list (capc) or, at 40 queries, a 32-row block stages 1280 > 512 hits.  At 8
    queries neither holds -- chunks are 64 rows, capc is 64 and a block stages 256 hits -- so there every
    list must be exactly full instead."""
    n = 65_600
    kind, mb, cr, nch, capc = _plan(n, nq, k1s=False)
    assert (kind, mb) == {8: (1, 1), 40: (1, 2), 100: (1, 4), 200: (0, 2), 600: (2, 4)}[nq]
    codes, qb, ones = C.two_valued_case(n, nq, 7400 + nq)
    codes_t, qb_t = _t(codes, dev), _t(qb, dev)
    ovf, rerun, _, j = scan_paths(codes_t, qb_t, K)
    print(f"two-valued nq={nq}: j={j}, {int(ovf.sum())} of {nq} queries overflowed, {int(rerun.sum())} re-ran")
    if cr > capc or 32 * nq > C.STG:
        assert ovf.all(), "every query's lists must overflow"
    else:
        assert nq == 8 and cr == capc and not ovf.any()
        check_scan_lists(codes_t, qb_t, K)               # exactly full lists, none lost, none marked
    D0, I0 = _assert_topk(oracle_lib, codes, qb, codes_t, qb_t, K)
    zeros = np.setdiff1d(np.arange(K + 50), ones)[:K - 50]
    assert np.array_equal(I0[0], np.concatenate([ones, zeros])) and (D0[0, 50:] == 1024).all()
