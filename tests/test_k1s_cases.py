"""The preconditions of the K1s edge tests (tests/test_gpu_k1s_edges.py), checked without a GPU: exact
NumPy distances of the inputs tests/k1s_cases.py builds against the geometry vrq_scan_plan reports (host
only), with (K-th distance + 3) as a generous stand-in for the threshold a pass runs with.  Also the
Python restatement of mfma_sample_order against the library's plan: where the sampled threshold is live
(j < K) and where it is not, which decides whether a test of the re-run can reach it at all.
"""
import numpy as np
import pytest

from tests import k1s_cases as C

K = 100


def _plan(n, nq, K_=K):
    from vectorragquantization_amd import _native as N
    info = np.zeros(12, np.int64)
    N.check(N.load().vrq_scan_plan(n, 1024, nq, K_, N.VRQ_SEARCH_SCAN_MFMA, info.ctypes.data), "plan")
    return [int(x) for x in info]


def test_sample_order_restatement():
    """j = K (no sampled threshold, no re-run) up to 100 000 rows; 88, 64, 48 and 16 above."""
    for n, want in [(65_536, 100), (70_001, 100), (100_000, 100), (131_072, 88), (200_000, 64), (300_007, 48),
                    (4_200_007, 16)]:
        info = _plan(n, 1024)
        assert info[9] == want, (n, info[9])
        assert C.sample_order(K * info[8] / n, K) == want          # info[8]: the plan's sample rows
    # the planned sample never drops below MIN_SAMPLE less one tile per sample chunk
    assert C.sample_order(K * C.MIN_SAMPLE / 100_000, K) == K
    for nq in (20, 50, 100, 300, 600, 1100):                       # the re-run test's shapes
        assert _plan(300_007, nq)[9] == 48
    for nq in (40, 64, 200, 600):                                  # the stage-overflow test's: tau = tau_p
        assert _plan(100_000, nq)[9] == K


def test_geometry_shapes():
    """The property each shape of the geometry matrix is there for, from the plan."""
    for nq, n in [(512, 65_536), (513, 65_665), (545, 65_537), (577, 66_241), (1025, 65_536), (2048, 65_599),
                  (1024, 70_001)]:
        info = _plan(n, nq)
        assert (info[0], info[1]) == (2, 4) and info[2] % C.SRS == 0
    cr, nch = _plan(65_536, 512)[2:4]
    assert cr // C.SRS == 4 < C.SNW
    cr, nch = _plan(65_665, 513)[2:4]
    assert 65_665 - (nch - 1) * cr == 1 and C.blocks_run(513, 1) == (2, 1)
    cr, nch = _plan(65_537, 545)[2:4]
    assert (65_537 - (nch - 1) * cr) % C.SRS == 1
    cr, nch = _plan(66_241, 577)[2:4]
    assert 66_241 - (nch - 1) * cr == 1 and C.blocks_run(577, 1) == (4, 3)
    assert C.blocks_run(1025, 2) == (2, 1)
    cr, nch = _plan(65_599, 2048)[2:4]
    assert cr // C.SRS == 17 and (17 - 0 + C.SNW - 1) // C.SNW == 3


def test_patch_preconditions():
    n, nq = 66_241, 577
    _, _, cr, nch, capc = _plan(n, nq)[:5]
    codes, qb, patches = C.patch_case(n, nq, cr, 7200)
    D = C.distances(qb, codes)
    hit = D < C.standin_tau(D, K)[:, None]
    assert max(int(C.stage_load(hit, wg).max()) for wg in range(2)) <= C.STG
    assert int(C.list_load(hit, cr).max()) <= capc
    rowpos, qpos, waves, kth, blocks = set(), set(), set(), set(), set()
    partial = False
    for qs, rows in patches:
        assert (D[np.ix_(qs, rows)] <= 10).all() and hit[np.ix_(qs, rows)].all()
        assert np.unique(rows // cr).size == 1 and np.unique(rows // C.SRS).size == 1 and np.unique(qs // 32).size == 1
        rs = int(rows[0] % cr) // C.SRS
        rowpos |= set((rows % cr % C.SRS).tolist())
        qpos |= set((qs % 32).tolist())
        waves.add(rs % C.SNW)
        kth.add(rs // C.SNW)
        blocks.add((int(qs[0]) // C.SQPB, int(qs[0]) % C.SQPB // 32))
        partial |= min(n, (int(rows[0]) // cr + 1) * cr) - int(rows[0]) // C.SRS * C.SRS < C.SRS
        if qs.size == 16 and rows.size == 16:                      # 256 hits in one accumulator, 8 per lane
            lane_rows = (rows % 32 % 8) // 4                       # row (g & 3) + 8 (g >> 2) + 4 h: lane half h
            assert np.bincount(lane_rows, minlength=2).tolist() == [8, 8]
    assert rowpos == set(range(64)) and qpos == set(range(32))
    assert waves == set(range(C.SNW)) and kth == {0, 1} and partial
    assert {(0, 0), (0, 15), (1, C.blocks_run(nq, 1)[1] - 1)} <= blocks


def test_flood_preconditions():
    n, nq = 70_001, 1024
    _, _, cr, nch, capc = _plan(n, nq)[:5]
    assert C.FLOOD_S % cr % C.SRS == 0                            # the suffix starts on a row set
    codes, qb, wit = C.flood_case(n, nq, 7300)
    fq, may = C.flood_queries(), C.flood_may_mark(nq)
    assert fq.size == 64 and np.isin(fq, may).all()
    assert (may < C.SQPB).sum() == 64 and (may >= C.SQPB).sum() == 224
    D = C.distances(qb, codes)
    wq, wr = np.array(wit).T
    flood_rows = np.setdiff1d(np.arange(C.FLOOD_S, n), wr)
    assert (D[np.ix_(fq, flood_rows)] == 10).all()
    hit = D < C.standin_tau(D, K)[:, None]
    back = hit.copy()
    back[fq] = False
    suffix_sets = np.arange(C.FLOOD_S // C.SRS, (n + C.SRS - 1) // C.SRS)
    for wg, (_, blk) in enumerate(C.FLOOD_BLOCKS):
        flood = C.stage_load(hit, wg) - C.stage_load(back, wg)
        assert (flood[suffix_sets[:-1]] > C.STG).all()
        assert int(C.stage_load(back, wg).max()) < C.STG
        # every suffix row set holds a witness of an earlier block of this workgroup
        w = wq // C.SQPB == wg
        assert (wq[w] % C.SQPB // 32 < blk).all()
        assert np.array_equal(np.unique(wr[w] // C.SRS), suffix_sets)
        assert set((wq[w] % C.SQPB // 32).tolist()) == set(range(blk))
    assert hit[wq, wr].all() and (D[wq, wr] == 8).all()
    # the unmarked queries' lists fit
    keep = np.setdiff1d(np.arange(nq), may)
    assert int(C.list_load(hit[keep], cr).max()) <= capc


@pytest.mark.parametrize("nq", [8, 40, 100, 200, 600])
def test_two_valued_preconditions(nq):
    n = 65_600
    kind, mb, cr, nch, capc = _plan(n, nq)[:5]
    codes, qb, ones = C.two_valued_case(n, nq, 7400 + nq)
    pc = np.unpackbits(qb, axis=1).sum(1)
    assert pc[0] == 1024 and pc[1] == 0 and ones.size == 50
    # the K-th distance of every query is its distance to the zero rows or more (only 50 rows are ones), so
    # every zero row is below tau and a chunk without ones rows puts all its rows on the list
    assert (pc <= np.partition(C.distances(qb, codes), K - 1, axis=1)[:, K - 1]).all()
    assert np.diff(ones).max() > 2 * cr and cr >= capc
    # where the lists can overflow: more rows per chunk than capc, or more hits per 32-row block than the stage
    assert (cr > capc or 32 * nq > C.STG) == (nq != 8)
