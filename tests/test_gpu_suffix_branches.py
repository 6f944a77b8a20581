"""GPU checks of the suffix merge's middle branches (suffix_topk_kernel<CB> of mfma_threshold.hip, at 1024
bits and at two other dims), against the C restatement of
hammings_knn_hc (CohereEnhancedVectorDB.py:267-268: dist ascending, then row ascending), bit for bit.

The edge tests of test_gpu_mfma.py / test_gpu_k1m_edges.py / test_gpu_dims_mfma.py reach "every list fits
the sort buffer" and "a list overflowed: exact rescan".  Between them the kernel has three more branches,
each reached here by one planted query of the batch, with the branch's precondition asserted from the list
lengths the matrix pass left in the workspace:

* query A -- no list overflows, but the lists together hold more than SUF_CAP = 4096 keys: a histogram
  of the keys' v-fields finds the K-th smallest v, and the keys at or under it (about 103) fit the buffer;
* query B -- more than SUF_THREADS = 256 and at most 4096 keys: all gathered, then filtered in LDS to the
  keys at or under the K-th smallest v before the sort;
* query C -- as A, but all 6144 planted rows are at distance 5: the tie level alone exceeds the buffer, so
  the histogram branch gives up and the query is rescanned exactly (the first 100 dist-5 rows by row).

The planted rows sit at offsets the dense sample never reads (the sample tiles are 64 rows every `ts` rows;
ts comes from vrq_scan_sample_plan), so the thresholds come from the uniform background: tau_s is about
dim/2 - 3.15 sqrt(dim)/2 >= 103, every planted row (<= 60 bits from its query) is a candidate, and no query
re-runs.
"""
import numpy as np
import pytest
import torch

from tests.conftest import oracle_knn
from tests.test_gpu_dims_mfma import _flip, _phase1, _plan, _sample_rows, _scan_stages, _workspace_views

pytestmark = pytest.mark.gpu

N = 262_144
K = 100
NQ_ALL = 256
GROUP = 128              # three planted rows per query and 128-row group
SUF_THREADS, SUF_CAP = 256, 4096
QA, QB, QC = 0, 1, 2     # the planted queries (inside the first 8, so both batch sizes hold them)
# dim -> nq -> (scan kind, M-blocks per wave, chunks, rows per chunk) of vrq_scan_plan
PLANS = {1024: {8: (1, 1, 2048, 128), 256: (0, 2, 256, 1024)},
         384: {8: (3, 1, 2048, 128), 256: (3, 4, 512, 512)},
         2048: {8: (3, 1, 1024, 256), 256: (3, 2, 256, 1024)}}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _planted_rows(n, ts):
    """Three rows per 128-row group for each of A, C and B, all at offsets r % ts >= 64 (never in a sample
    tile) -> (rows_a[6144], rows_b[1024], rows_c[6144]), each ascending."""
    free = (np.arange(n) % ts >= 64).reshape(n // GROUP, GROUP)
    assert (free.sum(1) >= 54).all(), "every 128-row group needs 54 rows outside the sample tiles"
    order = np.argsort(~free, axis=1, kind="stable")          # a group's unsampled offsets first, ascending
    base = np.arange(n // GROUP, dtype=np.int64)[:, None] * GROUP
    pick = lambda first: np.sort((base + order[:, [first, first + 20, first + 40]]).reshape(-1))
    return pick(3), pick(13)[:1024], pick(8)


_CASE = {}


def _case(d, oracle_lib):
    """Corpus, the 256 queries and their exact top-K, once per dim (the 8-query batch is their first 8)."""
    if d not in _CASE:
        from vectorragquantization_amd import _native as Nn
        rng = np.random.default_rng(4100 + d)
        cb = d // 8
        sp = np.zeros(6, np.int64)
        Nn.check(Nn.load().vrq_scan_sample_plan(N, d, NQ_ALL, K, Nn.VRQ_SEARCH_SCAN_MFMA, sp.ctypes.data), "sample plan")
        ts = int(sp[4])
        codes = rng.integers(0, 256, (N, cb), dtype=np.uint8)
        qb = rng.integers(0, 256, (NQ_ALL, cb), dtype=np.uint8)
        qb[3::2] = _flip(rng, codes[rng.integers(0, N, qb[3::2].shape[0])], 30)   # near queries among the far
        rows_a, rows_b, rows_c = _planted_rows(N, ts)
        for q, rows in ((QA, rows_a), (QB, rows_b)):             # planted row i: 1 + i % 60 bits from the query
            for c in range(60):
                sel = rows[c::60]
                codes[sel] = _flip(rng, np.broadcast_to(qb[q:q + 1], (sel.size, cb)), 1 + c)
        codes[rows_c] = _flip(rng, np.broadcast_to(qb[QC:QC + 1], (rows_c.size, cb)), 5)
        D0, I0 = oracle_knn(oracle_lib, codes, qb, K, threads=16)
        assert (D0[QA] == 1).all() and (D0[QC] == 5).all() and np.array_equal(I0[QC], rows_c[:K])
        _CASE[d] = (codes, qb, D0, I0, ts, np.concatenate([rows_a, rows_b, rows_c]))
    return _CASE[d]


@pytest.mark.parametrize("nq", (8, NQ_ALL))
@pytest.mark.parametrize("d", (1024, 384, 2048))
def test_suffix_middle_branches(dev, oracle_lib, d, nq):
    from vectorragquantization_amd import _native as Nn
    codes, qb_all, D0, I0, ts, planted = _case(d, oracle_lib)
    qb = qb_all[:nq]
    # the plan (host-only planners)
    info = _plan(N, d, nq, K)
    kind, mb, cr, nch, capc, sample, j = (int(info[i]) for i in (0, 1, 2, 3, 4, 8, 9))
    assert (kind, mb, nch, cr) == PLANS[d][nq]
    assert capc == 64 and sample == 65_536 and j == 53
    sp = np.zeros(6, np.int64)
    Nn.check(Nn.load().vrq_scan_sample_plan(N, d, nq, K, Nn.VRQ_SEARCH_SCAN_MFMA, sp.ctypes.data), "sample plan")
    assert int(sp[4]) == ts == (N - 64) // (sample // 64 - 1), "the planted offsets were chosen for this tile stride"
    insamp = np.zeros(N, bool)
    insamp[_sample_rows(N, d, nq, K)] = True
    assert insamp.sum() == sample and not insamp[planted].any(), "a planted row is in the dense sample"

    # the branch each planted query takes, from the list lengths of PREFIX + MATRIX + RECHECK
    codes_t, qb_t = torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev)
    winfo, ws = _scan_stages(codes_t, qb_t, d, K, (Nn.VRQ_SCAN_STAGE_PREFIX, Nn.VRQ_SCAN_STAGE_MATRIX,
                                                   Nn.VRQ_SCAN_STAGE_RECHECK))
    cnt, _, _, _, rerun = _workspace_views(winfo, ws, nq)
    cnt, rerun = cnt.cpu().numpy(), rerun.cpu().numpy()
    total = cnt.sum(1)
    print(f"d {d} nq {nq}: lists A {total[QA]} (max {cnt[QA].max()}), B {total[QB]} (max {cnt[QB].max()}), "
          f"C {total[QC]} (max {cnt[QC].max()}), re-runs {int((rerun != 0).sum())}")
    assert not (rerun != 0).any(), "a query re-ran with tau_p"
    for q in (QA, QC):
        assert cnt[q].max() <= capc and total[q] > SUF_CAP, "histogram branch: complete lists, more than SUF_CAP keys"
    assert cnt[QB].max() <= capc and SUF_THREADS < total[QB] <= SUF_CAP, "in-LDS filter: 256 < keys <= SUF_CAP"

    # the top-K of every query, exact in (dist, row) order
    c, D1, I1 = _phase1(codes_t, qb_t, d, K, Nn.VRQ_SEARCH_SCAN_MFMA)
    assert np.array_equal(c, np.full(nq, K))
    assert np.array_equal(D1, D0[:nq]) and np.array_equal(I1, I0[:nq])
