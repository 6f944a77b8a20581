"""The host-side decisions of the counting scan against the recorded table (tests/golden/count_route_plans.npz,
written by tests/golden/make_golden_count_route.py from the library of commit b073ca6, the last one before the
plan and the pass loop moved into count_route.hip): the return code and every info word of vrq_scan_large_plan
and of vrq_scan_batch_plan under each engine, vrq_large_engine, and the eleven *_large / *_filtered / *_batch
and the two sharded *_large workspace sizes, exactly, at every shape of the grid.  CPU only: every function
asked is a pure function of the call shape."""
import os
import sys

import numpy as np
import pytest

from vectorragquantization_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_golden_count_route as G  # noqa: E402

AUTO, VALU, MFMA = range(3)  # the engine axis of ``batch``


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(os.path.join(GOLDEN, "count_route_plans.npz")))


def test_table_is_reproduced_exactly(recorded):
    got = G.collect(N.load())
    assert sorted(got) == sorted(recorded)
    for name, want in recorded.items():
        bad = np.argwhere(got[name] != want)
        assert got[name].shape == want.shape and bad.size == 0, (name, bad[:5].tolist())


def test_table_covers_the_boundaries_it_names(recorded):
    """The grid is not vacuous: each refusal, both AUTO answers, the flush boundary, the second pass and the
    chunk-count cap appear in it."""
    large, batch, engine, ws = (recorded[k] for k in ("large", "batch", "engine", "ws"))
    assert large.shape[:4] == (len(G.DIMS), len(G.NS), len(G.NQS), len(G.KS))
    assert {N.VRQ_OK, N.VRQ_EUNSUPPORTED} == set(large[..., 0].ravel().tolist())
    ok = large[..., 0] == N.VRQ_OK
    d320, n32, k8193 = G.DIMS.index(320), G.NS.index(2 ** 32), G.KS.index(8193)
    assert not ok[d320].any() and not ok[:, n32].any() and not ok[..., k8193].any()
    assert ok.sum() == (len(G.DIMS) - 1) * (len(G.NS) - 1) * len(G.NQS) * (len(G.KS) - 1)
    assert (batch[..., 0] == large[..., None, 0]).all() and ((ws > 0) == ok[..., None]).all()
    # AUTO answers both engines, and the same with and without a bitmap; a refusal is the plan's
    assert {N.VRQ_LARGE_ENGINE_VALU, N.VRQ_LARGE_ENGINE_MFMA} <= set(engine[ok].ravel().tolist())
    assert (engine[..., 0] == engine[..., 1]).all() and (engine[~ok][:, 0] == N.VRQ_EUNSUPPORTED).all()
    assert (batch[..., AUTO, 1][ok] == engine[..., 0][ok]).all()
    for d, first in ((1024, 16), (2048, 16)):   # the measured thresholds
        row = engine[G.DIMS.index(d), G.NS.index(1_000_000), :, 0, 0]
        assert [int(e) == N.VRQ_LARGE_ENGINE_MFMA for e in row] == [nq >= first for nq in G.NQS]
    # K1hm flushes (info[5] = 65 280) only where a chunk is longer than that
    flush = batch[..., MFMA, 6][ok]
    assert set(flush.tolist()) == {0, 65_280}
    assert (batch[:, G.NS.index(65_280), :, :, MFMA, 6] <= 0).all()
    assert ((flush > 0) == (batch[..., MFMA, 2][ok] > 65_280)).all()
    # chunk counts reach the cap of 1024 at large n, and the *_batch sizes cover both engines
    assert large[..., 2].max() == 1024 and batch[..., MFMA, 3].max() == 1024
    names = list(G.WS_NAMES)
    need = np.maximum(batch[..., VALU, 10], batch[..., MFMA, 10])[ok]
    assert (ws[..., names.index("vrq_search3_batch_workspace_size")][ok] == need).all()
    assert (ws[..., names.index("vrq_search3_large_workspace_size")][ok] == large[..., 8][ok]).all()
    assert (ws[..., names.index("vrq_shard_search3_large_workspace_size")][ok] == large[..., 8][ok]).all()
