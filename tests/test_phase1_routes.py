"""The host-side Phase-I decisions of every search entry point against the recorded table
(tests/golden/phase1_routes.npz, written by tests/golden/make_golden_routes.py): which scan a shape takes,
the plan, the sample plan and the workspace sizes, exactly; and the workspace refusal of each entry point
that runs a route, one byte below the size of that route.  CPU only: every call returns before a launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from vectorragquantization_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_golden_routes as G  # noqa: E402

P8 = C.c_void_p(8)  # a non-null pointer that validation must never dereference
ROUTE_FLAGS = (N.VRQ_SEARCH_SCAN_VALU, N.VRQ_SEARCH_SCAN_MFMA)  # the columns of route_bytes


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(os.path.join(GOLDEN, "phase1_routes.npz")))


def test_table_is_reproduced_exactly(recorded):
    got = G.collect(N.load())
    assert sorted(got) == sorted(recorded)
    for name, want in recorded.items():
        bad = np.argwhere(got[name] != want)
        assert got[name].shape == want.shape and bad.size == 0, (name, bad[:5].tolist())


def test_table_covers_both_routes(recorded):
    """The grid is not vacuous: both kinds, refusals and successful plans appear at every dim."""
    for j in range(len(G.DIMS)):
        kinds = set(recorded["kind"][j, ..., 0].ravel().tolist())
        assert {N.VRQ_SCAN_KIND_VALU, N.VRQ_SCAN_KIND_MFMA} <= kinds
        assert {N.VRQ_OK, N.VRQ_EUNSUPPORTED} <= set(recorded["plan"][j, ..., 0].ravel().tolist())
    assert (recorded["route_bytes"] > 0).all()


def _scan(L, d, flags, ws_bytes):
    n, nq, K = G.ROUTE_SHAPE
    return L.vrq_search3_dim_scan(P8, n, d, P8, nq, K, flags, P8, ws_bytes, None)


def _finish(L, d, flags, ws_bytes):
    n, nq, K = G.ROUTE_SHAPE
    return L.vrq_search3_dim_finish(P8, None, None, None, n, d, 0, None, nq, 1, K, 1,
                                    flags | N.VRQ_SEARCH_PHASE1_ONLY, P8, P8, P8, None, None, P8, ws_bytes, None)


def _finish2(L, d, flags, ws_bytes):
    n, nq, K = G.ROUTE_SHAPE
    return L.vrq_search2_finish(N.VRQ_RESCORE_F32, P8, P8, None, 0.0, None, n, d, 0, P8, nq, 1, K, flags,
                                P8, P8, P8, P8, P8, ws_bytes, None)


@pytest.mark.parametrize("route", (0, 1), ids=("wavefront", "matrix"))
@pytest.mark.parametrize("d", G.DIMS)
def test_workspace_refusal_one_byte_below_the_route(recorded, d, route):
    L = N.load()
    n, nq, K = G.ROUTE_SHAPE
    flags = ROUTE_FLAGS[route]
    need = int(recorded["route_bytes"][G.DIMS.index(d), route])
    assert L.vrq_scan_kind(n, d, nq, K, flags, None) == route
    for call in (_scan, _finish, _finish2):
        assert call(L, d, flags, need - 1) == N.VRQ_EWORKSPACE, call.__name__
    # vrq_hamming_topk takes no flags: it runs the route of the default choice
    if L.vrq_scan_kind(n, d, nq, K, 0, None) == route:
        assert L.vrq_hamming_topk(P8, n, d // 8, 0, P8, nq, K, P8, P8, P8, need - 1, None) == N.VRQ_EWORKSPACE
    # with exactly the route's size the refusal is never the workspace: an unsupported flag is reported
    # (still before any launch).  The 1024 scan and finish have no unsupported flag.
    assert _finish2(L, d, flags | N.VRQ_SEARCH_PHASE1_ONLY, need) == N.VRQ_EUNSUPPORTED
    if d != 1024:
        assert _scan(L, d, flags | N.VRQ_SEARCH_SHARD, need) == N.VRQ_EUNSUPPORTED
        assert _finish(L, d, flags | N.VRQ_SEARCH_SHARD, need) == N.VRQ_EUNSUPPORTED


def test_hamming_topk_default_route_is_covered(recorded):
    """The default choice at the refusal shape is the matrix scan at every dim, so the vrq_hamming_topk row
    above runs; its size function covers both routes."""
    L = N.load()
    n, nq, K = G.ROUTE_SHAPE
    for j, d in enumerate(G.DIMS):
        assert L.vrq_scan_kind(n, d, nq, K, 0, None) == N.VRQ_SCAN_KIND_MFMA
        assert L.vrq_hamming_topk_workspace_size(n, d // 8, nq, K) == int(recorded["route_bytes"][j].max())
