"""The gather entry points (vrq_*_gather: the *_batch calls over an ascending row list): symbols, the plan and
workspace equalities at m rows, and the return codes.  CPU only: every call returns before it would launch."""
import ctypes as C

import pytest

from vectorragquantization_amd import _native as N

P = C.c_void_p(8)     # a non-null, aligned pointer that is never dereferenced
ODD = C.c_void_p(10)  # non-null, not 4-byte aligned
BIG = 1 << 40
BASES = ("vrq_scan", "vrq_hamming_topk", "vrq_search3", "vrq_search2")
ENGINES = (N.VRQ_LARGE_ENGINE_AUTO, N.VRQ_LARGE_ENGINE_VALU, N.VRQ_LARGE_ENGINE_MFMA)


def scan(L, n=1000, dim=1024, K=2000, rows=P, m=500, wsb=BIG, engine=2, nq=2, codes=P):
    return L.vrq_scan_gather(codes, n, dim, P, nq, K, 0, rows, m, P, wsb, None, engine)


def hamming(L, n=1000, dim=1024, K=2000, rows=P, m=500, wsb=BIG, engine=2, nq=2, codes=P):
    return L.vrq_hamming_topk_gather(codes, n, dim // 8, 0, P, nq, K, rows, m, P, P, P, wsb, None, engine)


def search3(L, n=1000, dim=1024, K=2000, rows=P, m=500, wsb=BIG, engine=2, nq=2, codes=P, flags=0):
    return L.vrq_search3_gather(codes, P, P, None, n, dim, 0, P, P, nq, 10, K, 30, flags, rows, m, P, P, P, P, P, P,
                                wsb, None, engine)


def search2(L, n=1000, dim=1024, K=2000, rows=P, m=500, wsb=BIG, engine=2, nq=2, codes=P, flags=0):
    return L.vrq_search2_gather(0, codes, P, None, 0.3, None, n, dim, 0, P, P, nq, 10, K, flags, rows, m, P, P, P, P,
                                P, wsb, None, engine)


CALLS = (scan, hamming, search3, search2)


def test_symbols():
    lib = N.load()
    for b in BASES:
        assert hasattr(lib, b + "_gather") and hasattr(lib, b + "_gather_workspace_size")
    assert hasattr(lib, "vrq_scan_gather_plan")
    assert sum("_gather" in s and "binary_topk" not in s for s in N.SIGNATURES) == 9


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("m,dim,nq,K", [(1, 256, 1, 1), (12325, 1024, 17, 1500), (700, 384, 64, 1500),
                                        (1000000, 2048, 600, 8192), (40000, 1536, 3, 100)])
def test_plan_and_workspace_are_the_batch_calls_at_m_rows(m, dim, nq, K, engine):
    lib = N.load()
    a, b = (C.c_int64 * 10)(), (C.c_int64 * 10)()
    assert lib.vrq_scan_gather_plan(m, dim, nq, K, engine, a) == lib.vrq_scan_batch_plan(m, dim, nq, K, engine, b) == 0
    assert list(a) == list(b)
    for base in BASES:
        w = dim // 8 if base == "vrq_hamming_topk" else dim
        got = getattr(lib, base + "_gather_workspace_size")(m, w, nq, K)
        assert got == getattr(lib, base + "_batch_workspace_size")(m, w, nq, K) > 0
    assert lib.vrq_search3_gather_workspace_size(0, dim, nq, K) == lib.vrq_search3_batch_workspace_size(1, dim, nq, K)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("kw,rc", [
    (dict(rows=None), N.VRQ_EINVAL), (dict(rows=ODD), N.VRQ_EINVAL), (dict(m=-1), N.VRQ_EINVAL),
    (dict(m=1001), N.VRQ_EINVAL), (dict(engine=3), N.VRQ_EINVAL), (dict(engine=-1), N.VRQ_EINVAL),
    (dict(rows=None, wsb=16), N.VRQ_EINVAL),       # the list is checked before the workspace
    (dict(codes=None), N.VRQ_EINVAL),
    (dict(K=8193), N.VRQ_EUNSUPPORTED), (dict(dim=640), N.VRQ_EUNSUPPORTED),
    (dict(wsb=16), N.VRQ_EWORKSPACE), (dict(m=1000, wsb=16), N.VRQ_EWORKSPACE),
    (dict(m=0, rows=None, codes=None, nq=0), N.VRQ_OK),  # m = 0 is accepted and reads no list
])
def test_return_codes(call, kw, rc):
    for engine in ENGINES if "engine" not in kw else (kw["engine"],):
        assert call(N.load(), **{**kw, "engine": engine}) == rc


def test_search_call_route():
    class T:  # a stand-in with a shape: SearchCall reads the list's length only
        shape = (5,)
    c = N.SearchCall("vrq_search3", 100, rows=T())
    assert (c.name, c.engine, c.m) == ("vrq_search3_gather", N.VRQ_LARGE_ENGINE_AUTO, 5)
    for bad in (dict(allow=T()), dict(query_set=T(), allow=T()), dict(flags=N.VRQ_SEARCH_SHARD), dict(K=8193)):
        with pytest.raises(N.VrqNativeError):
            N.SearchCall("vrq_search3", **{"K": 100, "rows": T(), **bad})
