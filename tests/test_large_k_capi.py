"""The large-K entry points (vrq_*_large, the counting scan K1h): return codes and the host-side plan.
CPU only: every call returns before it would launch anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
P = C.c_void_p(8)  # a non-null pointer that is never dereferenced
BIG = 1 << 40      # workspace bytes no plan exceeds


def _plan(lib, n, dim, nq, K):
    info = np.zeros(8, np.int64)
    rc = lib.vrq_scan_large_plan(n, dim, nq, K, info.ctypes.data)
    return rc, [int(x) for x in info]


def hamming(L, codes=P, n=1000, cb=128, q=P, nq=2, k=2000, od=P, orows=P, ws=P, wsb=BIG):
    return L.vrq_hamming_topk_large(codes, n, cb, 0, q, nq, k, od, orows, ws, wsb, None)


def search3(L, codes=P, x8=P, norms=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, K3=30, flags=0, oc=P,
            orows=P, od=P, ob=P, ocos=P, ws=P, wsb=BIG):
    return L.vrq_search3_large(codes, x8, norms, None, n, dim, 0, qf, qb, nq, k, K, K3, flags, oc, orows, od, ob,
                               ocos, ws, wsb, None)


def search2(L, mode=0, codes=P, q=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, flags=0, oc=P, orows=P,
            od=P, osc=P, ws=P, wsb=BIG, minmax=None):
    return L.vrq_search2_large(mode, codes, q, minmax, 0.3, None, n, dim, 0, qf, qb, nq, k, K, flags, oc, orows, od,
                               osc, ws, wsb, None)


def test_limit_constant_matches_the_header():
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrq.h")
    m = re.search(r"#define\s+VRQ_K_LARGE_MAX\s+(\d+)", open(hdr).read())
    assert m and int(m.group(1)) == N.VRQ_K_LARGE_MAX == 8192


@pytest.mark.parametrize("call,expect", [
    # null pointers
    (lambda L: hamming(L, codes=None), N.VRQ_EINVAL),
    (lambda L: hamming(L, q=None), N.VRQ_EINVAL),
    (lambda L: hamming(L, od=None), N.VRQ_EINVAL),
    (lambda L: hamming(L, orows=None), N.VRQ_EINVAL),
    (lambda L: hamming(L, ws=None), N.VRQ_EINVAL),
    (lambda L: search3(L, codes=None), N.VRQ_EINVAL),
    (lambda L: search3(L, x8=None), N.VRQ_EINVAL),
    (lambda L: search3(L, norms=None), N.VRQ_EINVAL),
    (lambda L: search3(L, qf=None), N.VRQ_EINVAL),
    (lambda L: search3(L, qb=None), N.VRQ_EINVAL),
    (lambda L: search3(L, oc=None), N.VRQ_EINVAL),
    (lambda L: search3(L, orows=None), N.VRQ_EINVAL),
    (lambda L: search3(L, od=None), N.VRQ_EINVAL),
    (lambda L: search3(L, ob=None), N.VRQ_EINVAL),
    (lambda L: search3(L, ocos=None), N.VRQ_EINVAL),
    (lambda L: search3(L, ws=None), N.VRQ_EINVAL),
    (lambda L: search3(L, n=-1), N.VRQ_EINVAL),
    (lambda L: search3(L, K3=-1), N.VRQ_EINVAL),
    (lambda L: search2(L, codes=None), N.VRQ_EINVAL),
    (lambda L: search2(L, q=None), N.VRQ_EINVAL),
    (lambda L: search2(L, qf=None), N.VRQ_EINVAL),
    (lambda L: search2(L, qb=None), N.VRQ_EINVAL),
    (lambda L: search2(L, osc=None), N.VRQ_EINVAL),
    (lambda L: search2(L, ws=None), N.VRQ_EINVAL),
    (lambda L: search2(L, mode=3), N.VRQ_EINVAL),   # a local mode without minmax
    (lambda L: search2(L, mode=99), N.VRQ_EINVAL),
    (lambda L: L.vrq_scan_large_plan(1000, 1024, 1, 2000, None), N.VRQ_EINVAL),
    (lambda L: _plan(L, 0, 1024, 1, 2000)[0], N.VRQ_EINVAL),
    (lambda L: _plan(L, 1000, 1024, 0, 2000)[0], N.VRQ_EINVAL),
    (lambda L: _plan(L, 1000, 1024, 1, 0)[0], N.VRQ_EINVAL),
    # unsupported dim, K or k past the limit, n past 2^32 - 1
    (lambda L: hamming(L, cb=100), N.VRQ_EUNSUPPORTED),
    (lambda L: hamming(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: hamming(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: _plan(L, 1000, 640, 1, 2000)[0], N.VRQ_EUNSUPPORTED),
    (lambda L: _plan(L, 1000, 1024, 1, 8193)[0], N.VRQ_EUNSUPPORTED),
    (lambda L: _plan(L, 1 << 32, 1024, 1, 2000)[0], N.VRQ_EUNSUPPORTED),
    # flags outside the allowed set
    (lambda L: search3(L, flags=N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, flags=N.VRQ_SEARCH_SCAN_MFMA), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, flags=N.VRQ_SEARCH_SCAN_VALU), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, flags=N.VRQ_SCAN_STAGE_MATRIX), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, flags=N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SCAN_STAGE_SUFFIX), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, flags=N.VRQ_SEARCH_PHASE1_ONLY), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, flags=N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, flags=N.VRQ_SEARCH_SCAN_MFMA), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, flags=N.VRQ_SCAN_STAGE_PREFIX), N.VRQ_EUNSUPPORTED),
    # the staged scan
    (lambda L: L.vrq_scan_large(None, 1000, 1024, P, 1, 2000, 0, P, BIG, None), N.VRQ_EINVAL),
    (lambda L: L.vrq_scan_large(P, 1000, 1024, P, 1, 2000, 0, None, BIG, None), N.VRQ_EINVAL),
    (lambda L: L.vrq_scan_large(P, 1000, 640, P, 1, 2000, 0, P, BIG, None), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_scan_large(P, 1000, 1024, P, 1, 8193, 0, P, BIG, None), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_scan_large(P, 1000, 1024, P, 1, 2000, 8, P, BIG, None), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_scan_large(P, 1000, 1024, P, 1, 2000, N.VRQ_LARGE_STAGE_EMIT, P, 16, None), N.VRQ_EWORKSPACE),
    (lambda L: L.vrq_scan_large(None, 0, 1024, None, 1, 2000, 0, None, 0, None), N.VRQ_OK),
    # zero-size shapes: nothing to do (nq = 0 writes nothing at all)
    (lambda L: hamming(L, nq=0, codes=None, q=None, ws=None, wsb=0), N.VRQ_OK),
    (lambda L: search3(L, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, ws=None, wsb=0), N.VRQ_OK),
    (lambda L: search3(L, nq=0, flags=N.VRQ_SEARCH_PHASE1_ONLY, ob=None, ocos=None, ws=None, wsb=0), N.VRQ_OK),
    (lambda L: search2(L, nq=0, codes=None, q=None, qf=None, qb=None, ws=None, wsb=0), N.VRQ_OK),
])
def test_return_codes(call, expect):
    assert call(N.load()) == expect


@pytest.mark.parametrize("dim", DIMS)
def test_workspace_one_byte_short(dim):
    lib = N.load()
    for n, nq, K in ((20000, 3, 3000), (5, 1, 8192), (1_000_000, 64, 1024)):
        need = lib.vrq_search3_large_workspace_size(n, dim, nq, K)
        assert need > 0
        assert search3(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1) == N.VRQ_EWORKSPACE
        assert search3(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1, flags=N.VRQ_SEARCH_PHASE1_ONLY) == N.VRQ_EWORKSPACE
        assert search2(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1) == N.VRQ_EWORKSPACE
        assert hamming(lib, n=n, cb=dim // 8, nq=nq, k=K, wsb=need - 1) == N.VRQ_EWORKSPACE


@pytest.mark.parametrize("dim", DIMS)
def test_plan_invariants(dim):
    lib = N.load()
    ns = [1, 2, 63, 64, 65, 1000, 4096, 4097, 20000, 262143, 262144, 262145, 1_000_000, 10_000_000, 100_000_000,
          (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    for n in ns:
        for nq in (1, 5, 64, 70, 1024, 5000):
            for K in (1, 1024, 1025, 3000, 8192):
                rc, info = _plan(lib, n, dim, nq, K)
                assert rc == N.VRQ_OK, (n, nq, K)
                chunk_rows, chunks, qpw, prefix, off_cnt, off_tc, off_lists, nbytes = info
                assert chunk_rows > 0 and chunk_rows % 64 == 0 and chunk_rows <= 1 << 30
                assert 1 <= chunks <= 1024 and chunks * chunk_rows >= n and (chunks - 1) * chunk_rows < n
                assert 1 <= qpw <= 16
                assert prefix == 0                                                 # no bounding prefix
                assert 0 <= off_cnt < off_tc < off_lists < nbytes
                assert all(o % 256 == 0 for o in (off_cnt, off_tc, off_lists, nbytes))
                assert off_tc - off_cnt >= min(nq, 512) * chunks * (dim + 1) * 4   # the histograms
                assert off_lists - off_tc >= nq * 8                                # the (T, c_lt) pairs
                assert nbytes - off_lists >= nq * K * 8                            # the K-lists
                assert nbytes == lib.vrq_search3_large_workspace_size(n, dim, nq, K)
                assert nbytes == lib.vrq_search2_large_workspace_size(n, dim, nq, K)
                assert nbytes == lib.vrq_hamming_topk_large_workspace_size(n, dim // 8, nq, K)
                assert _plan(lib, n, dim, nq, K) == (rc, info)  # a pure function of the shape


def test_workspace_size_is_zero_for_unsupported_shapes():
    lib = N.load()
    assert lib.vrq_search3_large_workspace_size(1000, 640, 1, 2000) == 0
    assert lib.vrq_search3_large_workspace_size(1000, 1024, 1, 8193) == 0
    assert lib.vrq_search2_large_workspace_size(1000, 1024, 0, 2000) == 0
    assert lib.vrq_hamming_topk_large_workspace_size(1000, 100, 1, 2000) == 0
    assert lib.vrq_hamming_topk_large_workspace_size(1 << 32, 128, 1, 2000) == 0
    # the histograms of one pass stay bounded however large the batch
    small = lib.vrq_search3_large_workspace_size(100_000_000, 2048, 512, 1025)
    big = lib.vrq_search3_large_workspace_size(100_000_000, 2048, 100_000, 1025)
    assert big - small < 100_000 * (1025 * 28 + 1024 * 16 + 4096)


def test_python_routing_names_the_limit():
    from vectorragquantization_amd.enhanced import search3_call
    assert search3_call(1024) == "vrq_search3_dim" and search3_call(1025) == "vrq_search3_large"
    assert search3_call(8192) == "vrq_search3_large"
    assert search3_call(5000, N.VRQ_SEARCH_SHARD) == "vrq_search3_dim"  # sharding keeps K <= 1024 and its error
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        search3_call(9000)
