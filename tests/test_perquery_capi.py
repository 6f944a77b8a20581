"""The per-query entry points (vrq_*_perquery: the *_batch calls with a set of bitmaps and one set id per query):
return codes and the header / loader / library agreement.  CPU only: every call returns before it would launch
anything -- an accepted filter is shown by the check that FOLLOWS it (a short workspace, VRQ_EWORKSPACE)."""
import ctypes as C
import os
import re

import pytest

from vectorragquantization_amd import _native as N

P = C.c_void_p(8)     # a non-null, 8-byte aligned pointer that is never dereferenced
ODD = C.c_void_p(12)  # non-null, 4-byte but not 8-byte aligned
ODD2 = C.c_void_p(10)  # non-null, not 4-byte aligned
BIG = 1 << 40         # workspace bytes no plan exceeds
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrq.h")
NAMES = ("vrq_hamming_topk_perquery", "vrq_search3_perquery", "vrq_search2_perquery", "vrq_scan_perquery")
AUTO, VALU, MFMA = N.VRQ_LARGE_ENGINE_AUTO, N.VRQ_LARGE_ENGINE_VALU, N.VRQ_LARGE_ENGINE_MFMA
ENGINES = (AUTO, VALU, MFMA)
W1000 = 16  # ceil(1000 / 64)


def hamming(L, codes=P, n=1000, cb=128, q=P, nq=2, k=2000, allow=P, od=P, orows=P, ws=P, wsb=BIG, engine=MFMA,
            nsets=3, sw=W1000, qs=P):
    return L.vrq_hamming_topk_perquery(codes, n, cb, 0, q, nq, k, allow, od, orows, ws, wsb, None, engine, nsets, sw,
                                       qs)


def search3(L, codes=P, x8=P, norms=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, K3=30, flags=0, allow=P,
            oc=P, orows=P, od=P, ob=P, ocos=P, ws=P, wsb=BIG, engine=MFMA, nsets=3, sw=W1000, qs=P):
    return L.vrq_search3_perquery(codes, x8, norms, None, n, dim, 0, qf, qb, nq, k, K, K3, flags, allow, oc, orows,
                                  od, ob, ocos, ws, wsb, None, engine, nsets, sw, qs)


def search2(L, mode=0, codes=P, q=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, flags=0, allow=P, oc=P,
            orows=P, od=P, osc=P, ws=P, wsb=BIG, minmax=None, engine=MFMA, nsets=3, sw=W1000, qs=P):
    return L.vrq_search2_perquery(mode, codes, q, minmax, 0.3, None, n, dim, 0, qf, qb, nq, k, K, flags, allow, oc,
                                  orows, od, osc, ws, wsb, None, engine, nsets, sw, qs)


def scan(L, codes=P, n=1000, dim=1024, qb=P, nq=1, K=2000, stages=0, allow=P, ws=P, wsb=BIG, engine=MFMA, nsets=3,
         sw=W1000, qs=P):
    return L.vrq_scan_perquery(codes, n, dim, qb, nq, K, stages, allow, ws, wsb, None, engine, nsets, sw, qs)


CALLS = (hamming, search3, search2, scan)

# the VRQ_EINVAL rows of the filter, for each of the four calls
FILTER_EINVAL = [
    dict(allow=None),       # a null allow
    dict(qs=None),          # a null query_set
    dict(allow=ODD),        # allow not 8-byte aligned
    dict(qs=ODD2),          # query_set not 4-byte aligned
    dict(nsets=0),          # nsets < 1
    dict(nsets=-3),
    dict(sw=W1000 - 1),     # set_words < ceil(n / 64)
    dict(sw=0),
    dict(sw=-1),
]
# ... and filters that are accepted: only the workspace stops these
FILTER_OK = [
    dict(),
    dict(qs=ODD),                 # 4-byte aligned is enough for query_set
    dict(nsets=1),
    dict(sw=W1000 + 3),           # bitmaps sized for capacity
    dict(sw=1 << 40, nsets=1 << 30),  # 64-bit index arithmetic: nothing overflows a check
]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("row", range(len(FILTER_EINVAL)))
def test_filter_einval(row, call, engine):
    assert call(N.load(), engine=engine, **FILTER_EINVAL[row]) == N.VRQ_EINVAL
    # the filter is checked before the workspace size: a short workspace does not mask it
    assert call(N.load(), engine=engine, wsb=16, **FILTER_EINVAL[row]) == N.VRQ_EINVAL


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("row", range(len(FILTER_OK)))
def test_an_accepted_filter_reaches_the_workspace_check(row, call, engine):
    assert call(N.load(), engine=engine, wsb=16, **FILTER_OK[row]) == N.VRQ_EWORKSPACE


def test_set_words_is_measured_against_n():
    lib = N.load()
    for n in (1, 63, 64, 65, 12325):
        w = (n + 63) // 64
        for call, kw in ((hamming, dict(k=1)), (search3, dict(K=1, k=1)), (search2, dict(K=1, k=1)), (scan, dict(K=1))):
            assert call(lib, n=n, sw=w, wsb=16, **kw) == N.VRQ_EWORKSPACE
            assert call(lib, n=n, sw=w - 1, wsb=16, **kw) == N.VRQ_EINVAL


# the null-pointer, unsupported-shape and empty-call rows of the *_batch tables
ROWS = [
    # an empty or unsupported call never looks at the filter
    (lambda L, e: hamming(L, k=0, codes=None, q=None, allow=ODD, qs=None, nsets=0, sw=0, ws=None, wsb=0, engine=e),
     N.VRQ_OK),
    (lambda L, e: scan(L, n=0, codes=None, qb=None, allow=None, qs=None, nsets=0, sw=0, ws=None, wsb=0, engine=e),
     N.VRQ_OK),
    (lambda L, e: scan(L, K=0, codes=None, qb=None, allow=None, qs=ODD2, ws=None, wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: search3(L, nq=0, allow=ODD, qs=None, engine=e), N.VRQ_OK),
    (lambda L, e: search2(L, nq=0, allow=ODD, qs=ODD2, nsets=-1, sw=-1, engine=e), N.VRQ_OK),
    (lambda L, e: scan(L, dim=640, allow=ODD, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, K=8193, allow=ODD, qs=None, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, flags=N.VRQ_SEARCH_SHARD, allow=ODD, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: hamming(L, cb=100, allow=ODD, engine=e), N.VRQ_EUNSUPPORTED),
    # every null pointer of the *_batch tables
    (lambda L, e: hamming(L, codes=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: hamming(L, q=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: hamming(L, od=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: hamming(L, orows=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: hamming(L, ws=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, codes=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, x8=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, norms=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, qf=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, qb=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, oc=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, orows=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, od=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, ob=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, ocos=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, ws=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, n=-1, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, K3=-1, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search2(L, codes=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search2(L, q=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search2(L, qf=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search2(L, qb=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search2(L, osc=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search2(L, ws=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search2(L, mode=3, engine=e), N.VRQ_EINVAL),   # a local mode without minmax
    (lambda L, e: search2(L, mode=99, engine=e), N.VRQ_EINVAL),
    (lambda L, e: scan(L, codes=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: scan(L, qb=None, engine=e), N.VRQ_EINVAL),
    (lambda L, e: scan(L, ws=None, engine=e), N.VRQ_EINVAL),
    # K past the limit, unsupported dims, n past 2^32 - 1
    (lambda L, e: hamming(L, k=8193, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, K=8193, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, k=8193, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, K=8193, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, k=8193, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: scan(L, K=8193, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: hamming(L, cb=100, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, dim=640, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, dim=640, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: scan(L, dim=640, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: hamming(L, n=1 << 32, sw=1 << 26, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, n=1 << 32, sw=1 << 26, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, n=1 << 32, sw=1 << 26, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: scan(L, n=1 << 32, sw=1 << 26, engine=e), N.VRQ_EUNSUPPORTED),
    # K <= 1024 is this path's too: only the workspace stops these
    (lambda L, e: hamming(L, k=10, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    (lambda L, e: search3(L, K=10, k=1, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    # flags outside the allowed set: the scan flags and the sharded mode
    (lambda L, e: search3(L, flags=N.VRQ_SEARCH_SHARD, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, flags=N.VRQ_SEARCH_SCAN_MFMA, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, flags=N.VRQ_SEARCH_SCAN_VALU, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, flags=N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SCAN_STAGE_SUFFIX, engine=e),
     N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, flags=N.VRQ_SEARCH_PHASE1_ONLY, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, flags=N.VRQ_SEARCH_SHARD, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, flags=N.VRQ_SEARCH_SCAN_MFMA, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, flags=N.VRQ_SEARCH_SCAN_VALU, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: scan(L, stages=8, engine=e), N.VRQ_EUNSUPPORTED),
    # short workspace, with the accepted flags and stage masks
    (lambda L, e: scan(L, stages=N.VRQ_LARGE_STAGE_EMIT, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    (lambda L, e: search3(L, flags=N.VRQ_SEARCH_PHASE1_ONLY, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    # zero-size shapes: nothing to do (nq = 0 writes nothing at all), and neither array is asked for
    (lambda L, e: hamming(L, nq=0, codes=None, q=None, allow=None, qs=None, ws=None, wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: search3(L, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, allow=None, qs=None, ws=None,
                          wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: search3(L, nq=0, flags=N.VRQ_SEARCH_PHASE1_ONLY, ob=None, ocos=None, allow=None, qs=None, ws=None,
                          wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: search2(L, nq=0, codes=None, q=None, qf=None, qb=None, allow=None, qs=None, ws=None, wsb=0,
                          engine=e), N.VRQ_OK),
    (lambda L, e: scan(L, n=0, codes=None, qb=None, allow=None, qs=None, ws=None, wsb=0, engine=e), N.VRQ_OK),
]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("row", range(len(ROWS)))
def test_return_codes(row, engine):
    call, expect = ROWS[row]
    assert call(N.load(), engine) == expect


@pytest.mark.parametrize("engine", [-1, 3, 99])
def test_a_bad_engine_is_einval(engine):
    lib = N.load()
    for call in CALLS:
        assert call(lib, engine=engine) == N.VRQ_EINVAL


@pytest.mark.parametrize("dim", (256, 384, 1024, 2048))
def test_the_workspace_is_the_batch_calls_and_one_byte_short_fails(dim):
    lib = N.load()
    for n, nq, K in ((20000, 3, 3000), (12325, 520, 10), (1_000_000, 64, 1024)):
        need = lib.vrq_search3_batch_workspace_size(n, dim, nq, K)
        w = (n + 63) // 64
        assert need > 0
        for e in ENGINES:
            kw = dict(n=n, nq=nq, wsb=need - 1, engine=e, sw=w + 3, nsets=5)
            assert search3(lib, dim=dim, K=K, **kw) == N.VRQ_EWORKSPACE
            assert search3(lib, dim=dim, K=K, flags=N.VRQ_SEARCH_PHASE1_ONLY, **kw) == N.VRQ_EWORKSPACE
            assert search2(lib, dim=dim, K=K, **kw) == N.VRQ_EWORKSPACE
            assert hamming(lib, cb=dim // 8, k=K, **kw) == N.VRQ_EWORKSPACE
            assert scan(lib, dim=dim, K=K, **kw) == N.VRQ_EWORKSPACE


def test_header_loader_and_library_agree():
    src = open(HDR).read()
    raw = C.CDLL(N.lib_path())
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in N.SIGNATURES, name
        assert hasattr(raw, name), name
        assert not hasattr(raw, name + "_workspace_size")  # no new size functions
        # the *_batch prototype followed by int32 nsets, int64 set_words, const int32* query_set
        batch = N.SIGNATURES[name.replace("_perquery", "_batch")]
        res, args = N.SIGNATURES[name]
        assert res is batch[0] and list(args) == list(batch[1]) + [C.c_int32, C.c_int64, C.c_void_p]

        def params(sym):
            m = re.search(r"\bint " + sym + r"\s*\(([^;]*)\);", src)
            return [" ".join(p.split()) for p in m.group(1).replace("\n", " ").split(",")]
        assert params(name) == params(name.replace("_perquery", "_batch")) + [
            "int32_t nsets", "int64_t set_words", "const int32_t* query_set"]
        assert len(params(name)) == len(args)
    assert N.load().vrq_abi_version() == 1
