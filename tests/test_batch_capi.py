"""The batch entry points (vrq_*_batch: the counting scan with its engine chosen, K1h or K1hm): return codes,
workspace sizes, the engine choice and the plan, the header / loader / library agreement and the wrappers'
routing.  CPU only: every call returns before it would launch anything."""
import ctypes as C
import os
import re

import pytest
import torch

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
P = C.c_void_p(8)    # a non-null, 8-byte aligned pointer that is never dereferenced
ODD = C.c_void_p(12)  # non-null but not 8-byte aligned
BIG = 1 << 40        # workspace bytes no plan exceeds
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrq.h")
NAMES = ("vrq_hamming_topk_batch", "vrq_search3_batch", "vrq_search2_batch", "vrq_scan_batch")
AUTO, VALU, MFMA = N.VRQ_LARGE_ENGINE_AUTO, N.VRQ_LARGE_ENGINE_VALU, N.VRQ_LARGE_ENGINE_MFMA
ENGINES = (AUTO, VALU, MFMA)
SHAPES = ((20000, 3, 3000), (5, 1, 8192), (1_000_000, 64, 1024), (12325, 17, 10), (3_000_000, 600, 2000))


def hamming(L, codes=P, n=1000, cb=128, q=P, nq=2, k=2000, allow=P, od=P, orows=P, ws=P, wsb=BIG, engine=MFMA):
    return L.vrq_hamming_topk_batch(codes, n, cb, 0, q, nq, k, allow, od, orows, ws, wsb, None, engine)


def search3(L, codes=P, x8=P, norms=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, K3=30, flags=0, allow=P,
            oc=P, orows=P, od=P, ob=P, ocos=P, ws=P, wsb=BIG, engine=MFMA):
    return L.vrq_search3_batch(codes, x8, norms, None, n, dim, 0, qf, qb, nq, k, K, K3, flags, allow, oc, orows,
                               od, ob, ocos, ws, wsb, None, engine)


def search2(L, mode=0, codes=P, q=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, flags=0, allow=P, oc=P,
            orows=P, od=P, osc=P, ws=P, wsb=BIG, minmax=None, engine=MFMA):
    return L.vrq_search2_batch(mode, codes, q, minmax, 0.3, None, n, dim, 0, qf, qb, nq, k, K, flags, allow, oc,
                               orows, od, osc, ws, wsb, None, engine)


def scan(L, codes=P, n=1000, dim=1024, qb=P, nq=1, K=2000, stages=0, allow=P, ws=P, wsb=BIG, engine=MFMA):
    return L.vrq_scan_batch(codes, n, dim, qb, nq, K, stages, allow, ws, wsb, None, engine)


# A call that passes every check would launch, which a run without a GPU cannot do: the rows below all stop earlier, the
# accepted null bitmap is shown by the code that FOLLOWS its check (a short workspace, VRQ_EWORKSPACE)
ROWS = [
    # the bitmap: null is an unfiltered call and passes on to the workspace check, misaligned is refused
    (lambda L, e: hamming(L, allow=None, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    (lambda L, e: hamming(L, allow=ODD, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, allow=None, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    (lambda L, e: search3(L, allow=ODD, engine=e), N.VRQ_EINVAL),
    (lambda L, e: search3(L, allow=None, wsb=16, flags=N.VRQ_SEARCH_PHASE1_ONLY, engine=e), N.VRQ_EWORKSPACE),
    (lambda L, e: search2(L, allow=None, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    (lambda L, e: search2(L, allow=ODD, engine=e), N.VRQ_EINVAL),
    (lambda L, e: scan(L, allow=None, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    (lambda L, e: scan(L, allow=ODD, engine=e), N.VRQ_EINVAL),
    (lambda L, e: scan(L, allow=ODD, stages=N.VRQ_LARGE_STAGE_THRESHOLD, engine=e), N.VRQ_EINVAL),
    # ... but only where the *_filtered calls look at their bitmap: an empty or unsupported call never does
    (lambda L, e: hamming(L, k=0, codes=None, q=None, allow=ODD, ws=None, wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: scan(L, n=0, codes=None, qb=None, allow=ODD, ws=None, wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: search3(L, nq=0, allow=ODD, engine=e), N.VRQ_OK),
    (lambda L, e: search2(L, nq=0, allow=ODD, engine=e), N.VRQ_OK),
    (lambda L, e: scan(L, dim=640, allow=ODD, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, K=8193, allow=ODD, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, flags=N.VRQ_SEARCH_SHARD, allow=ODD, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: hamming(L, cb=100, allow=ODD, engine=e), N.VRQ_EUNSUPPORTED),
    # every null pointer of the *_large tables
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
    # K = 0 is an empty call, K past the limit, unsupported dims, n past 2^32 - 1
    (lambda L, e: hamming(L, k=0, codes=None, q=None, allow=None, ws=None, wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: scan(L, K=0, codes=None, qb=None, allow=None, ws=None, wsb=0, engine=e), N.VRQ_OK),
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
    (lambda L, e: hamming(L, n=1 << 32, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search3(L, n=1 << 32, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: search2(L, n=1 << 32, engine=e), N.VRQ_EUNSUPPORTED),
    (lambda L, e: scan(L, n=1 << 32, engine=e), N.VRQ_EUNSUPPORTED),
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
    # short workspace
    (lambda L, e: scan(L, stages=N.VRQ_LARGE_STAGE_EMIT, wsb=16, engine=e), N.VRQ_EWORKSPACE),
    # zero-size shapes: nothing to do (nq = 0 writes nothing at all), and no bitmap is asked for
    (lambda L, e: hamming(L, nq=0, codes=None, q=None, allow=None, ws=None, wsb=0, engine=e), N.VRQ_OK),
    (lambda L, e: search3(L, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, allow=None, ws=None, wsb=0,
                          engine=e), N.VRQ_OK),
    (lambda L, e: search3(L, nq=0, flags=N.VRQ_SEARCH_PHASE1_ONLY, ob=None, ocos=None, allow=None, ws=None, wsb=0,
                          engine=e), N.VRQ_OK),
    (lambda L, e: search2(L, nq=0, codes=None, q=None, qf=None, qb=None, allow=None, ws=None, wsb=0, engine=e),
     N.VRQ_OK),
    (lambda L, e: scan(L, n=0, codes=None, qb=None, allow=None, ws=None, wsb=0, engine=e), N.VRQ_OK),
]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("row", range(len(ROWS)))
def test_return_codes(row, engine):
    call, expect = ROWS[row]
    assert call(N.load(), engine) == expect


@pytest.mark.parametrize("engine", [-1, 3, 99])
def test_a_bad_engine_is_einval(engine):
    lib = N.load()
    assert hamming(lib, engine=engine) == N.VRQ_EINVAL
    assert search3(lib, engine=engine) == N.VRQ_EINVAL
    assert search2(lib, engine=engine) == N.VRQ_EINVAL
    assert scan(lib, engine=engine) == N.VRQ_EINVAL
    assert scan(lib, engine=engine, allow=None) == N.VRQ_EINVAL
    assert lib.vrq_scan_batch_plan(1000, 1024, 1, 2000, engine, (C.c_int64 * 10)()) == N.VRQ_EINVAL


def plan(lib, n, dim, nq, K, engine):
    info = (C.c_int64 * 10)()
    assert lib.vrq_scan_batch_plan(n, dim, nq, K, engine, info) == N.VRQ_OK
    return [int(v) for v in info]


@pytest.mark.parametrize("dim", DIMS)
def test_workspace_covers_either_engine_and_one_byte_short_fails(dim):
    lib = N.load()
    for n, nq, K in SHAPES:
        need = lib.vrq_search3_batch_workspace_size(n, dim, nq, K)
        assert need >= lib.vrq_search3_large_workspace_size(n, dim, nq, K) > 0
        assert lib.vrq_search2_batch_workspace_size(n, dim, nq, K) == need
        assert lib.vrq_scan_batch_workspace_size(n, dim, nq, K) == need
        assert lib.vrq_hamming_topk_batch_workspace_size(n, dim // 8, nq, K) == need
        for e in ENGINES:
            assert plan(lib, n, dim, nq, K, e)[9] == need
            for allow in (P, None):
                assert search3(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1, engine=e, allow=allow) == N.VRQ_EWORKSPACE
                assert search3(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1, flags=N.VRQ_SEARCH_PHASE1_ONLY, engine=e,
                               allow=allow) == N.VRQ_EWORKSPACE
                assert search2(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1, engine=e, allow=allow) == N.VRQ_EWORKSPACE
                assert hamming(lib, n=n, cb=dim // 8, nq=nq, k=K, wsb=need - 1, engine=e, allow=allow) == N.VRQ_EWORKSPACE
                assert scan(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1, engine=e, allow=allow) == N.VRQ_EWORKSPACE


def test_workspace_size_is_zero_for_unsupported_shapes():
    lib = N.load()
    assert lib.vrq_search3_batch_workspace_size(1000, 640, 1, 2000) == 0
    assert lib.vrq_search3_batch_workspace_size(1000, 1024, 1, 8193) == 0
    assert lib.vrq_search2_batch_workspace_size(1000, 1024, 0, 2000) == 0
    assert lib.vrq_scan_batch_workspace_size(0, 1024, 1, 2000) == 0
    assert lib.vrq_hamming_topk_batch_workspace_size(1000, 100, 1, 2000) == 0
    assert lib.vrq_hamming_topk_batch_workspace_size(1 << 32, 128, 1, 2000) == 0


@pytest.mark.parametrize("dim", DIMS)
def test_engine_choice_and_plan_are_pure_and_consistent(dim):
    lib = N.load()
    for n, nq, K in SHAPES + ((100_000_000, 1024, 8192), ((1 << 32) - 1, 512, 100)):
        need = lib.vrq_scan_batch_workspace_size(n, dim, nq, K)
        for filtered in (0, 1):
            e = lib.vrq_large_engine(n, dim, nq, K, filtered)
            assert e in (VALU, MFMA) and lib.vrq_large_engine(n, dim, nq, K, filtered) == e
            assert e == lib.vrq_large_engine(n, dim, nq, K, 0)   # the plan call has no filter axis: neither has AUTO
        auto = plan(lib, n, dim, nq, K, AUTO)
        assert auto == plan(lib, n, dim, nq, K, AUTO)
        assert auto[0] == lib.vrq_large_engine(n, dim, nq, K, 0) and auto == plan(lib, n, dim, nq, K, auto[0])
        # engine VALU: vrq_scan_large_plan's chunks, offsets and workgroup
        large = (C.c_int64 * 8)()
        assert lib.vrq_scan_large_plan(n, dim, nq, K, large) == N.VRQ_OK
        v = plan(lib, n, dim, nq, K, VALU)
        assert v[0] == VALU and v[1:4] == [large[0], large[1], large[2]] and v[5] == 0
        assert v[6:9] == [large[4], large[5], large[6]] and v[9] == need >= large[7]
        # engine MFMA
        m = plan(lib, n, dim, nq, K, MFMA)
        eng, rows, chunks, qpw, nqb, flush, off_hist, off_tc, off_lists, nbytes = m
        assert eng == MFMA and nbytes == need
        assert rows % 64 == 0 and rows >= 64 and 1 <= chunks <= 1024
        assert (chunks - 1) * rows < n <= chunks * rows
        assert qpw in (16, 32, 64) and (qpw == 16) == (dim == 2048)
        qb = min(nq, 512)
        assert nqb == -(-qb // qpw)
        # the 16-bit bins: a flush at the latest every 65535 rows, none asked for where a chunk is shorter
        # (a bin takes at most one count per row, so neither a flushed nor an unflushed bin can pass 65535)
        assert 0 <= flush < 65536 and flush % 64 == 0
        assert flush or rows < 65536
        if flush:
            assert rows > flush
        # the layout: histograms of one pass, then T / c_lt pairs, then K-lists, all inside the workspace
        hist = qb * chunks * (dim + 1) * 4
        assert off_hist == 0 and off_tc >= hist + nq * chunks * 16 and off_lists >= off_tc + nq * 8
        assert off_lists + nq * K * 8 <= nbytes


def test_plan_rejects_what_the_calls_reject():
    lib = N.load()
    info = (C.c_int64 * 10)()
    assert lib.vrq_scan_batch_plan(0, 1024, 1, 10, MFMA, info) == N.VRQ_EINVAL
    assert lib.vrq_scan_batch_plan(10, 1024, 1, 10, MFMA, None) == N.VRQ_EINVAL
    assert lib.vrq_scan_batch_plan(10, 640, 1, 10, MFMA, info) == N.VRQ_EUNSUPPORTED
    assert lib.vrq_scan_batch_plan(10, 1024, 1, 8193, MFMA, info) == N.VRQ_EUNSUPPORTED
    assert lib.vrq_scan_batch_plan(1 << 32, 1024, 1, 10, MFMA, info) == N.VRQ_EUNSUPPORTED
    assert lib.vrq_large_engine(0, 1024, 1, 10, 0) == N.VRQ_EINVAL
    assert lib.vrq_large_engine(10, 640, 1, 10, 0) == N.VRQ_EUNSUPPORTED
    assert lib.vrq_large_engine(10, 1024, 1, 8193, 1) == N.VRQ_EUNSUPPORTED


def test_header_loader_and_library_agree():
    src = open(HDR).read()
    raw = C.CDLL(N.lib_path())
    for sym in ("vrq_large_engine", "vrq_scan_batch_plan"):
        assert re.search(r"\b" + sym + r"\s*\(", src) and sym in N.SIGNATURES and hasattr(raw, sym), sym
    for name, value in (("AUTO", 0), ("VALU", 1), ("MFMA", 2)):
        assert re.search(r"#define VRQ_LARGE_ENGINE_%s %d\b" % (name, value), src)
        assert getattr(N, "VRQ_LARGE_ENGINE_" + name) == value
    for name in NAMES:
        for sym in (name, name + "_workspace_size"):
            assert re.search(r"\b" + sym + r"\s*\(", src), sym
            assert sym in N.SIGNATURES, sym
            assert hasattr(raw, sym), sym
        # one argument more than the *_filtered call: the engine, an int32 at the end
        filt = N.SIGNATURES[name.replace("_batch", "_filtered")]
        res, args = N.SIGNATURES[name]
        assert res is filt[0] and list(args) == list(filt[1]) + [C.c_int32]
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", src)
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert params[-1] == "int32_t engine" and "const uint64_t* allow" in params and len(params) == len(args)
        assert N.SIGNATURES[name + "_workspace_size"] == N.SIGNATURES["vrq_search3_large_workspace_size"]


# ---- the wrappers' routing ----
def test_routing_helpers_name_the_call_of_each_engine():
    allow = torch.zeros(1, dtype=torch.int64)
    for base in ("vrq_search3", "vrq_search2", "vrq_hamming_topk"):
        for K in (10, 5000):
            for a in (None, allow):
                for engine in ("auto", "mfma", "valu"):
                    assert N.batch_call(base, engine, K, 0, a) == base + "_batch"
                    assert hasattr(N.load(), base + "_batch_workspace_size")
        # engine=None: today's names
        assert N.batch_call(base, None, 10) == base and N.batch_call(base, None, 5000) == base + "_large"
        assert N.batch_call(base, None, 10, 0, allow) == N.batch_call(base, None, 5000, 0, allow) == base + "_filtered"
    assert N.batch_engine(None, 10 ** 6, N.VRQ_SEARCH_SHARD, "x") is None   # None never looks at K or flags
    assert [N.batch_engine(e, 10, N.VRQ_SEARCH_PHASE1_ONLY, "x") for e in ("auto", "valu", "mfma")] == [AUTO, VALU, MFMA]
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        N.batch_engine("mfma", 9000, 0, "x")
    with pytest.raises(N.VrqNativeError, match="engine"):
        N.batch_engine("fast", 10, 0, "x")
    for flag in (N.VRQ_SEARCH_SHARD, N.VRQ_SEARCH_SCAN_MFMA, N.VRQ_SEARCH_SCAN_VALU):
        with pytest.raises(N.VrqNativeError, match="engine"):
            N.batch_engine("auto", 10, flag, "x")


def test_search3_call_answers_as_before():
    from vectorragquantization_amd.enhanced import search3_call
    allow = torch.zeros(1, dtype=torch.int64)
    assert search3_call(10) == "vrq_search3_dim" and search3_call(5000) == "vrq_search3_large"
    assert search3_call(10, 0, allow) == search3_call(5000, 0, allow) == "vrq_search3_filtered"


def test_wrappers_raise_before_any_launch():
    """K past the limit, an unknown engine and the scan flags raise in the wrappers, on CPU tensors: nothing is
    launched."""
    from vectorragquantization_amd import quant as Q
    from vectorragquantization_amd.enhanced import search3
    n, d = 9000, 256
    codes = torch.zeros((n, d // 8), dtype=torch.uint8)
    qf, qb = torch.zeros((1, d)), torch.zeros((1, d // 8), dtype=torch.uint8)
    allow = torch.zeros((n + 63) // 64, dtype=torch.int64)
    for a in (None, allow):
        with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
            Q.search2("sbin", codes, codes, qf, qb, 900, 10, allow=a, engine="mfma")
        with pytest.raises(N.VrqNativeError, match="engine"):
            Q.search2("sbin", codes, codes, qf, qb, 10, 10, flags=N.VRQ_SEARCH_SCAN_VALU, allow=a, engine="auto")
        with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
            Q.vectordb_search("bin16", codes, None, None, qb, 900, 10, allow=a, engine="valu")
        with pytest.raises(N.VrqNativeError, match="engine"):
            Q.vectordb_search("bin16", codes, None, None, qb, 9, 10, allow=a, engine="matrix")
        x8, norms = torch.zeros((n, d), dtype=torch.int8), torch.zeros(n, dtype=torch.float64)
        with pytest.raises(N.VrqNativeError, match="engine"):
            search3(codes, x8, norms, qf, qb, 10, 100, 30, N.VRQ_SEARCH_SHARD, allow=a, engine="mfma")
        with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
            search3(codes, x8, norms, qf, qb, 10, 9000, 30, N.VRQ_SEARCH_PHASE1_ONLY, allow=a, engine="mfma")
    with pytest.raises(N.VrqNativeError, match="words"):
        Q.search2("sbin", codes, codes, qf, qb, 10, 10, allow=allow[:-1], engine="mfma")
