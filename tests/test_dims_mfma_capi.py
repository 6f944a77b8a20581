"""Host-only contract of the matrix-core Phase-I scan at the embedding dims other than 1024 (K1rd):
which scan a shape takes, the plan and the sample plan, workspace sizes, and the argument validation of
vrq_search3_dim_scan / vrq_search3_dim_finish that returns before any device work.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1536, 2048)
NQS = (1, 40, 128, 129, 1024)
P8 = C.c_void_p(8)  # a non-null pointer that validation must never dereference
N_ROWS = 200_000
INT_MAX = 2**31 - 1
# The smallest batch at which the matrix scan is the default, per dim (DESIGN section 5 "K1rd", measured in
# profiles/dim_mfma_bench.jsonl); INT_MAX: forced only.
MIN_QUERIES = {256: 1, 384: 1, 512: 1, 768: 1, 1536: 1, 2048: 1}


def _kind(lib, n, d, nq, K, flags):
    return lib.vrq_scan_kind(n, d, nq, K, flags, None)


@pytest.mark.parametrize("d", DIMS)
def test_scan_kind(d):
    lib = N.load()
    assert _kind(lib, N_ROWS, d, 64, 100, N.VRQ_SEARCH_SCAN_MFMA) == N.VRQ_SCAN_KIND_MFMA
    assert _kind(lib, N_ROWS, d, 64, 100, N.VRQ_SEARCH_SCAN_VALU) == N.VRQ_SCAN_KIND_VALU
    assert _kind(lib, N_ROWS, d, 64, 100, N.VRQ_SEARCH_SCAN_VALU | N.VRQ_SEARCH_SCAN_MFMA) == N.VRQ_SCAN_KIND_VALU
    assert _kind(lib, N_ROWS, d, 64, 129, N.VRQ_SEARCH_SCAN_MFMA) == N.VRQ_SCAN_KIND_VALU
    assert _kind(lib, 65_535, d, 64, 100, N.VRQ_SEARCH_SCAN_MFMA) == N.VRQ_SCAN_KIND_VALU
    assert _kind(lib, 65_536, d, 64, 100, N.VRQ_SEARCH_SCAN_MFMA) == N.VRQ_SCAN_KIND_MFMA
    pr = C.c_int64(-1)
    assert lib.vrq_scan_kind(N_ROWS, d, 64, 100, N.VRQ_SEARCH_SCAN_MFMA, C.byref(pr)) == N.VRQ_SCAN_KIND_MFMA
    assert pr.value == 0
    assert lib.vrq_scan_kind(N_ROWS, d, 64, 100, N.VRQ_SEARCH_SCAN_VALU, C.byref(pr)) == N.VRQ_SCAN_KIND_VALU
    assert pr.value == N_ROWS
    assert _kind(lib, N_ROWS, d, 64, 2000, 0) == N.VRQ_EUNSUPPORTED
    assert _kind(lib, 0, d, 64, 100, 0) == N.VRQ_EINVAL


@pytest.mark.parametrize("d", DIMS)
def test_default_choice_is_the_documented_table(d):
    """Without a forcing flag: the matrix scan from min_queries[dim] up (monotone in nq), never below the
    row minimum or above K = 128."""
    lib = N.load()
    kinds = [_kind(lib, N_ROWS, d, nq, 100, 0) for nq in range(1, 1100)]
    assert all(a <= b for a, b in zip(kinds, kinds[1:])), "the default choice must be monotone in nq"
    want = [N.VRQ_SCAN_KIND_MFMA if nq >= MIN_QUERIES[d] else N.VRQ_SCAN_KIND_VALU for nq in range(1, 1100)]
    assert kinds == want
    assert _kind(lib, 65_535, d, 1024, 100, 0) == N.VRQ_SCAN_KIND_VALU
    assert _kind(lib, N_ROWS, d, 1024, 129, 0) == N.VRQ_SCAN_KIND_VALU


def _plan(lib, n, d, nq, K, flags=N.VRQ_SEARCH_SCAN_MFMA):
    info = np.full(12, -1, np.int64)
    assert lib.vrq_scan_plan(n, d, nq, K, flags, info.ctypes.data) == N.VRQ_OK
    return info


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("nq", NQS)
def test_plan(d, nq):
    lib = N.load()
    K, n = 100, N_ROWS
    info = _plan(lib, n, d, nq, K)
    kind, mb, cr, nch, capc, off_cand, off_cnt, off_tau, sample, j, off_suffix, total = (int(x) for x in info)
    assert kind == N.VRQ_SCAN_PLAN_K1RD == 3
    assert mb == (1 if nq <= 32 else 2 if nq <= 64 or d >= 1536 else 4)
    assert cr % 64 == 0 and cr * nch >= n and cr * (nch - 1) < n
    assert capc >= 64 and capc & (capc - 1) == 0
    assert 0 < off_suffix < off_cand < off_cnt < off_tau < total
    assert all(o % 256 == 0 for o in (off_suffix, off_cand, off_cnt, off_tau))
    assert off_cand - off_suffix >= nq * K * 8 and off_cnt - off_cand >= nq * nch * capc * 8
    assert off_tau - off_cnt >= nq * nch * 4
    assert 1 <= j <= K and sample <= n
    assert total <= lib.vrq_search3_dim_workspace_size(n, d, nq, K)
    assert total <= lib.vrq_hamming_topk_workspace_size(n, d // 8, nq, K)
    sp = np.full(6, -1, np.int64)
    assert lib.vrq_scan_sample_plan(n, d, nq, K, N.VRQ_SEARCH_SCAN_MFMA, sp.ctypes.data) == N.VRQ_OK
    rows_sample, nsc, scr, sstride, ts, cols = (int(x) for x in sp)
    assert rows_sample == 1 and scr % 64 == 0 and ts >= 64
    assert sstride == (scr // 64) * ts and cols == 32 * nsc and sample == nsc * scr
    assert nsc >= 8 and sample > 65_536 - scr        # fewer than one chunk's tiles short of the 65 536-row minimum
    assert off_suffix >= nq * cols * 2
    last_tile = (nsc * (scr // 64) - 1) * ts
    assert 0 <= last_tile and last_tile + 64 <= n
    # pure functions of the call shape
    assert np.array_equal(info, _plan(lib, n, d, nq, K))
    sp2 = np.full(6, -1, np.int64)
    assert lib.vrq_scan_sample_plan(n, d, nq, K, N.VRQ_SEARCH_SCAN_MFMA, sp2.ctypes.data) == N.VRQ_OK
    assert np.array_equal(sp, sp2)


def test_sampled_order_is_live_at_the_test_size():
    """n = 300 007, K = 100: the sample is 65 536 rows and the sampled order j < K (the GPU tests rely on it)."""
    lib = N.load()
    for d in DIMS:
        info = _plan(lib, 300_007, d, 40, 100)
        assert int(info[8]) == 65_536 and int(info[9]) < 100


def test_plan_refused_where_the_wavefront_scan_runs():
    lib = N.load()
    info = np.zeros(12, np.int64)
    for d in DIMS:
        assert lib.vrq_scan_plan(N_ROWS, d, 64, 100, N.VRQ_SEARCH_SCAN_VALU, info.ctypes.data) == N.VRQ_EUNSUPPORTED
        assert lib.vrq_scan_plan(1000, d, 64, 100, N.VRQ_SEARCH_SCAN_MFMA, info.ctypes.data) == N.VRQ_EUNSUPPORTED
        assert lib.vrq_scan_sample_plan(N_ROWS, d, 64, 129, N.VRQ_SEARCH_SCAN_MFMA,
                                        info.ctypes.data) == N.VRQ_EUNSUPPORTED
        assert lib.vrq_scan_plan(N_ROWS, d, 64, 100, N.VRQ_SEARCH_SCAN_MFMA, None) == N.VRQ_EINVAL
    assert lib.vrq_scan_plan(N_ROWS, 1032, 64, 100, N.VRQ_SEARCH_SCAN_MFMA, info.ctypes.data) == N.VRQ_EUNSUPPORTED


def test_workspace_sizes():
    lib = N.load()
    for d in DIMS:
        small = lib.vrq_search3_dim_workspace_size(1000, d, 1, 10)   # below the row minimum: the chunk lists
        assert small > 0 and small % 80 == 0
        assert lib.vrq_hamming_topk_workspace_size(1000, d // 8, 1, 10) == small
        for nq in NQS:
            a = lib.vrq_search3_dim_workspace_size(N_ROWS, d, nq, 100)
            assert a == lib.vrq_hamming_topk_workspace_size(N_ROWS, d // 8, nq, 100)
            assert a >= int(_plan(lib, N_ROWS, d, nq, 100)[11])
        # K > 128: the wavefront scan's lists only (a multiple of nq * K * 8)
        assert lib.vrq_search3_dim_workspace_size(N_ROWS, d, 2, 200) % (2 * 200 * 8) == 0


def _scan(L, dim=384, n=N_ROWS, nq=4, K=10, flags=0, codes=P8, qb=P8, ws=P8, ws_bytes=1 << 40):
    return L.vrq_search3_dim_scan(codes, n, dim, qb, nq, K, flags, ws, ws_bytes, None)


def _finish(L, dim=384, n=N_ROWS, nq=4, K=10, flags=N.VRQ_SEARCH_PHASE1_ONLY, codes=P8, outs=P8, ws=P8,
            ws_bytes=1 << 40):
    return L.vrq_search3_dim_finish(codes, None, None, None, n, dim, 0, None, nq, 1, K, 1, flags, outs, outs, outs,
                                    None, None, ws, ws_bytes, None)


MF = N.VRQ_SEARCH_SCAN_MFMA


@pytest.mark.parametrize("call,expect", [
    (lambda L: _scan(L, codes=None), N.VRQ_EINVAL),
    (lambda L: _scan(L, qb=None), N.VRQ_EINVAL),
    (lambda L: _scan(L, ws=None), N.VRQ_EINVAL),
    (lambda L: _scan(L, n=-1), N.VRQ_EINVAL),
    (lambda L: _scan(L, dim=1032), N.VRQ_EUNSUPPORTED),
    (lambda L: _scan(L, dim=4096), N.VRQ_EUNSUPPORTED),
    (lambda L: _scan(L, K=2000), N.VRQ_EUNSUPPORTED),
    (lambda L: _scan(L, flags=N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: _scan(L, flags=MF | N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: _scan(L, flags=MF, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _scan(L, flags=MF | N.VRQ_SCAN_STAGE_PREFIX, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _scan(L, flags=N.VRQ_SEARCH_SCAN_VALU, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _scan(L, nq=0, codes=None), N.VRQ_OK),
    (lambda L: _scan(L, n=0, codes=None), N.VRQ_OK),
    (lambda L: _scan(L, dim=1024, K=2000), N.VRQ_EUNSUPPORTED),          # 1024 forwards
    (lambda L: _scan(L, dim=1024, flags=MF, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _finish(L, outs=None), N.VRQ_EINVAL),
    (lambda L: _finish(L, codes=None), N.VRQ_EINVAL),
    (lambda L: _finish(L, ws=None), N.VRQ_EINVAL),
    (lambda L: _finish(L, flags=0), N.VRQ_EINVAL),                        # full mode needs the score outputs
    (lambda L: _finish(L, dim=1032), N.VRQ_EUNSUPPORTED),
    (lambda L: _finish(L, K=2000), N.VRQ_EUNSUPPORTED),
    (lambda L: _finish(L, flags=N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: _finish(L, flags=N.VRQ_SEARCH_PHASE1_ONLY | MF, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _finish(L, flags=N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_VALU, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _finish(L, nq=0), N.VRQ_OK),
    (lambda L: _finish(L, dim=1024, K=2000), N.VRQ_EUNSUPPORTED),        # 1024 forwards
    (lambda L: _finish(L, dim=1024, flags=N.VRQ_SEARCH_PHASE1_ONLY | MF, ws_bytes=16), N.VRQ_EWORKSPACE),
])
def test_argument_validation(call, expect):
    assert call(N.load()) == expect


def test_1024_is_unchanged():
    """At 1024 the introspection and the sizes are those of the 1024 path: kinds 0 / 1 / 2, never 3."""
    lib = N.load()
    for n, nq, K, want in ((1_000_000, 8, 100, (1, 1)), (1_000_000, 128, 100, (1, 4)), (1_000_000, 256, 100, (0, 2)),
                           (1_000_000, 1024, 100, (2, 4))):
        info = _plan(lib, n, 1024, nq, K, 0)
        assert (int(info[0]), int(info[1])) == want
        assert _kind(lib, n, 1024, nq, K, 0) == N.VRQ_SCAN_KIND_MFMA
        assert int(info[11]) <= lib.vrq_search3_dim_workspace_size(n, 1024, nq, K) \
            == lib.vrq_search3_workspace_size(n, 1024, nq, K)
    assert _kind(lib, 1000, 1024, 8, 100, 0) == N.VRQ_SCAN_KIND_VALU
