"""Host-only contract of the exhaustive top-k entry points at every embedding dim
(vrq_gemm_topk_dim, vrq_flat_ip_topk_dim, vrq_gemm_topk_dim_workspace_size, vrq_gemm_topk_dim_plan):
the symbols, workspace sizes, K5d's plan and the argument validation that returns before any device
work.  CPU only."""
import ctypes as C

import pytest

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1536, 2048)
MODES = (N.VRQ_GEMM_BINARY, N.VRQ_GEMM_INT8_COSINE, N.VRQ_GEMM_FLOAT_IP)
P8 = C.c_void_p(8)  # a non-null pointer that validation must never dereference


def _plan(L, mode, n, dim, nq, k):
    info = (C.c_int64 * 6)()
    rc = L.vrq_gemm_topk_dim_plan(mode, n, dim, nq, k, info)
    return rc, [int(v) for v in info]


def test_symbols_and_flag():
    lib = N.load()
    for name in ("vrq_gemm_topk_dim_workspace_size", "vrq_gemm_topk_dim_plan", "vrq_gemm_topk_dim",
                 "vrq_flat_ip_topk_dim"):
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert N.VRQ_GEMM_SCAN_EXACT == 256
    stage = N.VRQ_GEMM_STAGE_SAMPLE | N.VRQ_GEMM_STAGE_MAIN | N.VRQ_GEMM_STAGE_FINISH | N.VRQ_GEMM_NO_FALLBACK
    assert N.VRQ_GEMM_SCAN_EXACT & stage == 0


def test_workspace_sizes():
    lib = N.load()
    for mode in MODES:
        for n, nq, k in ((1000, 1, 10), (1_000_000, 1024, 100)):
            assert (lib.vrq_gemm_topk_dim_workspace_size(mode, n, 1024, nq, k)
                    == lib.vrq_gemm_topk_workspace_size(mode, n, 1024, nq, k) > 0)
        for d in DIMS:
            assert lib.vrq_gemm_topk_dim_workspace_size(mode, 1000, d, 1, 10) > 0, (mode, d)
        assert lib.vrq_gemm_topk_dim_workspace_size(mode, 1000, 1032, 1, 10) == 0
        assert lib.vrq_gemm_topk_dim_workspace_size(mode, 1000, 384, 1, 2000) == 0
        assert lib.vrq_gemm_topk_dim_workspace_size(mode, 1 << 32, 384, 1, 10) == 0
        assert _plan(lib, mode, 1000, 1032, 1, 10)[0] == N.VRQ_EUNSUPPORTED
        assert _plan(lib, mode, 1000, 384, 1, 2000)[0] == N.VRQ_EUNSUPPORTED
    assert lib.vrq_gemm_topk_dim_workspace_size(7, 1000, 384, 1, 10) == 0   # not a mode
    # the ABI-1 function keeps refusing the other dims
    assert lib.vrq_gemm_topk_workspace_size(N.VRQ_GEMM_BINARY, 1000, 384, 1, 10) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dim", DIMS + (1024,))
def test_plan_fields(mode, dim):
    lib = N.load()
    for n, nq, k in ((1, 1, 1), (63, 3, 10), (64, 9, 10), (5000, 3, 1024), (200_000, 9, 10), (10_000_000, 1024, 10),
                     (10_000_000, 1, 100)):
        rc, (tile, chunk_rows, chunks, qb, cap, nbytes) = _plan(lib, mode, n, dim, nq, k)
        assert rc == N.VRQ_OK, (n, nq, k)
        assert tile > 0 and chunk_rows % tile == 0 and chunk_rows > 0
        assert chunks >= 1 and chunks * chunk_rows >= n > (chunks - 1) * chunk_rows   # no empty chunk
        assert 1 <= qb and cap >= k + tile                                            # a tile fits after a cut
        if dim != 1024:
            assert nbytes == lib.vrq_gemm_topk_dim_workspace_size(mode, n, dim, nq, k)
        assert nbytes >= nq * chunks * k * 12                                         # the chunk lists
    # several chunks as soon as there are several tiles
    rc, info = _plan(lib, mode, 3 * 64 + 5, dim, 9, 10)
    assert rc == N.VRQ_OK and info[2] >= 3


def test_workspace_does_not_scale_with_n():
    lib = N.load()
    for mode in MODES:
        for d in DIMS:
            ws = lib.vrq_gemm_topk_dim_workspace_size(mode, 10_000_000, d, 1024, 10)
            assert 0 < ws < 2 ** 30, (mode, d, ws)
            assert ws == lib.vrq_gemm_topk_dim_workspace_size(mode, 100_000_000, d, 1024, 10)  # grid-bounded chunks


def _gemm(L, mode=N.VRQ_GEMM_BINARY, dim=384, k=10, flags=0, outs=P8, ins=P8, ws=P8, ws_bytes=1 << 40, n=1000):
    return L.vrq_gemm_topk_dim(mode, ins, ins, ins, n, dim, 0, ins, 1, k, flags, outs, outs, outs, ws, ws_bytes, None)


def _flat(L, dim=384, k=10, flags=0, outs=P8, xf=P8, ws=P8, ws_bytes=1 << 40, n=1000):
    return L.vrq_flat_ip_topk_dim(xf, None, None, None, n, dim, 0, P8, 1, k, flags, outs, outs, outs, ws, ws_bytes,
                                  None)


@pytest.mark.parametrize("call,expect", [
    (lambda L: _gemm(L, outs=None), N.VRQ_EINVAL),                                  # null outputs
    (lambda L: _flat(L, outs=None), N.VRQ_EINVAL),
    (lambda L: _gemm(L, ins=None), N.VRQ_EINVAL),                                   # null inputs
    (lambda L: _flat(L, xf=None), N.VRQ_EINVAL),
    (lambda L: _gemm(L, mode=N.VRQ_GEMM_FLOAT_IP), N.VRQ_EINVAL),                   # the flat entry point's mode
    (lambda L: _gemm(L, mode=N.VRQ_GEMM_FLOAT_IP, dim=1024), N.VRQ_EINVAL),
    (lambda L: _gemm(L, mode=N.VRQ_GEMM_FLOAT_IP, dim=1024, flags=N.VRQ_GEMM_SCAN_EXACT), N.VRQ_EINVAL),
    (lambda L: _gemm(L, dim=1032), N.VRQ_EUNSUPPORTED),
    (lambda L: _flat(L, dim=1000), N.VRQ_EUNSUPPORTED),
    (lambda L: _gemm(L, k=2000), N.VRQ_EUNSUPPORTED),
    (lambda L: _flat(L, k=2000), N.VRQ_EUNSUPPORTED),
    (lambda L: _gemm(L, flags=N.VRQ_GEMM_STAGE_SAMPLE), N.VRQ_EUNSUPPORTED),        # no stages off 1024
    (lambda L: _gemm(L, mode=N.VRQ_GEMM_INT8_COSINE, flags=N.VRQ_GEMM_STAGE_MAIN), N.VRQ_EUNSUPPORTED),
    (lambda L: _flat(L, flags=N.VRQ_GEMM_STAGE_FINISH), N.VRQ_EUNSUPPORTED),
    (lambda L: _gemm(L, dim=1024, flags=N.VRQ_GEMM_SCAN_EXACT | N.VRQ_GEMM_STAGE_MAIN), N.VRQ_EUNSUPPORTED),
    (lambda L: _gemm(L, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _gemm(L, flags=N.VRQ_GEMM_NO_FALLBACK, ws_bytes=16), N.VRQ_EWORKSPACE),  # accepted flag
    (lambda L: _gemm(L, flags=N.VRQ_GEMM_SCAN_EXACT, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _flat(L, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _gemm(L, dim=1024, flags=N.VRQ_GEMM_SCAN_EXACT, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _flat(L, dim=1024, flags=N.VRQ_GEMM_SCAN_EXACT, ws_bytes=16), N.VRQ_EWORKSPACE),
    # 1024 without the flag forwards: the ABI-1 functions' validation answers
    (lambda L: _gemm(L, dim=1024, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _gemm(L, dim=1024, k=2000), N.VRQ_EUNSUPPORTED),
    (lambda L: _flat(L, dim=1024), N.VRQ_EINVAL),                                   # x8 / inv_scale / bounds required there
])
def test_argument_validation(call, expect):
    assert call(N.load()) == expect


def test_plan_null_info():
    assert N.load().vrq_gemm_topk_dim_plan(N.VRQ_GEMM_BINARY, 1000, 384, 1, 10, None) == N.VRQ_EINVAL
