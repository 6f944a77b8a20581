"""The filtered exhaustive entry points (vrq_row_list, vrq_gemm_topk_rows, vrq_flat_ip_topk_rows): symbols, plans,
return codes.  CPU only: every call returns before it would launch anything."""
import ctypes as C

import pytest

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1536, 2048)
P = C.c_void_p(8)  # a non-null, 8-byte aligned pointer that is never dereferenced
BIG = 1 << 40
COS, BIN, FIP = N.VRQ_GEMM_INT8_COSINE, N.VRQ_GEMM_BINARY, N.VRQ_GEMM_FLOAT_IP
SHAPES = ((1, 1, 1), (4096, 3, 10), (40000, 3, 10), (1_000_000, 600, 1024))


def gemm(L, mode=COS, dim=256, n=1000, m=500, rows=P, flags=0, ws=P, wsb=BIG, x8=P):
    return L.vrq_gemm_topk_rows(mode, None, x8, P, n, dim, 0, rows, m, P, 2, 10, flags, P, P, P, ws, wsb, None)


def flat(L, dim=256, n=1000, m=500, rows=P, flags=0, ws=P, wsb=BIG, bounds=P):
    return L.vrq_flat_ip_topk_rows(P, P, P, bounds, n, dim, 0, rows, m, P, 2, 10, flags, P, P, P, ws, wsb, None)


def plan(fn, *a):
    info = (C.c_int64 * 8)()
    return fn(*a, info), [int(v) for v in info]


def test_symbols():
    names = [n for n in N.SIGNATURES if "_rows" in n or "row_list" in n]
    assert len(names) == 8 and all(getattr(N.load(), n) is not None for n in names)


@pytest.mark.parametrize("m,nq,k", SHAPES)
@pytest.mark.parametrize("dim", DIMS)
def test_plan_is_the_unfiltered_plan_on_m_rows(dim, m, nq, k):
    L = N.load()
    ref = plan(L.vrq_gemm_topk_dim_mfma_plan, COS, m, dim, nq, k)
    assert ref[0] == N.VRQ_OK
    assert plan(L.vrq_gemm_topk_rows_plan, COS, m, dim, nq, k) == ref
    assert plan(L.vrq_flat_ip_topk_rows_plan, m, dim, nq, k) == plan(L.vrq_flat_ip_topk_dim_mfma_plan, m, dim, nq, k)
    assert L.vrq_gemm_topk_rows_workspace_size(COS, m, dim, nq, k) == ref[1][6] == \
        L.vrq_flat_ip_topk_rows_workspace_size(m, dim, nq, k)


def test_plan_at_1024_and_empty_list():
    L = N.load()
    rc, info = plan(L.vrq_gemm_topk_rows_plan, COS, 4096, 1024, 3, 10)
    assert rc == N.VRQ_OK and info[0] > 0 and info[1] > 0 and info[6] > 0 and info[7] == 128
    assert plan(L.vrq_flat_ip_topk_rows_plan, 4096, 1024, 3, 10) == (rc, info)
    for dim in DIMS + (1024,):  # m = 0 is accepted and answers as one row
        assert plan(L.vrq_gemm_topk_rows_plan, COS, 0, dim, 3, 10) == plan(L.vrq_gemm_topk_rows_plan, COS, 1, dim, 3, 10)
        assert L.vrq_flat_ip_topk_rows_workspace_size(0, dim, 3, 10) > 0
    assert plan(L.vrq_gemm_topk_rows_plan, COS, -1, 256, 3, 10)[0] == N.VRQ_EINVAL
    assert plan(L.vrq_gemm_topk_rows_plan, COS, 100, 640, 3, 10)[0] == N.VRQ_EUNSUPPORTED


ROWS = [
    (lambda L: gemm(L, mode=BIN), N.VRQ_EUNSUPPORTED),
    (lambda L: gemm(L, mode=FIP), N.VRQ_EINVAL),
    (lambda L: plan(L.vrq_gemm_topk_rows_plan, BIN, 100, 256, 3, 10)[0], N.VRQ_EUNSUPPORTED),
    (lambda L: gemm(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: gemm(L, flags=N.VRQ_GEMM_SCAN_EXACT), N.VRQ_EUNSUPPORTED),
    (lambda L: flat(L, flags=N.VRQ_GEMM_SCAN_EXACT | N.VRQ_GEMM_STAGE_MAIN), N.VRQ_EUNSUPPORTED),
    (lambda L: gemm(L, m=1001), N.VRQ_EINVAL),   # m <= n
    (lambda L: flat(L, m=-1), N.VRQ_EINVAL),
    (lambda L: gemm(L, rows=None), N.VRQ_EINVAL),
    (lambda L: flat(L, bounds=None), N.VRQ_EINVAL),
    # a workspace one byte short, at every dim; all stage flags and VRQ_GEMM_NO_FALLBACK pass the flag check
    *[(lambda L, d=d: gemm(L, dim=d, flags=240, wsb=L.vrq_gemm_topk_rows_workspace_size(COS, 500, d, 2, 10) - 1),
       N.VRQ_EWORKSPACE) for d in DIMS + (1024,)],
    *[(lambda L, d=d: flat(L, dim=d, wsb=L.vrq_flat_ip_topk_rows_workspace_size(500, d, 2, 10) - 1),
       N.VRQ_EWORKSPACE) for d in DIMS + (1024,)],
    (lambda L: L.vrq_row_list(P, 0, P, 0, P, P, BIG, None), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_row_list(P, 100, None, 0, P, P, L.vrq_row_list_workspace_size(100) - 1, None), N.VRQ_EWORKSPACE),
]


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_return_codes(i):
    call, want = ROWS[i]
    assert call(N.load()) == want
