"""vrq_binary_topk_gather*: symbols, plans, return codes.  CPU only: every call returns before it would launch."""
import ctypes as C

import pytest

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1536, 2048)
P = C.c_void_p(8)  # a non-null, 8-byte aligned pointer that is never dereferenced


def call(L, dim=256, n=1000, m=500, rows=P, flags=0, wsb=1 << 40):
    return L.vrq_binary_topk_gather(P, n, dim, 0, rows, m, P, 2, 10, flags, P, P, P, P, wsb, None)


def plan(fn, *a):
    info = (C.c_int64 * 8)()
    return fn(*a, info), [int(v) for v in info]


@pytest.mark.parametrize("m,nq,k", ((1, 1, 1), (4096, 3, 10), (40000, 3, 10), (1_000_000, 600, 1024)))
@pytest.mark.parametrize("dim", DIMS)
def test_plan_is_the_unfiltered_plan_on_m_rows(dim, m, nq, k):
    L = N.load()
    ref = plan(L.vrq_binary_topk_dim_mfma_plan, m, dim, nq, k)
    assert ref[0] == N.VRQ_OK and plan(L.vrq_binary_topk_gather_plan, m, dim, nq, k) == ref
    assert L.vrq_binary_topk_gather_workspace_size(m, dim, nq, k) == ref[1][6]


def test_symbols_plan_at_1024_and_empty_list():
    L = N.load()
    assert len([getattr(L, n) for n in N.SIGNATURES if n.startswith("vrq_binary_topk_gather")]) == 3
    rc, info = plan(L.vrq_binary_topk_gather_plan, 4096, 1024, 3, 10)
    assert rc == N.VRQ_OK and info[7] == 128 and info[6] == L.vrq_binary_topk_gather_workspace_size(4096, 1024, 3, 10) > 0
    for dim in DIMS + (1024,):  # m = 0 is accepted and answers as one row
        assert plan(L.vrq_binary_topk_gather_plan, 0, dim, 3, 10) == plan(L.vrq_binary_topk_gather_plan, 1, dim, 3, 10)


CODES = [
    (lambda L: call(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: call(L, flags=N.VRQ_GEMM_SCAN_EXACT | N.VRQ_GEMM_STAGE_MAIN), N.VRQ_EUNSUPPORTED),
    (lambda L: call(L, m=1001), N.VRQ_EINVAL),   # m <= n
    (lambda L: call(L, m=-1), N.VRQ_EINVAL),
    (lambda L: call(L, rows=None), N.VRQ_EINVAL),
    # a workspace one byte short, at every dim; all stage flags and VRQ_GEMM_NO_FALLBACK pass the flag check
    *[(lambda L, d=d: call(L, dim=d, flags=240, wsb=L.vrq_binary_topk_gather_workspace_size(500, d, 2, 10) - 1),
       N.VRQ_EWORKSPACE) for d in DIMS + (1024,)],
]


@pytest.mark.parametrize("i", range(len(CODES)))
def test_return_codes(i):
    assert CODES[i][0](N.load()) == CODES[i][1]
