"""Host-only contract of the entry points for embedding dims other than 1024 (vrq_dim_supported,
vrq_search3_dim*, vrq_hamming_topk at the other code sizes): supported set, workspace sizes and the
argument validation that returns before any device work.  CPU only."""
import ctypes as C

import pytest

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1536, 2048)
P8 = C.c_void_p(8)  # a non-null pointer that validation must never dereference


def test_dim_supported():
    lib = N.load()
    for d in DIMS + (1024,):
        assert lib.vrq_dim_supported(d) == 1, d
    for d in (0, 8, 1000, 1032, 4096, -384):
        assert lib.vrq_dim_supported(d) == 0, d


def test_workspace_sizes():
    lib = N.load()
    for d in DIMS:
        ws = lib.vrq_search3_dim_workspace_size(1000, d, 1, 10)
        assert ws > 0 and ws % 80 == 0, d            # chunk lists: nq * nchunks * K * 8 bytes
        assert lib.vrq_hamming_topk_workspace_size(1000, d // 8, 1, 10) == ws
    for shape in ((1000, 1, 10), (1_000_000, 1024, 100)):
        n, nq, K = shape
        assert lib.vrq_search3_dim_workspace_size(n, 1024, nq, K) == lib.vrq_search3_workspace_size(n, 1024, nq, K) > 0
    assert lib.vrq_search3_dim_workspace_size(1000, 1032, 1, 10) == 0
    assert lib.vrq_search3_dim_workspace_size(1000, 384, 1, 2000) == 0
    assert lib.vrq_hamming_topk_workspace_size(1000, 40, 1, 10) == 0      # 320 bits: not a multiple of 128
    # the ABI-1 function keeps refusing the other dims
    assert lib.vrq_search3_workspace_size(1000, 384, 1, 10) == 0


def _search3_dim(L, dim=384, K=10, flags=0, outs=P8, ins=None, ws=None, ws_bytes=0, n=10):
    return L.vrq_search3_dim(ins, ins, ins, None, n, dim, 0, ins, ins, 1, 1, K, 1, flags, outs, outs, outs, outs, outs,
                             ws, ws_bytes, None)


@pytest.mark.parametrize("call,expect", [
    (lambda L: _search3_dim(L, outs=None), N.VRQ_EINVAL),                          # null outputs
    (lambda L: _search3_dim(L, dim=1032), N.VRQ_EUNSUPPORTED),
    (lambda L: _search3_dim(L, dim=4096), N.VRQ_EUNSUPPORTED),
    (lambda L: _search3_dim(L, K=2000), N.VRQ_EUNSUPPORTED),
    (lambda L: _search3_dim(L, flags=N.VRQ_SEARCH_SCAN_MFMA), N.VRQ_EUNSUPPORTED),
    (lambda L: _search3_dim(L, flags=N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: _search3_dim(L, flags=N.VRQ_SCAN_STAGE_MATRIX), N.VRQ_EUNSUPPORTED),
    (lambda L: _search3_dim(L), N.VRQ_EINVAL),                                     # null inputs
    (lambda L: _search3_dim(L, ins=P8, ws=P8, ws_bytes=16, n=100_000), N.VRQ_EWORKSPACE),
    (lambda L: _search3_dim(L, flags=N.VRQ_SEARCH_SCAN_VALU, ins=P8, ws=P8, ws_bytes=16), N.VRQ_EWORKSPACE),
    # 1024 forwards to vrq_search3: its validation answers
    (lambda L: _search3_dim(L, dim=1024, K=2000), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_hamming_topk(None, 10, 48, 0, None, 1, 1, None, None, None, 0, None), N.VRQ_EINVAL),
    (lambda L: L.vrq_hamming_topk(P8, 10, 40, 0, P8, 1, 1, P8, P8, P8, 1 << 20, None), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_hamming_topk(P8, 100_000, 48, 0, P8, 1, 10, P8, P8, P8, 16, None), N.VRQ_EWORKSPACE),
    (lambda L: L.vrq_rescore_binary_dim(None, 1, 1032, None, 1, None, 1, None, None), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_rescore_int8_cosine_dim(None, 1, 1000, None, None, 1, None, 1, None, None), N.VRQ_EUNSUPPORTED),
    (lambda L: L.vrq_rescore_binary_dim(None, 1, 384, None, 1, None, 1, None, None), N.VRQ_EINVAL),
    (lambda L: L.vrq_rescore_binary_dim(None, 0, 384, None, 1, None, 1, None, None), N.VRQ_OK),
])
def test_argument_validation(call, expect):
    assert call(N.load()) == expect
