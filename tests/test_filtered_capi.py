"""The filtered entry points (vrq_*_filtered: a row allow-bitmap through the counting scan K1h): return codes,
workspace sizes, the header / loader / library agreement, the bitmap helpers and the wrappers' routing.
CPU only: every call returns before it would launch anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
P = C.c_void_p(8)    # a non-null, 8-byte aligned pointer that is never dereferenced
ODD = C.c_void_p(12)  # non-null but not 8-byte aligned
BIG = 1 << 40        # workspace bytes no plan exceeds
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrq.h")
NAMES = ("vrq_hamming_topk_filtered", "vrq_search3_filtered", "vrq_search2_filtered", "vrq_scan_filtered")


def hamming(L, codes=P, n=1000, cb=128, q=P, nq=2, k=2000, allow=P, od=P, orows=P, ws=P, wsb=BIG):
    return L.vrq_hamming_topk_filtered(codes, n, cb, 0, q, nq, k, allow, od, orows, ws, wsb, None)


def search3(L, codes=P, x8=P, norms=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, K3=30, flags=0, allow=P,
            oc=P, orows=P, od=P, ob=P, ocos=P, ws=P, wsb=BIG):
    return L.vrq_search3_filtered(codes, x8, norms, None, n, dim, 0, qf, qb, nq, k, K, K3, flags, allow, oc, orows,
                                  od, ob, ocos, ws, wsb, None)


def search2(L, mode=0, codes=P, q=P, n=1000, dim=1024, qf=P, qb=P, nq=2, k=10, K=2000, flags=0, allow=P, oc=P,
            orows=P, od=P, osc=P, ws=P, wsb=BIG, minmax=None):
    return L.vrq_search2_filtered(mode, codes, q, minmax, 0.3, None, n, dim, 0, qf, qb, nq, k, K, flags, allow, oc,
                                  orows, od, osc, ws, wsb, None)


def scan(L, codes=P, n=1000, dim=1024, qb=P, nq=1, K=2000, stages=0, allow=P, ws=P, wsb=BIG):
    return L.vrq_scan_filtered(codes, n, dim, qb, nq, K, stages, allow, ws, wsb, None)


@pytest.mark.parametrize("call,expect", [
    # the bitmap: null, misaligned
    (lambda L: hamming(L, allow=None), N.VRQ_EINVAL),
    (lambda L: hamming(L, allow=ODD), N.VRQ_EINVAL),
    (lambda L: search3(L, allow=None), N.VRQ_EINVAL),
    (lambda L: search3(L, allow=ODD), N.VRQ_EINVAL),
    (lambda L: search3(L, allow=None, flags=N.VRQ_SEARCH_PHASE1_ONLY), N.VRQ_EINVAL),
    (lambda L: search2(L, allow=None), N.VRQ_EINVAL),
    (lambda L: search2(L, allow=ODD), N.VRQ_EINVAL),
    (lambda L: scan(L, allow=None), N.VRQ_EINVAL),
    (lambda L: scan(L, allow=ODD), N.VRQ_EINVAL),
    (lambda L: scan(L, allow=ODD, stages=N.VRQ_LARGE_STAGE_THRESHOLD), N.VRQ_EINVAL),
    # every null pointer of the *_large tables
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
    (lambda L: scan(L, codes=None), N.VRQ_EINVAL),
    (lambda L: scan(L, qb=None), N.VRQ_EINVAL),
    (lambda L: scan(L, ws=None), N.VRQ_EINVAL),
    # K = 0 is an empty call (as the *_large ones: nothing scanned, no bitmap read), K past the limit,
    # unsupported dims, n past 2^32 - 1
    (lambda L: hamming(L, k=0, codes=None, q=None, allow=None, ws=None, wsb=0), N.VRQ_OK),
    (lambda L: scan(L, K=0, codes=None, qb=None, allow=None, ws=None, wsb=0), N.VRQ_OK),
    (lambda L: hamming(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: scan(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: hamming(L, cb=100), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: scan(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: hamming(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    (lambda L: scan(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    # K <= 1024 is this path's too: only the workspace stops these
    (lambda L: hamming(L, k=10, wsb=16), N.VRQ_EWORKSPACE),
    (lambda L: search3(L, K=10, k=1, wsb=16), N.VRQ_EWORKSPACE),
    # flags outside the allowed set
    (lambda L: search3(L, flags=N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, flags=N.VRQ_SEARCH_SCAN_MFMA), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, flags=N.VRQ_SEARCH_SCAN_VALU), N.VRQ_EUNSUPPORTED),
    (lambda L: search3(L, flags=N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SCAN_STAGE_SUFFIX), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, flags=N.VRQ_SEARCH_PHASE1_ONLY), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, flags=N.VRQ_SEARCH_SHARD), N.VRQ_EUNSUPPORTED),
    (lambda L: search2(L, flags=N.VRQ_SEARCH_SCAN_MFMA), N.VRQ_EUNSUPPORTED),
    (lambda L: scan(L, stages=8), N.VRQ_EUNSUPPORTED),
    # short workspace
    (lambda L: scan(L, stages=N.VRQ_LARGE_STAGE_EMIT, wsb=16), N.VRQ_EWORKSPACE),
    # zero-size shapes: nothing to do (nq = 0 writes nothing at all), and no bitmap is asked for
    (lambda L: hamming(L, nq=0, codes=None, q=None, allow=None, ws=None, wsb=0), N.VRQ_OK),
    (lambda L: search3(L, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, allow=None, ws=None, wsb=0),
     N.VRQ_OK),
    (lambda L: search3(L, nq=0, flags=N.VRQ_SEARCH_PHASE1_ONLY, ob=None, ocos=None, allow=None, ws=None, wsb=0),
     N.VRQ_OK),
    (lambda L: search2(L, nq=0, codes=None, q=None, qf=None, qb=None, allow=None, ws=None, wsb=0), N.VRQ_OK),
    (lambda L: scan(L, n=0, codes=None, qb=None, allow=None, ws=None, wsb=0), N.VRQ_OK),
])
def test_return_codes(call, expect):
    assert call(N.load()) == expect


@pytest.mark.parametrize("dim", DIMS)
def test_workspace_is_the_large_one_and_one_byte_short_fails(dim):
    lib = N.load()
    for n, nq, K in ((20000, 3, 3000), (5, 1, 8192), (1_000_000, 64, 1024), (12325, 17, 10)):
        need = lib.vrq_search3_large_workspace_size(n, dim, nq, K)
        assert need > 0
        assert lib.vrq_search3_filtered_workspace_size(n, dim, nq, K) == need
        assert lib.vrq_search2_filtered_workspace_size(n, dim, nq, K) == need
        assert lib.vrq_scan_filtered_workspace_size(n, dim, nq, K) == need
        assert lib.vrq_hamming_topk_filtered_workspace_size(n, dim // 8, nq, K) == need
        assert search3(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1) == N.VRQ_EWORKSPACE
        assert search3(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1, flags=N.VRQ_SEARCH_PHASE1_ONLY) == N.VRQ_EWORKSPACE
        assert search2(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1) == N.VRQ_EWORKSPACE
        assert hamming(lib, n=n, cb=dim // 8, nq=nq, k=K, wsb=need - 1) == N.VRQ_EWORKSPACE
        assert scan(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1) == N.VRQ_EWORKSPACE


def test_workspace_size_is_zero_for_unsupported_shapes():
    lib = N.load()
    assert lib.vrq_search3_filtered_workspace_size(1000, 640, 1, 2000) == 0
    assert lib.vrq_search3_filtered_workspace_size(1000, 1024, 1, 8193) == 0
    assert lib.vrq_search2_filtered_workspace_size(1000, 1024, 0, 2000) == 0
    assert lib.vrq_scan_filtered_workspace_size(0, 1024, 1, 2000) == 0
    assert lib.vrq_hamming_topk_filtered_workspace_size(1000, 100, 1, 2000) == 0
    assert lib.vrq_hamming_topk_filtered_workspace_size(1 << 32, 128, 1, 2000) == 0


def test_header_loader_and_library_agree():
    src = open(HDR).read()
    raw = C.CDLL(N.lib_path())
    for name in NAMES:
        for sym in (name, name + "_workspace_size"):
            assert re.search(r"\b" + sym + r"\s*\(", src), sym
            assert sym in N.SIGNATURES, sym
            assert hasattr(raw, sym), sym
        # one argument more than the *_large call: the bitmap, a pointer
        large = N.SIGNATURES[name.replace("_filtered", "_large")]
        res, args = N.SIGNATURES[name]
        assert res is large[0] and len(args) == len(large[1]) + 1
        rest = list(args)
        i = {"vrq_hamming_topk_filtered": 7, "vrq_search3_filtered": 14, "vrq_search2_filtered": 15,
             "vrq_scan_filtered": 7}[name]
        assert rest.pop(i) is C.c_void_p and rest == list(large[1])
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", src)
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert params[i] == "const uint64_t* allow" and len(params) == len(args)
        assert N.SIGNATURES[name + "_workspace_size"] == N.SIGNATURES["vrq_search3_large_workspace_size"]


# ---- filters.py on CPU tensors ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 12325])
def test_row_bitmap_matches_packbits(n):
    from vectorragquantization_amd.filters import row_bitmap
    rng = np.random.default_rng(n)
    for mask in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1):
        by = np.packbits(mask, bitorder="little")
        ref = np.zeros(((n + 63) // 64) * 8, np.uint8)
        ref[:by.shape[0]] = by
        got = row_bitmap(torch.from_numpy(mask))
        assert got.dtype == torch.int64 and got.shape == ((n + 63) // 64,) and got.is_contiguous()
        assert np.array_equal(got.numpy().view("<u8"), ref.view("<u8"))


def test_row_bitmap_of_no_rows():
    from vectorragquantization_amd.filters import row_bitmap
    assert row_bitmap(torch.zeros(0, dtype=torch.bool)).shape == (0,)


def test_ids_bitmap_duplicates_and_unknown_ids():
    from vectorragquantization_amd.filters import ids_bitmap, row_bitmap
    id_map = torch.tensor([7, 3, 7, 9, 11, 3] + list(range(100, 170)), dtype=torch.int64)
    got = ids_bitmap(id_map, [7, 3, 555, -1, 169])           # 555 and -1: not in the index
    mask = torch.zeros(76, dtype=torch.bool)
    mask[[0, 1, 2, 5, 75]] = True                               # both rows of 7 and of 3
    assert torch.equal(got, row_bitmap(mask))
    assert torch.equal(ids_bitmap(id_map, torch.tensor([9])), row_bitmap(id_map == 9))
    assert torch.equal(ids_bitmap(id_map, {555}), torch.zeros(2, dtype=torch.int64))
    assert torch.equal(ids_bitmap(id_map, []), torch.zeros(2, dtype=torch.int64))
    assert torch.equal(ids_bitmap(id_map, (i for i in (11,))), row_bitmap(id_map == 11))


def test_bitmap_shape_is_checked():
    from vectorragquantization_amd.filters import checked
    ok = torch.zeros(3, dtype=torch.int64)
    assert checked(ok, 129, "cpu") is ok or torch.equal(checked(ok, 129, "cpu"), ok)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros((3, 1), dtype=torch.int64),
                np.zeros(3, np.int64)):
        with pytest.raises(N.VrqNativeError, match="3 words"):
            checked(bad, 129, "cpu")


# ---- the wrappers' routing ----
def test_wrappers_route_every_k_to_the_filtered_call():
    from vectorragquantization_amd.enhanced import search3_call
    allow = torch.zeros(1, dtype=torch.int64)
    assert search3_call(10, 0, allow) == "vrq_search3_filtered"
    assert search3_call(5000, 0, allow) == "vrq_search3_filtered"
    assert search3_call(10, N.VRQ_SEARCH_PHASE1_ONLY, allow) == "vrq_search3_filtered"
    assert search3_call(10) == "vrq_search3_dim" and search3_call(5000) == "vrq_search3_large"   # allow=None: as before
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        search3_call(9000, 0, allow)
    with pytest.raises(N.VrqNativeError, match="row filter"):
        search3_call(10, N.VRQ_SEARCH_SHARD, allow)
    with pytest.raises(N.VrqNativeError, match="row filter"):
        search3_call(5000, N.VRQ_SEARCH_SCAN_MFMA, allow)
    assert hasattr(N.load(), "vrq_search3_filtered_workspace_size")


def test_search2_and_vectordb_search_raise_before_any_launch():
    """K past the limit and the scan flags raise in the wrappers with a filter, on CPU tensors: nothing is
    launched (the *_filtered names are what the calls would have taken)."""
    from vectorragquantization_amd import quant as Q
    n, d = 9000, 256
    codes = torch.zeros((n, d // 8), dtype=torch.uint8)
    qf, qb = torch.zeros((1, d)), torch.zeros((1, d // 8), dtype=torch.uint8)
    allow = torch.zeros((n + 63) // 64, dtype=torch.int64)
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        Q.search2("sbin", codes, codes, qf, qb, 900, 10, allow=allow)
    with pytest.raises(N.VrqNativeError, match="row filter"):
        Q.search2("sbin", codes, codes, qf, qb, 10, 10, flags=N.VRQ_SEARCH_SCAN_VALU, allow=allow)
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        Q.vectordb_search("bin16", codes, None, None, qb, 900, 10, allow=allow)
    with pytest.raises(N.VrqNativeError, match="words"):
        Q.search2("sbin", codes, codes, qf, qb, 10, 10, allow=allow[:-1])
