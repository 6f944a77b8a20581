"""The sharded large-K entry points (vrq_shard_search3_large, vrq_shard_search2_large, vrq_merge_shards_large,
vrq_merge_shards2_large): exports, return codes, workspace sizes and the Python route.  CPU only: every call
returns before it would launch anything."""
import ctypes as C

import pytest

from vectorragquantization_amd import _native as N

DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
P = C.c_void_p(8)  # a non-null pointer that is never dereferenced
BIG = 1 << 40      # workspace bytes no plan exceeds
NAMES = ("vrq_shard_search3_large", "vrq_shard_search3_large_workspace_size", "vrq_shard_search2_large",
         "vrq_shard_search2_large_workspace_size", "vrq_merge_shards_large", "vrq_merge_shards2_large",
         "vrq_merge_shards_large_workspace_size")


def s3(L, dim=384, n=20_000, nq=4, K=2000, flags=0, codes=P, x8=P, norms=P, qf=P, qb=P, outs=P, ws=P, wsb=BIG, **out):
    o = {name: out.get(name, outs) for name in ("count", "rows", "dist", "b", "c")}
    return L.vrq_shard_search3_large(codes, x8, norms, None, n, dim, 0, qf, qb, nq, K, flags, o["count"], o["rows"],
                                     o["dist"], o["b"], o["c"], ws, wsb, None)


def s2(L, mode=17, dim=384, n=20_000, nq=4, K=2000, flags=0, codes=P, q=P, mm=None, qf=P, qb=P, outs=P, ws=P,
       wsb=BIG, **out):
    o = {name: out.get(name, outs) for name in ("count", "rows", "dist", "score")}
    return L.vrq_shard_search2_large(mode, codes, q, mm, 0.3, None, n, dim, 0, qf, qb, nq, K, flags, o["count"],
                                     o["rows"], o["dist"], o["score"], ws, wsb, None)


def m3(L, S=3, nq=4, K=2000, k=200, K3=600, ins=P, outs=P, src=None, ws=P, wsb=BIG, **kw):
    i = {name: kw.get(name, ins) for name in ("counts", "rows", "dist", "s2", "s3")}
    o = {name: kw.get(name, outs) for name in ("ocount", "orows", "odist", "ob", "oc")}
    return L.vrq_merge_shards_large(S, nq, K, i["counts"], i["rows"], i["dist"], i["s2"], i["s3"], k, K3,
                                    o["ocount"], o["orows"], o["odist"], o["ob"], o["oc"], src, ws, wsb, None)


def m2(L, S=3, nq=4, K=2000, k=200, ins=P, outs=P, src=None, ws=P, wsb=BIG, **kw):
    i = {name: kw.get(name, ins) for name in ("counts", "rows", "dist", "score")}
    o = {name: kw.get(name, outs) for name in ("ocount", "orows", "odist", "oscore")}
    return L.vrq_merge_shards2_large(S, nq, K, i["counts"], i["rows"], i["dist"], i["score"], k, o["ocount"],
                                     o["orows"], o["odist"], o["oscore"], src, ws, wsb, None)


def test_exports_and_abi_version():
    N.load()
    raw = C.CDLL(N.lib_path())
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in N.SIGNATURES
    assert raw.vrq_abi_version() == 1


@pytest.mark.parametrize("call,expect", [
    # ---- vrq_shard_search3_large
    (lambda L: s3(L, codes=None), N.VRQ_EINVAL),
    (lambda L: s3(L, x8=None), N.VRQ_EINVAL),
    (lambda L: s3(L, norms=None), N.VRQ_EINVAL),
    (lambda L: s3(L, qf=None), N.VRQ_EINVAL),
    (lambda L: s3(L, qb=None), N.VRQ_EINVAL),
    (lambda L: s3(L, ws=None), N.VRQ_EINVAL),
    (lambda L: s3(L, outs=None), N.VRQ_EINVAL),
    (lambda L: s3(L, count=None), N.VRQ_EINVAL),
    (lambda L: s3(L, rows=None), N.VRQ_EINVAL),
    (lambda L: s3(L, dist=None), N.VRQ_EINVAL),
    (lambda L: s3(L, b=None), N.VRQ_EINVAL),
    (lambda L: s3(L, c=None), N.VRQ_EINVAL),
    (lambda L: s3(L, n=-1), N.VRQ_EINVAL),
    (lambda L: s3(L, nq=-1), N.VRQ_EINVAL),
    (lambda L: s3(L, K=-1), N.VRQ_EINVAL),
    (lambda L: s3(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: s3(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: s3(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    (lambda L: s3(L, wsb=16), N.VRQ_EWORKSPACE),
    (lambda L: s3(L, dim=1024, K=8192, wsb=16), N.VRQ_EWORKSPACE),
    (lambda L: s3(L, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, ws=None, wsb=0), N.VRQ_OK),
    # ---- vrq_shard_search2_large
    (lambda L: s2(L, mode=99), N.VRQ_EINVAL),
    (lambda L: s2(L, mode=5), N.VRQ_EINVAL),                   # bin16 has no rescoring: not sharded
    (lambda L: s2(L, mode=3), N.VRQ_EINVAL),                   # a local mode needs minmax
    (lambda L: s2(L, codes=None), N.VRQ_EINVAL),
    (lambda L: s2(L, q=None), N.VRQ_EINVAL),
    (lambda L: s2(L, qf=None), N.VRQ_EINVAL),
    (lambda L: s2(L, qb=None), N.VRQ_EINVAL),
    (lambda L: s2(L, ws=None), N.VRQ_EINVAL),
    (lambda L: s2(L, outs=None), N.VRQ_EINVAL),
    (lambda L: s2(L, count=None), N.VRQ_EINVAL),
    (lambda L: s2(L, rows=None), N.VRQ_EINVAL),
    (lambda L: s2(L, dist=None), N.VRQ_EINVAL),
    (lambda L: s2(L, score=None), N.VRQ_EINVAL),
    (lambda L: s2(L, n=-1), N.VRQ_EINVAL),
    (lambda L: s2(L, dim=640), N.VRQ_EUNSUPPORTED),
    (lambda L: s2(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: s2(L, n=1 << 32), N.VRQ_EUNSUPPORTED),
    (lambda L: s2(L, wsb=16), N.VRQ_EWORKSPACE),
    (lambda L: s2(L, mode=0, dim=1024, wsb=16), N.VRQ_EWORKSPACE),
    (lambda L: s2(L, nq=0, codes=None, q=None, qf=None, qb=None, ws=None, wsb=0), N.VRQ_OK),
    # ---- vrq_merge_shards_large
    (lambda L: m3(L, S=0), N.VRQ_EINVAL),
    (lambda L: m3(L, nq=-1), N.VRQ_EINVAL),
    (lambda L: m3(L, K=-1), N.VRQ_EINVAL),
    (lambda L: m3(L, k=-1), N.VRQ_EINVAL),
    (lambda L: m3(L, K3=-1), N.VRQ_EINVAL),
    (lambda L: m3(L, outs=None), N.VRQ_EINVAL),
    (lambda L: m3(L, ocount=None), N.VRQ_EINVAL),
    (lambda L: m3(L, orows=None), N.VRQ_EINVAL),
    (lambda L: m3(L, odist=None), N.VRQ_EINVAL),
    (lambda L: m3(L, ob=None), N.VRQ_EINVAL),
    (lambda L: m3(L, oc=None), N.VRQ_EINVAL),
    (lambda L: m3(L, ins=None), N.VRQ_EINVAL),
    (lambda L: m3(L, counts=None), N.VRQ_EINVAL),
    (lambda L: m3(L, rows=None), N.VRQ_EINVAL),
    (lambda L: m3(L, dist=None), N.VRQ_EINVAL),
    (lambda L: m3(L, s2=None), N.VRQ_EINVAL),
    (lambda L: m3(L, s3=None), N.VRQ_EINVAL),
    (lambda L: m3(L, ws=None), N.VRQ_EINVAL),
    (lambda L: m3(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: m3(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: m3(L, S=4097), N.VRQ_EUNSUPPORTED),
    (lambda L: m3(L, wsb=16), N.VRQ_EWORKSPACE),
    (lambda L: m3(L, S=4096, K=8192, k=8192, K3=1 << 30, wsb=16), N.VRQ_EWORKSPACE),   # every limit at once
    (lambda L: m3(L, S=4096, nq=0), N.VRQ_OK),
    (lambda L: m3(L, nq=0, ins=None, ws=None, wsb=0), N.VRQ_OK),
    # ---- vrq_merge_shards2_large
    (lambda L: m2(L, S=0), N.VRQ_EINVAL),
    (lambda L: m2(L, nq=-1), N.VRQ_EINVAL),
    (lambda L: m2(L, K=-1), N.VRQ_EINVAL),
    (lambda L: m2(L, k=-1), N.VRQ_EINVAL),
    (lambda L: m2(L, outs=None), N.VRQ_EINVAL),
    (lambda L: m2(L, ocount=None), N.VRQ_EINVAL),
    (lambda L: m2(L, orows=None), N.VRQ_EINVAL),
    (lambda L: m2(L, odist=None), N.VRQ_EINVAL),
    (lambda L: m2(L, oscore=None), N.VRQ_EINVAL),
    (lambda L: m2(L, ins=None), N.VRQ_EINVAL),
    (lambda L: m2(L, counts=None), N.VRQ_EINVAL),
    (lambda L: m2(L, rows=None), N.VRQ_EINVAL),
    (lambda L: m2(L, dist=None), N.VRQ_EINVAL),
    (lambda L: m2(L, score=None), N.VRQ_EINVAL),
    (lambda L: m2(L, ws=None), N.VRQ_EINVAL),
    (lambda L: m2(L, K=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: m2(L, k=8193), N.VRQ_EUNSUPPORTED),
    (lambda L: m2(L, S=4097), N.VRQ_EUNSUPPORTED),
    (lambda L: m2(L, wsb=16), N.VRQ_EWORKSPACE),
    (lambda L: m2(L, S=4096, nq=0), N.VRQ_OK),
    (lambda L: m2(L, nq=0, ins=None, ws=None, wsb=0), N.VRQ_OK),
])
def test_return_codes(call, expect):
    assert call(N.load()) == expect


@pytest.mark.parametrize("dim", (384, 1024))
@pytest.mark.parametrize("bit", (N.VRQ_SEARCH_PHASE1_ONLY, N.VRQ_SEARCH_SHARD, N.VRQ_SEARCH_SCAN_VALU,
                                 N.VRQ_SEARCH_SCAN_MFMA, N.VRQ_SCAN_STAGE_PREFIX, N.VRQ_SCAN_STAGE_MATRIX,
                                 N.VRQ_SCAN_STAGE_SUFFIX, N.VRQ_SCAN_STAGE_RECHECK, 256))
def test_no_flag_is_accepted(dim, bit):
    """The counting scan takes no scan flags: any bit is VRQ_EUNSUPPORTED, at a small K too."""
    L = N.load()
    for K in (100, 2000):
        assert s3(L, dim=dim, K=K, flags=bit) == N.VRQ_EUNSUPPORTED
        assert s2(L, dim=dim, K=K, flags=bit) == N.VRQ_EUNSUPPORTED


@pytest.mark.parametrize("dim", DIMS)
def test_shard_workspace_is_the_single_index_one_and_one_byte_short(dim):
    lib = N.load()
    for n, nq, K in ((20000, 3, 3000), (5, 1, 8192), (1_000_000, 64, 1024), (900, 5, 1025)):
        need = lib.vrq_search3_large_workspace_size(n, dim, nq, K)
        assert need > 0
        assert lib.vrq_shard_search3_large_workspace_size(n, dim, nq, K) == need
        assert lib.vrq_shard_search2_large_workspace_size(n, dim, nq, K) == need
        assert lib.vrq_shard_search3_large_workspace_size(n, dim, nq, K) == need   # a pure function
        assert s3(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1) == N.VRQ_EWORKSPACE
        assert s2(lib, n=n, dim=dim, nq=nq, K=K, wsb=need - 1) == N.VRQ_EWORKSPACE


def test_merge_workspace_size():
    lib = N.load()
    size = lib.vrq_merge_shards_large_workspace_size
    for S, nq, K in ((1, 1, 1), (3, 5, 1025), (8, 8, 8192), (2, 64, 1500), (4096, 2, 100), (3, 4, 1024)):
        need = size(S, nq, K)
        # keys u64 + src i32 + s2, s3, s3 by position f64 + the Phase-II order i32, per candidate; a count per query
        assert need >= nq * K * (8 + 4 + 8 + 8 + 8 + 4) + nq * 4 and need % 256 == 0
        assert need == size(S, nq, K)                                              # a pure function
        assert need == size(1, nq, K)                                              # ... of (nq, K) for a valid S
        assert m3(lib, S=S, nq=nq, K=K, k=min(K, 10), wsb=need - 1) == N.VRQ_EWORKSPACE
        assert m2(lib, S=S, nq=nq, K=K, k=min(K, 10), wsb=need - 1) == N.VRQ_EWORKSPACE
    for S, nq, K in ((0, 1, 100), (4097, 1, 100), (2, 0, 100), (2, 1, 0), (2, 1, 8193), (-1, 1, 100), (2, -1, 100)):
        assert size(S, nq, K) == 0


def test_shard_workspace_size_is_zero_for_unsupported_shapes():
    lib = N.load()
    for fn in (lib.vrq_shard_search3_large_workspace_size, lib.vrq_shard_search2_large_workspace_size):
        assert fn(1000, 640, 1, 2000) == 0
        assert fn(1000, 1024, 1, 8193) == 0
        assert fn(1000, 1024, 0, 2000) == 0
        assert fn(1 << 32, 1024, 1, 2000) == 0


def test_empty_shapes_are_ok_without_inputs():
    """n or K = 0 with nq = 0 never touch a pointer; nq = 0 writes nothing at all."""
    L = N.load()
    assert s3(L, n=0, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, ws=None, wsb=0) == N.VRQ_OK
    assert s2(L, K=0, nq=0, codes=None, q=None, qf=None, qb=None, ws=None, wsb=0) == N.VRQ_OK
    assert m3(L, K=0, nq=0, ins=None, ws=None, wsb=0) == N.VRQ_OK
    assert m2(L, k=0, nq=0, ins=None, ws=None, wsb=0) == N.VRQ_OK


def test_python_route():
    from vectorragquantization_amd.dist import shard_calls
    small = {"search3": "vrq_shard_search3", "search2": "vrq_shard_search2", "merge3": "vrq_merge_shards",
             "merge2": "vrq_merge_shards2"}
    assert shard_calls(1) == small and shard_calls(1024) == small
    assert shard_calls(1024, N.VRQ_SEARCH_SCAN_MFMA) == small           # the scan flags stay with K <= 1024
    large = {k: v + "_large" for k, v in small.items()}
    assert shard_calls(1025) == large and shard_calls(8192) == large
    lib = N.load()
    for name in list(small.values()) + list(large.values()):
        assert hasattr(lib, name)
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        shard_calls(9000)
    with pytest.raises(N.VrqNativeError, match=r"flags 8.*1025.*1024"):
        shard_calls(1025, N.VRQ_SEARCH_SCAN_MFMA)


def test_existing_calls_still_refuse_1025():
    """The feature is additive: the K <= 1024 contract of the existing sharded calls is not widened."""
    L = N.load()
    assert L.vrq_shard_search3(P, P, P, None, 20_000, 384, 0, P, P, 4, 1025, 0, P, P, P, P, P, P, BIG, None) == \
        N.VRQ_EUNSUPPORTED
    assert L.vrq_shard_search2(17, P, P, None, 0.0, None, 20_000, 384, 0, P, P, 4, 1025, 0, P, P, P, P, P, BIG,
                               None) == N.VRQ_EUNSUPPORTED
    assert L.vrq_merge_shards(2, 4, 1025, P, P, P, P, P, 5, 15, P, P, P, P, P, None, None) == N.VRQ_EUNSUPPORTED
    assert L.vrq_merge_shards2(2, 4, 1025, P, P, P, P, 5, P, P, P, P, None, None) == N.VRQ_EUNSUPPORTED
    assert L.vrq_shard_search3_workspace_size(20_000, 384, 4, 1025) == 0
