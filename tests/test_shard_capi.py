"""Host-only contract of the sharded-search additions: ``vrq_shard_search3``, ``vrq_shard_search2`` and
``vrq_merge_shards2`` -- their exports, workspace sizes and argument validation (everything that returns
before any device work).  CPU only."""
import ctypes as C

import pytest

from vectorragquantization_amd import _native as N

P8 = C.c_void_p(8)  # a non-null pointer that validation must never dereference
DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
MF, VA = N.VRQ_SEARCH_SCAN_MFMA, N.VRQ_SEARCH_SCAN_VALU
# every flag bit of vrq.h but the two scan bits, and the first bit past them
OTHER_BITS = (N.VRQ_SEARCH_PHASE1_ONLY, N.VRQ_SEARCH_SHARD, N.VRQ_SCAN_STAGE_PREFIX, N.VRQ_SCAN_STAGE_MATRIX,
              N.VRQ_SCAN_STAGE_SUFFIX, N.VRQ_SCAN_STAGE_RECHECK, 256)


def test_exports_and_abi_version():
    N.load()
    raw = C.CDLL(N.lib_path())
    for name in ("vrq_shard_search3", "vrq_shard_search3_workspace_size", "vrq_shard_search2",
                 "vrq_shard_search2_workspace_size", "vrq_merge_shards2"):
        assert hasattr(raw, name), name
        assert name in N.SIGNATURES
    assert raw.vrq_abi_version() == 1


def test_workspace_sizes_are_the_three_phase_one():
    lib = N.load()
    for d in DIMS:
        assert lib.vrq_dim_supported(d) == 1
        for n, nq, K in ((1000, 1, 10), (200_000, 33, 100), (1_000_000, 1024, 100), (200_000, 2, 200),
                         (66_000, 40, 1000)):
            ws = lib.vrq_search3_dim_workspace_size(n, d, nq, K)
            assert ws > 0
            assert lib.vrq_shard_search3_workspace_size(n, d, nq, K) == ws
            assert lib.vrq_shard_search2_workspace_size(n, d, nq, K) == ws
    for fn in (lib.vrq_shard_search3_workspace_size, lib.vrq_shard_search2_workspace_size):
        assert fn(1000, 1032, 1, 10) == 0
        assert fn(1000, 4096, 1, 10) == 0
        assert fn(1000, 1024, 1, 1025) == 0


def _s3(L, dim=384, n=200_000, nq=4, K=10, flags=0, codes=P8, x8=P8, norms=P8, qf=P8, qb=P8, outs=P8, ws=P8,
        ws_bytes=1 << 40, **out):
    o = {name: out.get(name, outs) for name in ("count", "rows", "dist", "s2", "s3")}
    return L.vrq_shard_search3(codes, x8, norms, None, n, dim, 0, qf, qb, nq, K, flags, o["count"], o["rows"],
                               o["dist"], o["s2"], o["s3"], ws, ws_bytes, None)


def _s2(L, mode=17, dim=384, n=200_000, nq=4, K=10, flags=0, codes=P8, q=P8, mm=None, qf=P8, qb=P8, outs=P8, ws=P8,
        ws_bytes=1 << 40, **out):
    o = {name: out.get(name, outs) for name in ("count", "rows", "dist", "score")}
    return L.vrq_shard_search2(mode, codes, q, mm, 0.3, None, n, dim, 0, qf, qb, nq, K, flags, o["count"], o["rows"],
                               o["dist"], o["score"], ws, ws_bytes, None)


def _m2(L, S=2, nq=4, K=10, k=5, ins=P8, outs=P8, src=None, **kw):
    i = {name: kw.get(name, ins) for name in ("counts", "rows", "dist", "score")}
    o = {name: kw.get(name, outs) for name in ("ocount", "orows", "odist", "oscore")}
    return L.vrq_merge_shards2(S, nq, K, i["counts"], i["rows"], i["dist"], i["score"], k, o["ocount"], o["orows"],
                               o["odist"], o["oscore"], src, None)


@pytest.mark.parametrize("call,expect", [
    # ---- vrq_shard_search3
    (lambda L: _s3(L, dim=1032), N.VRQ_EUNSUPPORTED),
    (lambda L: _s3(L, dim=4096), N.VRQ_EUNSUPPORTED),
    (lambda L: _s3(L, K=1025), N.VRQ_EUNSUPPORTED),
    (lambda L: _s3(L, dim=1024, K=1025), N.VRQ_EUNSUPPORTED),
    (lambda L: _s3(L, n=-1), N.VRQ_EINVAL),
    (lambda L: _s3(L, nq=-1), N.VRQ_EINVAL),
    (lambda L: _s3(L, K=-1), N.VRQ_EINVAL),
    (lambda L: _s3(L, outs=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, count=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, rows=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, dist=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, s2=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, s3=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, codes=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, x8=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, norms=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, qf=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, qb=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, ws=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, dim=1024, x8=None), N.VRQ_EINVAL),      # checked before the forwarded scan is launched
    (lambda L: _s3(L, dim=1024, qf=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, dim=1024, s3=None), N.VRQ_EINVAL),
    (lambda L: _s3(L, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, ws=None), N.VRQ_OK),
    (lambda L: _s3(L, dim=1024, nq=0, codes=None, x8=None, norms=None, qf=None, qb=None, ws=None), N.VRQ_OK),
    (lambda L: _s3(L, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s3(L, flags=VA, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s3(L, flags=MF, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s3(L, dim=1024, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s3(L, dim=1024, flags=MF, ws_bytes=16), N.VRQ_EWORKSPACE),
    # ---- vrq_shard_search2
    (lambda L: _s2(L, mode=99), N.VRQ_EINVAL),
    (lambda L: _s2(L, mode=5), N.VRQ_EINVAL),                   # bin16 has no rescoring: not sharded
    (lambda L: _s2(L, mode=7), N.VRQ_EINVAL),                   # the encoder mode is not a rescore mode
    (lambda L: _s2(L, dim=1032), N.VRQ_EUNSUPPORTED),
    (lambda L: _s2(L, dim=4096), N.VRQ_EUNSUPPORTED),
    (lambda L: _s2(L, K=1025), N.VRQ_EUNSUPPORTED),
    (lambda L: _s2(L, dim=1024, K=1025), N.VRQ_EUNSUPPORTED),
    (lambda L: _s2(L, n=-1), N.VRQ_EINVAL),
    (lambda L: _s2(L, outs=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, count=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, rows=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, dist=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, score=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, codes=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, q=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, qf=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, qb=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, ws=None), N.VRQ_EINVAL),
    (lambda L: _s2(L, mode=3), N.VRQ_EINVAL),                   # a local mode needs minmax
    (lambda L: _s2(L, mode=4), N.VRQ_EINVAL),
    (lambda L: _s2(L, nq=0, codes=None, q=None, qf=None, qb=None, ws=None), N.VRQ_OK),
    (lambda L: _s2(L, dim=1024, nq=0, codes=None, q=None, qf=None, qb=None, ws=None), N.VRQ_OK),
    (lambda L: _s2(L, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s2(L, flags=VA, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s2(L, flags=MF, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s2(L, mode=16, dim=1024, ws_bytes=16), N.VRQ_EWORKSPACE),
    (lambda L: _s2(L, mode=0, dim=1024, flags=MF, ws_bytes=16), N.VRQ_EWORKSPACE),
    # ---- vrq_merge_shards2
    (lambda L: _m2(L, S=0), N.VRQ_EINVAL),
    (lambda L: _m2(L, nq=-1), N.VRQ_EINVAL),
    (lambda L: _m2(L, K=-1), N.VRQ_EINVAL),
    (lambda L: _m2(L, k=-1), N.VRQ_EINVAL),
    (lambda L: _m2(L, outs=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, ocount=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, orows=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, odist=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, oscore=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, ins=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, counts=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, rows=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, dist=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, score=None), N.VRQ_EINVAL),
    (lambda L: _m2(L, K=1025), N.VRQ_EUNSUPPORTED),
    (lambda L: _m2(L, S=4097), N.VRQ_EUNSUPPORTED),             # nshards > MAX_LISTS
    (lambda L: _m2(L, S=4096, nq=0), N.VRQ_OK),
    (lambda L: _m2(L, nq=0, ins=None), N.VRQ_OK),
])
def test_argument_validation(call, expect):
    assert call(N.load()) == expect


@pytest.mark.parametrize("dim", (384, 1024))
@pytest.mark.parametrize("bit", OTHER_BITS)
def test_only_the_two_scan_bits_are_flags(dim, bit):
    L = N.load()
    for flags in (bit, bit | VA, bit | MF):
        assert _s3(L, dim=dim, flags=flags) == N.VRQ_EUNSUPPORTED
        assert _s2(L, dim=dim, flags=flags) == N.VRQ_EUNSUPPORTED


def test_existing_entry_points_still_refuse_the_shard_bit():
    """The feature is additive: VRQ_SEARCH_SHARD keeps its contract on the ABI-1 and _dim entry points."""
    L = N.load()
    none = None
    assert L.vrq_search3_dim_scan(P8, 1000, 384, P8, 2, 10, N.VRQ_SEARCH_SHARD, P8, 1 << 40, none) == \
        N.VRQ_EUNSUPPORTED
    assert L.vrq_search2(17, P8, P8, none, 0.0, none, 1000, 384, 0, P8, P8, 2, 5, 10, N.VRQ_SEARCH_SHARD, P8, P8, P8,
                         P8, P8, 1 << 40, none) == N.VRQ_EUNSUPPORTED
