"""GPU checks of the row-sharded search with more than 1024 Phase-I candidates: the per-shard calls
vrq_shard_search3_large / vrq_shard_search2_large and the merges vrq_merge_shards_large / vrq_merge_shards2_large.
Every comparison is exact.  The references are those of tests/test_gpu_large_k.py (torch ops for Phase I, the
stand-alone rescoring calls and NumPy stable sorts for the rest) and the single-index vrq_search3_large /
vrq_search2_large over the whole corpus.  The stand-alone rescoring kernels of the reference are pinned against
exact rational arithmetic by tests/test_gpu_exact_scores.py."""
import numpy as np
import pytest
import torch

from tests.test_gpu_dims import _far_corpus
from tests.test_gpu_large_k import (INT32_MAX, N_ROWS, _deq, _N, _rescore, corpus, phase1_ref, ref_phase1,
                                    ref_search2, ref_search3, same, same_values, search2, search3, sub)

pytestmark = pytest.mark.gpu

CUTS = (0, 12_000, 12_900, N_ROWS)   # three uneven shards; the middle one holds fewer rows than any K here
NQ = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


# ----------------------------------------------------------------------------- corpus
def shard_rr(rr, cuts):
    """rescore_row with every target inside its source's shard (a rescore_row that crosses shards is out of
    scope).  The corpus remaps rows 5, 16, 27, ... to row // 2; that target is kept where it lies in the source's
    range, which it does for every such row of the first shard and for none of a later one (row // 2 is below
    the row, and below 10 000 < 12 000).  So that the last shard has duplicated ids too -- its local rescore_row
    then indexes with a non-zero row offset -- its rows of that pattern take the same halving inside their own
    range: lo + (row - lo) // 2.  Both the sharded and the single-index side use this array."""
    out = np.arange(rr.shape[0], dtype=np.int64)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        rows = np.arange(lo, hi)
        moved = rows[rr[lo:hi] != rows]
        inside = (rr[moved] >= lo) & (rr[moved] < hi)
        out[moved[inside]] = rr[moved[inside]]
        if lo == cuts[-2]:
            out[moved[~inside]] = lo + (moved[~inside] - lo) // 2
    return out


_sharded = {}


def sharded_corpus(dev, dim):
    """corpus(dev, dim) with 5 queries and the shard-restricted rescore_row."""
    if dim not in _sharded:
        c = sub(corpus(dev, dim), NQ)
        c["rr"] = shard_rr(c["rr"], CUTS)
        moved = np.flatnonzero(c["rr"] != np.arange(c["n"]))
        assert ((moved < CUTS[1]).sum() > 0) and ((moved >= CUTS[2]).sum() > 0)      # remapped rows in shards 0 and 2
        for lo, hi in zip(CUTS[:-1], CUTS[1:]):
            assert ((c["rr"][lo:hi] >= lo) & (c["rr"][lo:hi] < hi)).all()
        _sharded[dim] = c
    return _sharded[dim]


def p1(c, K):
    D, R = phase1_ref(c, K)
    return D[:c["qf"].shape[0]], R[:c["qf"].shape[0]]


# ----------------------------------------------------------------------------- calls under test
def _wsbuf(lib, size_fn, args, dev, fill=None):
    need = getattr(lib, size_fn)(*args)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    return ws


def _local_rr(c, lo, hi, dev):
    return None if c["rr"] is None else torch.from_numpy(c["rr"][lo:hi] - lo).to(dev)


def shard3(name, dev, c, lo, hi, K, flags=0):
    """One shard's (count, rows, dist, s2, s3) device tensors [nq, K] from rows [lo, hi) of the corpus."""
    N, lib = _N()
    nq, n = c["qf"].shape[0], hi - lo
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, K), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, K), -7, dtype=torch.int32, device=dev)
    s2 = torch.full((nq, K), -7.0, dtype=torch.float64, device=dev)
    s3 = torch.full((nq, K), -7.0, dtype=torch.float64, device=dev)
    ws = _wsbuf(lib, name + "_workspace_size", (n, c["dim"], nq, K), dev) if n else None
    rr = _local_rr(c, lo, hi, dev)
    codes, x8, norms = c["codes"][lo:hi], c["x8"][lo:hi], c["norms"][lo:hi]
    N.check(getattr(lib, name)(N.ptr(codes) if n else 0, N.ptr(x8) if n else 0, N.ptr(norms) if n else 0,
                               N.ptr(rr) if n else 0, n, c["dim"], lo, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, K, flags,
                               N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), N.ptr(ws),
                               0 if ws is None else ws.numel(), N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return cnt, rows, dist, s2, s3


def shard2(name, dev, c, deq, lo, hi, K, flags=0):
    N, lib = _N()
    mode, q_t, mm_t, limit = deq
    nq, n = c["qf"].shape[0], hi - lo
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, K), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, K), -7, dtype=torch.int32, device=dev)
    sc = torch.full((nq, K), -7.0, dtype=torch.float64, device=dev)
    ws = _wsbuf(lib, name + "_workspace_size", (n, c["dim"], nq, K), dev) if n else None
    rr = _local_rr(c, lo, hi, dev)
    mm = None if mm_t is None else mm_t[lo:hi]
    N.check(getattr(lib, name)(mode, N.ptr(c["codes"][lo:hi]) if n else 0, N.ptr(q_t[lo:hi]) if n else 0, N.ptr(mm),
                               float(limit), N.ptr(rr) if n else 0, n, c["dim"], lo, N.ptr(c["qf"]), N.ptr(c["qb"]),
                               nq, K, flags, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(sc), N.ptr(ws),
                               0 if ws is None else ws.numel(), N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return cnt, rows, dist, sc


def stack(parts):
    return tuple(torch.stack(t).contiguous() for t in zip(*parts))


def _merge_extra(name, lib, S, nq, K, dev, ws):
    """The (workspace, bytes) arguments of a _large merge (none for the K <= 1024 merges) and the buffer, which
    the caller holds until it has synchronised."""
    if not name.endswith("_large"):
        return (), None
    if ws is None:
        ws = _wsbuf(lib, "vrq_merge_shards_large_workspace_size", (S, nq, K), dev)
    return (int(ws.data_ptr()), ws.numel()), ws


def merge3(name, dev, st, k, K3, ws=None):
    """-> (count, rows, dist, s2, s3, src) NumPy arrays of the merge `name` over stacked [S, nq, K] tensors."""
    N, lib = _N()
    cnt, rows, dist, s2, s3 = st
    S, nq, K = rows.shape
    oc = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    orow = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    od = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    o2 = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    o3 = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    src = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    extra, ws = _merge_extra(name, lib, S, nq, K, dev, ws)
    N.check(getattr(lib, name)(S, nq, K, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), k, K3, N.ptr(oc),
                               N.ptr(orow), N.ptr(od), N.ptr(o2), N.ptr(o3), N.ptr(src), *extra,
                               N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (oc, orow, od, o2, o3, src))


def merge2(name, dev, st, k, ws=None):
    N, lib = _N()
    cnt, rows, dist, sc = st
    S, nq, K = rows.shape
    oc = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    orow = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    od = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    osc = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    src = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    extra, ws = _merge_extra(name, lib, S, nq, K, dev, ws)
    N.check(getattr(lib, name)(S, nq, K, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(sc), k, N.ptr(oc), N.ptr(orow),
                               N.ptr(od), N.ptr(osc), N.ptr(src), *extra, N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (oc, orow, od, osc, src))


def check_src(st_rows, out_rows, src):
    """out_src = s * K + p of every result in the stacked rows, -1 for the padding."""
    S, nq, K = st_rows.shape
    flat = st_rows.permute(1, 0, 2).reshape(nq, S * K).cpu().numpy()
    assert ((src >= 0) == (out_rows >= 0)).all() and (src[out_rows < 0] == -1).all()
    assert src.max() < S * K
    assert np.array_equal(np.take_along_axis(flat, np.maximum(src, 0).astype(np.int64), 1)[src >= 0],
                          out_rows[src >= 0])


def shards3(dev, c, K, cuts=CUTS, name="vrq_shard_search3_large"):
    return [shard3(name, dev, c, lo, hi, K) for lo, hi in zip(cuts[:-1], cuts[1:])]


def shards2(dev, c, deq, K, cuts=CUTS, name="vrq_shard_search2_large"):
    return [shard2(name, dev, c, deq, lo, hi, K) for lo, hi in zip(cuts[:-1], cuts[1:])]


# ----------------------------------------------------------------------------- 1: merged = single index
@pytest.mark.parametrize("K", (1025, 3000, 8192))
@pytest.mark.parametrize("dim", (384, 1024, 2048))
def test_merged_equals_single_index(dev, dim, K):
    c = sharded_corpus(dev, dim)
    D1, R1 = p1(c, K)
    parts = shards3(dev, c, K)
    counts = [int(p[0][0]) for p in parts]
    assert all((p[0] == p[0][0]).all() for p in parts)
    assert counts == [min(K, hi - lo) for lo, hi in zip(CUTS[:-1], CUTS[1:])]
    if K == 3000:
        assert counts == [3000, 900, 3000]                  # the middle shard holds fewer rows than K
    if K == 8192:
        assert counts == [8192, 900, 7100]                  # only shard 0 holds K rows
    st = stack(parts)
    for k, K3 in ((K // 10, 3 * (K // 10)), (300, K + 1000), (2000, 900)):
        got = merge3("vrq_merge_shards_large", dev, st, k, K3)
        single = search3("vrq_search3_large", dev, c, k, K, K3)
        same(got[:5], single)
        same_values(single, ref_search3(dev, c, D1, R1, k, K3))
        check_src(st[1], got[1], got[5])
        assert (got[0] == min(k, K3)).all()
    # two-phase: one score per candidate
    for mode in ("sbin", "int8g", "int4", "f32") if dim == 384 else ("sbin",):
        deq = _deq(dev, c, mode)
        st2 = stack(shards2(dev, c, deq, K))
        assert torch.equal(st2[0], st[0]) and torch.equal(st2[1], st[1]) and torch.equal(st2[2], st[2])
        for k in (K // 10, K):
            got = merge2("vrq_merge_shards2_large", dev, st2, k)
            single = search2("vrq_search2_large", dev, c, deq, k, K)
            same(got[:4], single)
            same_values(single, ref_search2(dev, c, deq, D1, R1, k))
            check_src(st2[1], got[1], got[4])
    # an all-zero query (binary and float): every score ties, the result is the first k of Phase-I order
    z = dict(c)
    z["qf"] = c["qf"].clone()
    z["qf"][2] = 0
    assert not bool(z["qb"][2].any())
    deq = _deq(dev, z, "sbin")
    k = K // 10
    got = merge2("vrq_merge_shards2_large", dev, stack(shards2(dev, z, deq, K)), k)
    same(got[:4], search2("vrq_search2_large", dev, z, deq, k, K))
    assert np.array_equal(got[1][2], R1[2, :k]) and np.array_equal(got[2][2], D1[2, :k]) and (got[3][2] == 0).all()


# ----------------------------------------------------------------------------- 2: per-shard outputs
@pytest.mark.parametrize("dim", (384, 2048))
def test_per_shard_outputs(dev, dim):
    K = 3000
    c = sharded_corpus(dev, dim)
    deq = _deq(dev, c, "int8g" if dim == 384 else "sbin")
    k_all = search3("vrq_search3_large", dev, c, K, K, K)       # the single index: every candidate with both scores
    by_row = [{int(r): (a, b) for r, a, b in zip(k_all[1][i], k_all[3][i].view(np.int64), k_all[4][i].view(np.int64))}
              for i in range(NQ)]
    rr = c["rr"]
    for si, (lo, hi) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        cnt, rows, dist, s2, s3 = (t.cpu().numpy() for t in shard3("vrq_shard_search3_large", dev, c, lo, hi, K))
        c2, rows2, dist2, sc = (t.cpu().numpy() for t in shard2("vrq_shard_search2_large", dev, c, deq, lo, hi, K))
        m = min(K, hi - lo)
        assert (cnt == m).all() and (c2 == m).all()
        assert np.array_equal(rows, rows2) and np.array_equal(dist, dist2)
        assert (rows[:, m:] == -1).all() and (dist[:, m:] == INT32_MAX).all()
        assert np.isnan(s2[:, m:]).all() and np.isnan(s3[:, m:]).all() and np.isnan(sc[:, m:]).all()
        assert (rows[:, :m] >= lo).all() and (rows[:, :m] < hi).all()
        key = (dist[:, :m].astype(np.int64) << 40) | rows[:, :m]
        assert (np.diff(key, axis=1) > 0).all()                 # strictly ascending (dist, row)
        # the shard's Phase I is the Phase I of its rows alone
        D0, R0 = ref_phase1(c["codes"][lo:hi], c["qb"], K)
        assert np.array_equal(dist, D0) and np.array_equal(rows, np.where(R0 >= 0, R0 + lo, -1))
        # scores: the stand-alone rescoring of the (remapped) global rows, bit for bit
        cand = np.where(rows >= 0, rr[np.maximum(rows, 0)], -1)
        want2 = _rescore("binary", dev, c["qf"], dim, cand, c["n"], codes_t=c["codes"])
        want3 = _rescore("cosine", dev, c["qf"], dim, cand, c["n"], x8_t=c["x8"], norms_t=c["norms"])
        wantq = _rescore("dequant", dev, c["qf"], dim, cand, c["n"], deq=deq)
        same((s2[:, :m], s3[:, :m], sc[:, :m]), (want2[:, :m], want3[:, :m], wantq[:, :m]))
        if si == 0:   # ... and the single index's scores of the same rows
            hit = 0
            for i in range(NQ):
                for j in range(m):
                    e = by_row[i].get(int(rows[i, j]))
                    if e is not None:
                        hit += 1
                        assert e == (s2[i, j:j + 1].view(np.int64)[0], s3[i, j:j + 1].view(np.int64)[0])
            assert hit > NQ * K // 4


# ----------------------------------------------------------------------------- 3: ties that cross shards
@pytest.mark.parametrize("K", (3000, 5000))
def test_ties_across_shards(dev, K):
    dim, n, cut = 384, N_ROWS, 9001
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (6, dim // 8), dtype=np.uint8)
    pick = rng.integers(0, 6, n)
    q = np.concatenate([base[:2], rng.integers(0, 256, (2, dim // 8), dtype=np.uint8), np.zeros((1, dim // 8), np.uint8)])
    qf = rng.standard_normal((q.shape[0], dim)).astype(np.float32)
    for identical, codes_np in ((False, base[pick]), (True, np.repeat(base[:1], n, axis=0))):   # 6 codes / 1 code
        c = dict(dim=dim, n=n, codes=torch.from_numpy(codes_np).to(dev), qf=torch.from_numpy(qf).to(dev),
                 qb=torch.from_numpy(q).to(dev), rr=None)
        D0, R0 = ref_phase1(c["codes"], c["qb"], K)
        if identical:
            assert np.array_equal(R0, np.tile(np.arange(K), (q.shape[0], 1)))
        else:
            # the class at T spans the cut, and the K-list ends inside it on the far side of the cut
            D_next = ref_phase1(c["codes"], c["qb"], K + 1)[0][:, -1]
            spans = [(R0[i][D0[i] == D0[i, -1]] < cut).any() and (R0[i][D0[i] == D0[i, -1]] >= cut).any() and
                     D_next[i] == D0[i, -1] for i in range(q.shape[0])]
            assert any(spans)
        deq = _deq(dev, c, "sbin")
        st = stack(shards2(dev, c, deq, K, cuts=(0, cut, n)))
        # with real scores: the merged candidates are exactly Phase I's, and equal the single index
        got = merge2("vrq_merge_shards2_large", dev, st, K)
        same(got[:4], search2("vrq_search2_large", dev, c, deq, K, K))
        key = np.sort((got[2].astype(np.int64) << 40) | got[1], axis=1)
        assert np.array_equal(key, (D0.astype(np.int64) << 40) | R0)
        # with every score equal, both merges return the Phase-I order itself
        zero = torch.zeros_like(st[3])
        got = merge2("vrq_merge_shards2_large", dev, (st[0], st[1], st[2], zero), K)
        assert np.array_equal(got[1], R0) and np.array_equal(got[2], D0) and (got[0] == K).all()
        got = merge3("vrq_merge_shards_large", dev, (st[0], st[1], st[2], zero, zero), K, K)
        assert np.array_equal(got[1], R0) and np.array_equal(got[2], D0) and (got[0] == K).all()
        check_src(st[1], got[1], got[5])


# ----------------------------------------------------------------------------- 4: global top-K in one shard
def test_top_k_in_the_last_shard(dev):
    dim, K, n, cut = 384, 1025, 40_003, 21_000
    c = dict(corpus(dev, dim, n=n, nq=5, seed=1))
    c["rr"] = None
    codes = c["codes"].clone()
    codes[n - 2000:] = c["qb"][0]
    codes[n - 2000:, 0] ^= torch.arange(2000, device=dev).to(torch.uint8) & 3
    c["codes"] = codes
    parts = shards3(dev, c, K, cuts=(0, cut, n))
    st = stack(parts)
    k, K3 = 100, 300
    got = merge3("vrq_merge_shards_large", dev, st, k, K3)
    single = search3("vrq_search3_large", dev, c, k, K, K3)
    same(got[:5], single)
    D1, R1 = ref_phase1(codes, c["qb"], K)
    same_values(single, ref_search3(dev, c, D1, R1, k, K3))
    assert (R1[0] >= n - 2000).all()                             # query 0: the late cluster is the whole K-list
    assert (got[1][0] >= cut).all() and (got[5][0] // K == 1).all() and (got[0] == k).all()
    full = merge3("vrq_merge_shards_large", dev, st, K, K)       # every candidate of query 0 from the last shard
    assert (full[5][0] // K == 1).all() and (full[0] == K).all()


# ----------------------------------------------------------------------------- 5: an empty shard
def test_empty_shard_changes_nothing(dev):
    dim, K, k, K3 = 384, 3000, 300, 900
    c = sharded_corpus(dev, dim)
    parts = shards3(dev, c, K)
    empty = shard3("vrq_shard_search3_large", dev, c, CUTS[1], CUTS[1], K)
    assert (empty[0] == 0).all() and (empty[1] == -1).all()
    assert torch.isnan(empty[3]).all() and torch.isnan(empty[4]).all()
    a = merge3("vrq_merge_shards_large", dev, stack(parts), k, K3)
    st = stack([parts[0], empty, parts[1], parts[2]])
    b = merge3("vrq_merge_shards_large", dev, st, k, K3)
    same(a[:5], b[:5])
    check_src(st[1], b[1], b[5])
    assert ((b[5] // K) != 1).all()
    deq = _deq(dev, c, "sbin")
    parts2 = shards2(dev, c, deq, K)
    empty2 = shard2("vrq_shard_search2_large", dev, c, deq, CUTS[1], CUTS[1], K)
    assert (empty2[0] == 0).all() and (empty2[1] == -1).all() and torch.isnan(empty2[3]).all()
    a = merge2("vrq_merge_shards2_large", dev, stack(parts2), k)
    b = merge2("vrq_merge_shards2_large", dev, stack([parts2[0], empty2, parts2[1], parts2[2]]), k)
    same(a[:4], b[:4])
    same(a[:4], search2("vrq_search2_large", dev, c, deq, k, K))


# ----------------------------------------------------------------------------- 6: K <= 1024
@pytest.mark.parametrize("K", (100, 1000, 1024))
@pytest.mark.parametrize("dim", (384, 1024))
def test_equals_the_existing_calls(dev, dim, K):
    c = sharded_corpus(dev, dim)
    new = shards3(dev, c, K)
    old = shards3(dev, c, K, name="vrq_shard_search3")
    for a, b in zip(new, old):
        same(tuple(t.cpu().numpy() for t in a), tuple(t.cpu().numpy() for t in b))
    st = stack(old)
    for k, K3 in ((K // 10, 3 * (K // 10)), (K, 2 * K), (K, 50)):
        same(merge3("vrq_merge_shards_large", dev, st, k, K3), merge3("vrq_merge_shards", dev, st, k, K3))
    for mode in ("sbin", "int8g", "int4", "f32"):
        deq = _deq(dev, c, mode)
        new2 = shards2(dev, c, deq, K)
        old2 = shards2(dev, c, deq, K, name="vrq_shard_search2")
        for a, b in zip(new2, old2):
            same(tuple(t.cpu().numpy() for t in a), tuple(t.cpu().numpy() for t in b))
        st2 = stack(old2)
        for k in (K // 10, K):
            same(merge2("vrq_merge_shards2_large", dev, st2, k), merge2("vrq_merge_shards2", dev, st2, k))


# ----------------------------------------------------------------------------- 7: distances above 1027
def test_distances_above_1027(dev):
    d, K, cut = 2048, 1100, 4000
    rng = np.random.default_rng(d)
    codes, q = _far_corpus(d, rng)
    n = codes.shape[0]
    qf = rng.standard_normal((q.shape[0], d)).astype(np.float32)
    c = dict(dim=d, n=n, codes=torch.from_numpy(codes).to(dev), qf=torch.from_numpy(qf).to(dev),
             qb=torch.from_numpy(q).to(dev), rr=None)
    deq = _deq(dev, c, "sbin")
    st = stack(shards2(dev, c, deq, K, cuts=(0, cut, n)))
    D0, R0 = ref_phase1(c["codes"], c["qb"], K)
    assert D0.min() >= 1028
    for k in (110, K):
        got = merge2("vrq_merge_shards2_large", dev, st, k)
        single = search2("vrq_search2_large", dev, c, deq, k, K)
        same(got[:4], single)
        same_values(single, ref_search2(dev, c, deq, D0, R0, k))
        assert got[2].min() >= 1028 and (got[0] == k).all()
        check_src(st[1], got[1], got[4])


# ----------------------------------------------------------------------------- 8: workspace hygiene
def test_merge_workspace_prefilled_with_ff(dev):
    """The merge twice on one workspace pre-filled with 0xFF, and once zero-filled: every slot is written before
    it is read."""
    lib = _N()[1]
    dim = 384
    c = sharded_corpus(dev, dim)
    for K, k, K3 in ((3000, 300, 900), (1025, 1025, 2000)):
        D1, R1 = p1(c, K)
        st = stack(shards3(dev, c, K))
        ws = _wsbuf(lib, "vrq_merge_shards_large_workspace_size", (3, NQ, K), dev, fill=0xFF)
        a = merge3("vrq_merge_shards_large", dev, st, k, K3, ws=ws)
        b = merge3("vrq_merge_shards_large", dev, st, k, K3, ws=ws)
        ws.fill_(0)
        z = merge3("vrq_merge_shards_large", dev, st, k, K3, ws=ws)
        same(a, b)
        same(a, z)
        same_values(a[:5], ref_search3(dev, c, D1, R1, k, K3))
        deq = _deq(dev, c, "sbin")
        st2 = stack(shards2(dev, c, deq, K))
        ws.fill_(0xFF)
        a = merge2("vrq_merge_shards2_large", dev, st2, k, ws=ws)
        b = merge2("vrq_merge_shards2_large", dev, st2, k, ws=ws)
        ws.fill_(0)
        z = merge2("vrq_merge_shards2_large", dev, st2, k, ws=ws)
        same(a, b)
        same(a, z)
        same_values(a[:4], ref_search2(dev, c, deq, D1, R1, k))


# ----------------------------------------------------------------------------- 9: the classes
def test_sharded_classes_k150(dev):
    """ShardedSearch / ShardedSearch2 with k * binary_oversample = 1500 over a world-1 process group equal the
    single-index searches; external ids travel through out_src."""
    import socket

    import torch.distributed as dist

    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd import quant
    from vectorragquantization_amd.dist import ShardedSearch, ShardedSearch2
    from vectorragquantization_amd.enhanced import search3 as py_search3
    c = corpus(dev, 384, dup=False, seed=3, nq=4)
    n, codes, x8, norms, qf, qb = c["n"], c["codes"], c["x8"], c["norms"], c["qf"], c["qb"]
    ids = torch.arange(n, dtype=torch.int64, device=dev) * 3 + 11
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        res = ShardedSearch(codes, x8, norms, ids, 0, n).search_vectors(qf, qb, k=150)
        two = ShardedSearch2("sbin", codes, codes, ids, 0, n).search_vectors(qf, qb, k=150)
        with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
            ShardedSearch(codes, x8, norms, ids, 0, n).search_vectors(qf, qb, k=900)
        with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
            ShardedSearch2("sbin", codes, codes, ids, 0, n).search_vectors(qf, qb, k=900)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    cnt, rows, d, s2, s3 = py_search3(codes, x8, norms, qf, qb, 150, 1500, 450)
    assert bool((cnt == 150).all())
    assert torch.equal(res.count, cnt) and torch.equal(res.row, rows) and torch.equal(res.hamming, d)
    assert torch.equal(res.binary, s2) and torch.equal(res.cosine, s3)
    assert torch.equal(res.doc_id, rows * 3 + 11)
    D1, R1 = ref_phase1(codes, qb, 1500)
    same_values(tuple(t.cpu().numpy() for t in (cnt, rows, d, s2, s3)), ref_search3(dev, c, D1, R1, 150, 450))
    rr, rd, rs = quant.search2("sbin", codes, codes, qf, qb, k=150, binary_oversample=10)
    c2, i2, r2, d2, sc2 = two
    assert bool((c2 == 150).all()) and torch.equal(r2, rr) and torch.equal(d2, rd) and torch.equal(sc2, rs)
    assert torch.equal(i2, rr * 3 + 11)
