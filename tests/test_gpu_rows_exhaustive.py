"""K5g on the GPU (vrq_row_list, vrq_gemm_topk_rows, vrq_flat_ip_topk_rows and the wrappers above them) against
a float64 NumPy reference over the allowed rows and against the unfiltered matrix call on the gathered copy."""
import ctypes as C

import numpy as np
import pytest
import torch

from vectorragquantization_amd import _native as N
from vectorragquantization_amd import filters
from vectorragquantization_amd.enhanced import gemm_topk
from vectorragquantization_amd.flat import CohereVectorDBFloat, FloatIndexIDMap, flat_ip_prepare, flat_ip_topk

pytestmark = pytest.mark.gpu
DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
MODES = ("int8_cosine", "float_ip")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    N.load()
    return torch.device("cuda", 0)


def _corpus(rng, mode, n, dim):
    if mode == "int8_cosine":
        return rng.integers(-127, 128, (n, dim), dtype=np.int8)
    F = rng.standard_normal((n, dim))
    return (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)


def _like_queries(mode, qf):  # rows that score at the top for their query: scaled copies of the queries
    if mode == "int8_cosine":
        return np.rint(qf * (127.0 / np.abs(qf).max(axis=1, keepdims=True))).astype(np.int8)
    return (qf * 3.0).astype(np.float32)


def _ops(mode, X, dev):
    Xd = torch.from_numpy(X).to(dev)
    if mode == "int8_cosine":
        return Xd, torch.from_numpy(np.sqrt((X.astype(np.float64) ** 2).sum(axis=1))).to(dev)
    bounds = torch.zeros((2,), dtype=torch.float64, device=dev)
    return (Xd, *flat_ip_prepare(Xd, bounds), bounds)


def _search(mode, ops, qf, k, rows=None, flags=0):
    q = torch.from_numpy(qf).to(ops[0].device)
    if mode == "int8_cosine":
        out = gemm_topk("int8_cosine", q, k, x8=ops[0], norms=ops[1], flags=flags, rows=rows,
                        engine=None if rows is not None else "mfma")
    else:
        out = flat_ip_topk(*ops, q, k, flags=flags, rows=rows, engine=None if rows is not None else "mfma")
    return [t.cpu().numpy() for t in out]


def _u32(a, dev):
    return torch.from_numpy(np.asarray(a, dtype=np.uint32)).to(dev)


def _reference(mode, X, qf, allowed, k, dup=()):
    """float64 scores of the allowed rows and their top-k (score desc, row asc); asserts the tie precondition."""
    A = X[allowed].astype(np.float64)
    S = qf.astype(np.float64) @ A.T
    if mode == "int8_cosine":
        nrm = np.sqrt((A ** 2).sum(axis=1))
        S = np.where(nrm > 0, S / np.where(nrm > 0, nrm, 1.0), -np.inf)
    order = np.lexsort((np.broadcast_to(allowed, S.shape), -S), axis=1)[:, :k + 1]
    top = np.take_along_axis(S, order, 1)
    for j in range(qf.shape[0]):
        keep = ~np.isin(allowed[order[j]], dup)
        v = top[j][keep].astype(np.float32)
        assert len(np.unique(v)) == len(v), "the seed gives a float32 tie among the top k + 1"
    return allowed[order[:, :k]], top[:, :k]


def _check(mode, X, qf, allowed, k, out, dup=()):
    cnt, rows, sc = out
    kc = min(k, len(allowed))
    assert np.all(cnt == kc) and np.all(rows[:, kc:] == -1) and np.all(np.isnan(sc[:, kc:]))
    if kc == 0:
        return
    ref_rows, ref = _reference(mode, X, qf, np.asarray(allowed, dtype=np.int64), k, dup)
    assert np.array_equal(rows[:, :kc], ref_rows)
    got = sc[:, :kc]
    if mode == "int8_cosine":
        assert np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref))
    else:
        r32 = ref.astype(np.float32)
        lo = np.where(r32 > ref, np.nextafter(r32, np.float32(-np.inf)), r32)
        hi = np.where(r32 < ref, np.nextafter(r32, np.float32(np.inf)), r32)
        assert np.all((got == lo) | (got == hi))


def _check_copy(mode, ops, qf, allowed, k, out, dev):
    idx = torch.from_numpy(np.asarray(allowed, dtype=np.int64)).to(dev)
    if mode == "int8_cosine":
        cops = (ops[0][idx].contiguous(), ops[1][idx].contiguous())
    else:
        cops = (ops[0][idx].contiguous(), ops[1][idx].contiguous(), ops[2][idx].contiguous(), ops[3])
    ident = _u32(np.arange(len(allowed)), dev) if qf.shape[1] == 1024 else None
    cnt, rows, sc = _search(mode, cops, qf, k, rows=ident)
    assert np.array_equal(cnt, out[0]) and np.array_equal(sc.view(np.int64), out[2].view(np.int64))
    assert np.array_equal(np.where(rows >= 0, np.asarray(allowed)[np.maximum(rows, 0)], -1), out[1])


def _case(mode, dim, n, nq, k, allowed, dev, seed, plant=None, dup=()):
    rng = np.random.default_rng(seed)
    X = _corpus(rng, mode, n, dim)
    qf = rng.standard_normal((nq, dim)).astype(np.float32)
    if plant is not None:
        plant(X, qf)
    ops = _ops(mode, X, dev)
    out = _search(mode, ops, qf, k, rows=_u32(allowed, dev))
    _check(mode, X, qf, allowed, k, out, dup)
    if len(allowed):
        _check_copy(mode, ops, qf, allowed, k, out, dev)
    return X, qf, ops, out


# (dim, n, m, nq, k): every KS instance on half the rows (m None: random, rows 0 and n - 1 allowed); tile edges, m < k
# and m = 0 (m = 97 spans four one-tile chunks, the last a single row); the smallest list whose chunks are two
# tiles long with 33 rows in the last (the shifted tile); more than one query block (nq None: the block + 2)
SHAPES = [(d, 4096, None, 3, 10) for d in DIMS] + \
    [(d, 300, m, 3, 5) for d in (256, 384, 1024, 2048) for m in (0, 1, 3, 31, 32, 33, 97)] + \
    [(d, 40000, 32768 + 64 + 33, 3, 5) for d in (256, 1536)] + [(d, 2048, 1000, None, 5) for d in (256, 2048)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dim,n,m,nq,k", SHAPES)
def test_shapes(dev, mode, dim, n, m, nq, k):
    rng = np.random.default_rng(dim + (m or 0))
    mask = rng.random(n) < 0.5
    mask[[0, n - 1]] = True
    allowed = np.flatnonzero(mask) if m is None else np.sort(rng.choice(n, m, replace=False))
    info = (C.c_int64 * 8)()
    assert N.load().vrq_gemm_topk_rows_plan(N.VRQ_GEMM_INT8_COSINE, len(allowed), dim, nq or 1, k, info) == 0
    assert m != 32768 + 64 + 33 or info[0] == 64
    _case(mode, dim, n, nq or int(info[7]) + 2, k, allowed, dev, 100 + dim + (m or 0))


@pytest.mark.parametrize("mode", MODES)
def test_the_filter_decides(dev, mode):
    """The unfiltered top of every query is a planted row: disallowed, none comes back; allowed, all do."""
    dim, n, nq, k = 384, 2000, 3, 4
    planted = np.array([5, 700, 1999])
    def plant(X, qf):
        X[planted] = _like_queries(mode, qf)
    rest = np.setdiff1d(np.arange(n)[::2], planted)
    X, qf, ops, out = _case(mode, dim, n, nq, k, rest, dev, 500, plant)
    assert not np.isin(out[1], planted).any()
    assert np.array_equal(_search(mode, ops, qf, 1)[1][:, 0], planted)  # unfiltered: they are the top
    both = np.union1d(rest, planted)
    out = _search(mode, ops, qf, k, rows=_u32(both, dev))
    _check(mode, X, qf, both, k, out)
    assert np.array_equal(out[1][:, 0], planted)


@pytest.mark.parametrize("mode", MODES)
def test_real_sample_and_tie_order(dev, mode):
    """The sample is a strict subset of the list; four copies of query 0's best row sit at virtual rows 31 | 32 (a
    tile boundary) and 63 | 64 (a chunk boundary) and come back first, in ascending physical order."""
    dim, n, m, nq, k = 256, 100000, 40000, 3, 10
    info = (C.c_int64 * 8)()
    assert N.load().vrq_flat_ip_topk_rows_plan(m, dim, nq, k, info) == 0
    assert info[0] == 64 and info[4] * info[5] < m  # chunk rows; sample chunks x rows per sample chunk
    allowed = np.sort(np.random.default_rng(7).choice(n, m, replace=False))
    dup = allowed[[31, 32, 63, 64]]
    def plant(X, qf):
        X[dup] = _like_queries(mode, qf[:1])
    X, qf, ops, out = _case(mode, dim, n, nq, k, allowed, dev, 600, plant, dup)
    assert np.array_equal(out[1][0, :4], dup) and len(np.unique(out[2][0, :4])) == 1


@pytest.mark.parametrize("mode", MODES)
def test_retry_and_fallback_through_the_list(dev, mode):
    """All rows identical, every second one allowed, at the smallest list whose chunks exceed the list capacity: every
    list overflows twice and the exact scan serves the queries through the list, or leaves them unserved."""
    dim, nq, k = 256, 2, 5
    L, info = N.load(), (C.c_int64 * 8)()
    m = next(c for c in range(1 << 15, 1 << 22, 1 << 15)
             if L.vrq_flat_ip_topk_rows_plan(c, dim, nq, k, info) == 0 and info[0] > info[2])
    rng = np.random.default_rng(700)
    row, qf = _corpus(rng, mode, 1, dim), rng.standard_normal((nq, dim)).astype(np.float32)
    ops = tuple(t.expand(2 * m, *t.shape[1:]).contiguous() if t.shape[0] == 1 else t for t in _ops(mode, row, dev))
    allowed = _u32(np.arange(0, 2 * m, 2), dev)
    assert np.all(_search(mode, ops, qf, k, rows=allowed, flags=N.VRQ_GEMM_NO_FALLBACK)[0] == -1)
    cnt, rows, sc = _search(mode, ops, qf, k, rows=allowed)
    assert np.all(cnt == k) and np.array_equal(rows, np.tile(np.arange(0, 2 * k, 2), (nq, 1)))
    _check(mode, row, qf, np.array([0]), 1, (np.ones(nq), rows[:, :1] * 0, sc[:, :1]))
    assert np.all(sc == sc[:, :1])


@pytest.mark.parametrize("n,kind", [(1000, "random"), (777, "zero"), (777, "one"), (64 * 256 * 3 + 5, "random")])
def test_row_list(dev, n, kind):
    """Ragged n with set bits past n in the last word, all-zero, all-one, and more than one scan block."""
    rng = np.random.default_rng(n)
    mask = {"random": rng.random(n) < 0.3, "zero": np.zeros(n, bool), "one": np.ones(n, bool)}[kind]
    allow = filters.row_bitmap(torch.from_numpy(mask).to(dev))
    allow[-1] |= -1 << (n % 64)  # bits at and past n: ignored
    rows = filters.row_list(allow, n)
    assert rows.dtype == torch.uint32 and np.array_equal(rows.cpu().numpy(), np.flatnonzero(mask))
    L, m = N.load(), torch.full((1,), -1, dtype=torch.int64, device=dev)  # count only
    ws = torch.empty((L.vrq_row_list_workspace_size(n),), dtype=torch.uint8, device=dev)
    assert L.vrq_row_list(N.ptr(allow), n, 0, 0, N.ptr(m), N.ptr(ws), ws.numel(), N.stream_handle(dev)) == 0
    assert int(m.item()) == int(mask.sum())


def test_classes_filtered(dev, tmp_path):
    """FloatIndexIDMap.search(allow=) and CohereVectorDBFloat.search_vectors(allowed_ids=) at 384 with engine=None:
    FAISS-order results over the allowed ids, and the unfiltered search unchanged by the first filtered call."""
    dim, n, nq, k = 384, 1500, 3, 5
    rng = np.random.default_rng(800)
    X, qf = _corpus(rng, "float_ip", n, dim), rng.standard_normal((nq, dim)).astype(np.float32)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    mask = rng.random(n) < 0.4
    allowed = np.flatnonzero(mask)
    ref_rows, ref = _reference("float_ip", X, qf, allowed, k)
    idx = FloatIndexIDMap(dim, dev)
    idx.add_with_ids(X[:1000], ids[:1000])
    D0, L0 = idx.search(qf, k)
    D, Lb = idx.search(qf, k, allow=filters.row_bitmap(torch.from_numpy(mask[:1000]).to(dev)))
    assert np.isin(Lb, ids[:1000][mask[:1000]]).all()
    idx.add_with_ids(X[1000:], ids[1000:])  # the operands the filtered search prepared keep up
    D, Lb = idx.search(qf, k, allow=filters.row_bitmap(torch.from_numpy(mask).to(dev)))
    assert np.array_equal(Lb, ids[ref_rows]) and np.all(np.abs(D - ref) <= np.spacing(np.abs(ref).astype(np.float32)))
    assert idx.engine is None
    idx.remove_ids(ids[1000:])
    D3, L3 = idx.search(qf, k)  # unfiltered after the filtered calls: the same route and bits as before them
    assert np.array_equal(D0, D3) and np.array_equal(L0, L3)
    db = CohereVectorDBFloat(str(tmp_path / "db"), embedding_dim=dim, provider=object(), device=dev)
    db.add_vectors(ids, X)
    cnt, got, sc = db.search_vectors(qf, k, allowed_ids=ids[allowed])
    assert np.all(cnt.cpu().numpy() == k) and np.array_equal(got.cpu().numpy(), ids[ref_rows])
    assert np.array_equal(sc.cpu().numpy().astype(np.float32), D)
