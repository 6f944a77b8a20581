"""K1g: the counting scan over an ascending row list (vrq_*_gather), on both engines.  Every comparison is exact.

Corpus: 40 000 rows, 17 queries that are a base vector with a few signs flipped.  Rows 15 000 .. 18 000 all carry
one code, an eighth of the dim away from the base: for every query they are one tie group, nearer than the random
rows (about dim / 2 away), so the cut at T falls inside it for K = 100 and K = 1500, and in every multi-chunk list
it lies in a middle chunk.  Forty scattered rows are nearer still (the dist < T part).  The reference is NumPy:
xor + popcount over the listed rows, lexsort by (dist, row)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS, NQ, M = 40000, 17, 3 * 4096 + 37
DIMS = (256, 384, 1024, 2048)
ENGINES = ("valu", "mfma")
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


_rng = np.random.default_rng(5)
LISTS = {
    "random": np.sort(_rng.choice(N_ROWS, M, replace=False)),
    "third": np.arange(0, N_ROWS, 3),
    "range": np.arange(14990, 14990 + 5003),   # starts and ends mid-tile, holds the tie group
    "first": np.array([0]), "last": np.array([N_ROWS - 1]), "empty": np.array([], np.int64),
    "m700": np.sort(_rng.choice(np.arange(14000, 19000), 700, replace=False)),   # m < K = 1500
    "identity": np.arange(M),
}
_corpus = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def corpus(dev, dim):
    if dim not in _corpus:
        rng = np.random.default_rng(dim)
        flip = lambda v, k: v * np.where(np.isin(np.arange(dim), rng.choice(dim, k, replace=False)), -1, 1)
        base = rng.standard_normal(dim)
        x = rng.standard_normal((N_ROWS, dim), dtype=np.float32)
        x[15000:18000] = np.abs(rng.standard_normal((3000, dim))) * np.sign(flip(base, dim // 8))
        for r in rng.choice(N_ROWS, 40, replace=False):
            x[r] = flip(base, dim // 16)
        qf = np.stack([flip(base, 2 * j) for j in range(NQ)]).astype(np.float32)
        codes, qb = np.packbits(x > 0, axis=1), np.packbits(qf > 0, axis=1)
        x8 = np.clip(np.rint(x * 40), -127, 127).astype(np.int8)
        rr = np.arange(N_ROWS, dtype=np.int64)
        rr[0:35000:7] = rr[3:35003:7]   # duplicated ids: a row rescored from another row's vector
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        _corpus[dim] = dict(dim=dim, codes=t(codes), qb=t(qb), qf=t(qf), x8=t(x8), rr=t(rr),
                            norms=t(np.sqrt((x8.astype(np.float32) ** 2).sum(1, dtype=np.float64))),
                            dmat=np.stack([POP[codes ^ q].sum(1) for q in qb]))
    return _corpus[dim]


def reference(c, rows, K):
    """(dist i32 [NQ, K], row i64 [NQ, K]) of the listed rows by (dist, row); INT32_MAX / -1 past the list."""
    D = np.full((NQ, K), np.iinfo(np.int32).max, np.int32)
    R = np.full((NQ, K), -1, np.int64)
    for q in range(NQ):
        d = c["dmat"][q, rows]
        o = np.lexsort((rows, d))[:K]
        D[q, :len(o)], R[q, :len(o)] = d[o], rows[o]
    return D, R


def lib_engine(engine):
    from vectorragquantization_amd import _native as N
    return N, N.load(), {"valu": N.VRQ_LARGE_ENGINE_VALU, "mfma": N.VRQ_LARGE_ENGINE_MFMA}[engine]


dev_rows = lambda dev, rows: torch.from_numpy(rows.astype(np.uint32)).to(dev)
outputs = lambda dev, shapes: [torch.full(s, -7, dtype=t, device=dev) for s, t in shapes]
bits = lambda x: x.view(torch.int64) if x.dtype == torch.float64 else x


def bitmap(dev, rows):
    mask = np.zeros((N_ROWS + 63) // 64 * 64, bool)
    mask[rows] = True
    return torch.from_numpy(np.packbits(mask, bitorder="little").view(np.int64)).to(dev)


@pytest.mark.parametrize("name", LISTS)
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("dim", DIMS)
def test_hamming_topk_gather_is_the_reference(dev, dim, engine, name):
    N, lib, e = lib_engine(engine)
    c, rows = corpus(dev, dim), LISTS[name]
    m, r = len(rows), dev_rows(dev, rows)
    if name == "random":   # the shape the list was made for: at least 3 chunks and a ragged last tile
        info = (C.c_int64 * 10)()
        N.check(lib.vrq_scan_gather_plan(m, dim, NQ, 1500, e, info), "plan")
        assert info[0] == e and info[2] >= 3 and m % 64 != 0
    for K in (100, 1500):
        D, R = outputs(dev, [((NQ, K), torch.int32), ((NQ, K), torch.int64)])
        ws = torch.empty((lib.vrq_hamming_topk_gather_workspace_size(m, dim // 8, NQ, K),), dtype=torch.uint8,
                         device=dev)
        N.check(lib.vrq_hamming_topk_gather(N.ptr(c["codes"]), N_ROWS, dim // 8, 0, N.ptr(c["qb"]), NQ, K,
                                            N.ptr(r) if m else 0, m, N.ptr(D), N.ptr(R), N.ptr(ws), ws.numel(),
                                            N.stream_handle(dev), e), "gather")
        torch.cuda.synchronize()
        wd, wr = reference(c, rows, K)
        assert np.array_equal(R.cpu().numpy(), wr)
        assert np.array_equal(D.cpu().numpy(), wd)
        assert ((wr >= 0).sum(1) == min(K, m)).all()   # counts (m < K gives lists of length m)


@pytest.mark.parametrize("name", LISTS)
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("dim", DIMS)
def test_search_gather_is_the_batch_call_with_the_bitmap(dev, dim, engine, name):
    N, lib, e = lib_engine(engine)
    c, rows = corpus(dev, dim), LISTS[name]
    m, r, allow = len(rows), dev_rows(dev, rows), bitmap(dev, rows)
    k, K, K3 = 10, 1500, 30
    wsb = torch.empty((lib.vrq_search3_batch_workspace_size(N_ROWS, dim, NQ, K),), dtype=torch.uint8, device=dev)
    wsg = torch.empty((max(8, lib.vrq_search3_gather_workspace_size(m, dim, NQ, K)),), dtype=torch.uint8, device=dev)
    s = N.stream_handle(dev)
    p = lambda key: N.ptr(c[key])
    o3 = [((NQ,), torch.int32), ((NQ, k), torch.int64), ((NQ, k), torch.int32), ((NQ, k), torch.float64),
          ((NQ, k), torch.float64)]
    head3 = (p("codes"), p("x8"), p("norms"), p("rr"), N_ROWS, dim, 5, p("qf"), p("qb"), NQ, k, K, K3, 0)
    head2 = (N.VRQ_RESCORE_SIGNED_BINARY, p("codes"), p("codes"), 0, 0.0, p("rr"), N_ROWS, dim, 5, p("qf"), p("qb"),
             NQ, k, K, 0)
    for fn, head, shapes in (("vrq_search3", head3, o3), ("vrq_search2", head2, o3[:4])):
        a, b = outputs(dev, shapes), outputs(dev, shapes)
        N.check(getattr(lib, fn + "_gather")(*head, N.ptr(r) if m else 0, m, *map(N.ptr, a), N.ptr(wsg), wsg.numel(),
                                             s, e), fn + "_gather")
        N.check(getattr(lib, fn + "_batch")(*head, N.ptr(allow), *map(N.ptr, b), N.ptr(wsb), wsb.numel(), s, e),
                fn + "_batch")
        torch.cuda.synchronize()
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
        assert int(b[0].min()) == min(k, m)


@pytest.mark.parametrize("engine", (None, "valu", "mfma"))
def test_python_rows_and_filter_route(tmp_path, dev, engine):
    from vectorragquantization_amd import filters
    from vectorragquantization_amd.binary import CohereVectorDBBinary
    from vectorragquantization_amd.embed import TableProvider
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    c, rows = corpus(dev, 384), LISTS["random"]
    ids = np.arange(N_ROWS, dtype=np.int64) * 3 + 11
    ix = BinaryIndexIDMap2(384, device=dev)
    ix.add_with_ids(c["codes"], ids)
    allow = bitmap(dev, rows)
    lst = filters.row_list(allow, N_ROWS)
    assert np.array_equal(lst.cpu().numpy(), rows)
    for k in (10, 1500):
        want = ix.search(c["qb"], k, allow=allow, engine=engine)
        got = ix.search(c["qb"], k, rows=lst, engine=engine)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    with pytest.raises(Exception):
        ix.search(c["qb"], 10, allow=allow, rows=lst)
    x = c["qf"].cpu().numpy()
    db = CohereVectorDBBinary(str(tmp_path / "db"), embedding_dim=384, provider=TableProvider({"q": x[0]}), device=dev)
    docs = np.random.default_rng(1).standard_normal((600, 384)).astype(np.float32)
    db.add_vectors(np.arange(600) + 10, docs, [f"doc {i}" for i in range(600)])
    S = list(range(15, 400, 2))
    want = db.search_vectors(x, 30, 10, allowed_ids=S, engine=engine)
    got = db.search_vectors(x, 30, 10, allowed_ids=S, engine=engine, filter_route="gather")
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want))
    with pytest.raises(Exception):
        db.search_vectors(x, 30, 10, allowed_ids_per_query=[S] * NQ, filter_route="gather")
