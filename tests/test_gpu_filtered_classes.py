"""``allowed_ids`` on the classes: a filtered search equals the same search on a second instance that holds only
the allowed documents (ids equal, scores and distances bit-equal); naming every document equals the unfiltered
search; an empty or unknown-only set finds nothing.  A few hundred synthetic documents at dims 1024 and 384."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_DOCS = 600
NQ = 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _floats(d, seed):
    """Clustered float rows and queries near some of them; ids are not the row numbers."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((16, d)) / np.sqrt(d)
    F = (C[rng.integers(0, 16, N_DOCS)] + (0.5 / np.sqrt(d)) * rng.standard_normal((N_DOCS, d))).astype(np.float32)
    Q = (F[rng.integers(0, N_DOCS, NQ)] + (0.1 / np.sqrt(d)) * rng.standard_normal((NQ, d))).astype(np.float32)
    ids = (rng.permutation(5000)[:N_DOCS] + 10).astype(np.int64)
    S = np.sort(rng.choice(ids, 220, replace=False))
    return F, Q, ids, S


def _bits(x):
    x = x.cpu().numpy()
    return x.view(np.int64) if x.dtype == np.float64 else x


def _same_hits(got, want):
    """Tuples of [nq, kk] tensors, ids first: the same hits per query, bit for bit, whatever the padded widths."""
    gi, wi = got[0].cpu().numpy(), want[0].cpu().numpy()
    for q in range(gi.shape[0]):
        m = int((wi[q] != -1).sum())
        assert int((gi[q] != -1).sum()) == m and m > 0
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g[q])[:m], _bits(w[q])[:m])


@pytest.mark.parametrize("d", (1024, 384))
def test_enhanced_allowed_ids(tmp_path, dev, d):
    from vectorragquantization_amd.embed import SyntheticCohereProvider
    from vectorragquantization_amd.enhanced import CohereEnhancedVectorDB
    from vectorragquantization_amd.quant import encode
    F, Q, ids, S = _floats(d, d)
    e = encode("cohere", F, 0.1, dev)
    eq = encode("cohere", Q, 0.1, dev)
    prov = SyntheticCohereProvider(dim=d, device=dev)
    db = CohereEnhancedVectorDB(str(tmp_path / "all"), embedding_dim=d, provider=prov, device=dev)
    db.add_vectors(ids, e["q"], e["codes"], [f"doc {i}" for i in ids])
    keep = torch.from_numpy(np.isin(ids, S)).to(dev)
    only = CohereEnhancedVectorDB(str(tmp_path / "only"), embedding_dim=d, provider=prov, device=dev)
    only.add_vectors(ids[keep.cpu().numpy()], e["q"][keep], e["codes"][keep])
    qf, qb = torch.from_numpy(Q).to(dev), eq["codes"]
    fields = lambda r: (r.doc_id, r.hamming, r.binary, r.cosine)
    for k, bo in ((10, 10), (30, 10), (150, 10)):               # K = 100, 300 and min(1500, ntotal)
        a = db.search_vectors(qf, qb, k, bo, 3, allowed_ids=S.tolist() + [7, 9_999_999])   # unknown ids: ignored
        b = only.search_vectors(qf, qb, k, bo, 3)
        torch.cuda.synchronize()
        assert np.array_equal(a.count.cpu().numpy(), b.count.cpu().numpy())
        _same_hits(fields(a), fields(b))
        assert np.isin(a.doc_id.cpu().numpy()[a.doc_id.cpu().numpy() != -1], S).all()
    a = db.search_vectors(qf, qb, 10, 10, 3, allowed_ids=ids)   # every document: the unfiltered search
    b = db.search_vectors(qf, qb, 10, 10, 3)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip((a.count, a.row) + fields(a), (b.count, b.row) + fields(b)))
    for none in ([], [7, 9_999_999]):                           # an empty set, unknown ids only
        r = db.search_vectors(qf, qb, 10, 10, 3, allowed_ids=none)
        assert (r.count == 0).all() and (r.doc_id == -1).all() and r.to_dicts() == [[]] * NQ
        assert db.search("anything", allowed_ids=none) == []
    hits = db.search("a query", k=5, allowed_ids=S)
    assert len(hits) == 5 and all(h["doc_id"] in set(S.tolist()) for h in hits)
    assert list(hits[0]) == ["doc_id", "score_hamming", "score_binary", "score_cosine", "doc"]
    assert [h["doc"] for h in hits] == [f"doc {h['doc_id']}" for h in hits]
    strip = lambda hs: [{a: b for a, b in h.items() if a != "doc"} for h in hs]   # (`only` was given no texts)
    assert strip(hits) == strip(only.search("a query", k=5))


@pytest.mark.parametrize("cls,d", [("VectorDBInt8", 1024), ("VectorDBInt4Global", 384), ("VectorDBInt16", 384)])
def test_vectordb_allowed_ids(tmp_path, dev, cls, d):
    from vectorragquantization_amd import vectordb
    from vectorragquantization_amd.embed import TableProvider
    F, Q, ids, S = _floats(d, d + 1)
    if cls == "VectorDBInt16":
        F, Q = (F * 20000).astype(np.int16), (Q * 20000).astype(np.int16)
    make = lambda name, table: getattr(vectordb, cls)(str(tmp_path / name), embedding_dim=d,
                                                       provider=TableProvider(table), device=dev)
    db = make("all", {"the query": Q[0]})
    db.add_vectors(ids, F, [f"doc {i}" for i in ids])
    keep = np.isin(ids, S)
    only = make("only", {"the query": Q[0]})
    only.add_vectors(ids[keep], F[keep], [f"doc {i}" for i in ids[keep]])
    modes = (False,) if cls == "VectorDBInt16" else (False, True)
    for cf in modes:
        for k, bo in ((10, 10), (30, 10), (150, 10)):
            a = db.search_vectors(Q, k, bo, cf, allowed_ids=S.tolist() + [7])
            b = only.search_vectors(Q, k, bo, cf)
            torch.cuda.synchronize()
            _same_hits((a[0], a[2], a[3]), (b[0], b[2], b[3]))
        a = db.search_vectors(Q, 10, 10, cf, allowed_ids=ids.tolist())
        b = db.search_vectors(Q, 10, 10, cf)
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    for none in ([], [7, 9_999_999]):
        r = db.search_vectors(Q, 10, 10, allowed_ids=none)
        assert (r[0] == -1).all() and (r[1] == -1).all()
        assert db.search("the query", allowed_ids=none) == []
    hits = db.search("the query", k=5, allowed_ids=S)
    assert hits == only.search("the query", k=5) and len(hits) == 5
    assert list(hits[0]) == ["doc_id", "score", "doc"]


@pytest.mark.parametrize("d", (1024, 384))
def test_binary_class_allowed_ids(tmp_path, dev, d):
    from vectorragquantization_amd.binary import CohereVectorDBBinary
    from vectorragquantization_amd.embed import TableProvider
    F, Q, ids, S = _floats(d, d + 2)
    make = lambda name: CohereVectorDBBinary(str(tmp_path / name), embedding_dim=d,
                                             provider=TableProvider({"the query": Q[0]}), device=dev)
    db, only = make("all"), make("only")
    db.add_vectors(ids, F, [f"doc {i}" for i in ids])
    keep = np.isin(ids, S)
    only.add_vectors(ids[keep], F[keep], [f"doc {i}" for i in ids[keep]])
    for cf in (False, True):
        for k, bo in ((10, 10), (30, 10), (150, 10)):
            a = db.search_vectors(Q, k, bo, cf, allowed_ids=S)
            b = only.search_vectors(Q, k, bo, cf)
            torch.cuda.synchronize()
            _same_hits((a[0], a[2], a[3]), (b[0], b[2], b[3]))
        a = db.search_vectors(Q, 10, 10, cf, allowed_ids=ids)
        b = db.search_vectors(Q, 10, 10, cf)
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    for none in ([], [7, 9_999_999]):
        r = db.search_vectors(Q, 10, 10, allowed_ids=none)
        assert (r[0] == -1).all() and (r[1] == -1).all()
        assert db.search("the query", allowed_ids=none) == []
    hits = db.search("the query", k=5, allowed_ids=S)
    assert hits == only.search("the query", k=5) and len(hits) == 5
