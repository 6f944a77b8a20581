"""GPU parity of the exact exhaustive top-k at every embedding dim (K5d behind vrq_gemm_topk_dim /
vrq_flat_ip_topk_dim, FloatIndexIDMap(d), CohereVectorDBFloat(embedding_dim=)) against the oracle
(oracle_np.exhaustive_scores / exhaustive_topk / flat_ip_scores / flat_ip_search).

Exactness inputs: Gaussian values rounded to a grid of 2^-20, queries clipped to |q| < 8, float rows to
|x| < 1.  They are exact in float32, every product is a multiple of 2^-40 (2^-20 for +-1 and int8
operands) and the largest sum at d = 2048 needs 51 bits, so the float64 sum is exact in every order:
the GPU's scores and rows must equal the oracle's, no tolerance.  For the cosine mode the norms are
uploaded from oracle_np.int8_row_norms, so the division's operands are the same on both sides."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

DIMS = (256, 384, 512, 768, 1536, 2048)
MODES = ("binary", "int8_cosine", "float_ip")
G = 2.0 ** -20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _mode_id(mode):
    from vectorragquantization_amd import _native as N
    return {"binary": N.VRQ_GEMM_BINARY, "int8_cosine": N.VRQ_GEMM_INT8_COSINE, "float_ip": N.VRQ_GEMM_FLOAT_IP}[mode]


def _plan(mode, n, dim, nq, k):
    from vectorragquantization_amd import _native as N
    info = (C.c_int64 * 6)()
    assert N.load().vrq_gemm_topk_dim_plan(_mode_id(mode), n, dim, nq, k, info) == N.VRQ_OK
    return [int(v) for v in info]  # tile, chunk rows, chunks, queries per workgroup, capacity, bytes


def _grid(rng, shape, sigma, clip):
    x = np.round(rng.standard_normal(shape) * sigma / G) * G
    return np.clip(x, -(clip - G), clip - G).astype(np.float32)


def _grid_queries(rng, nq, dim):
    return _grid(rng, (nq, dim), 1.0, 8.0)


def _rows(rng, mode, n, dim, exact=True):
    """The row operand of a mode (numpy): codes u8[n, dim/8], x8 i8[n, dim] or xf f32[n, dim]."""
    if mode == "binary":
        return rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
    if mode == "int8_cosine":
        return rng.integers(-127, 128, (n, dim), dtype=np.int8)
    if exact:
        return _grid(rng, (n, dim), 0.25, 1.0)
    F = rng.standard_normal((n, dim))
    return (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)


def _oracle_scores(mode, X, qf):
    if mode == "binary":
        return O.exhaustive_scores("binary", qf, codes=X)
    if mode == "int8_cosine":
        return O.exhaustive_scores("int8_cosine", qf, x8=X)
    return O.flat_ip_scores(X, qf)


def _oracle(mode, X, qf, k):
    S = _oracle_scores(mode, X, qf)
    rows = O.exhaustive_topk(S, k)
    if mode == "float_ip":
        sc2, rows2 = O.flat_ip_search(X, qf, k)
        assert np.array_equal(rows, rows2) and np.array_equal(np.take_along_axis(S, rows, 1), sc2)
    return S, rows, np.take_along_axis(S, rows, 1)


def _upload(mode, X, dev):
    t = torch.from_numpy(X).to(dev)
    norms = torch.from_numpy(O.int8_row_norms(X)).to(dev) if mode == "int8_cosine" else None
    return t, norms


def _run(mode, Xd, norms, qf, k, dev, row_offset=0, flags=0, workspace=None):
    from vectorragquantization_amd.enhanced import gemm_topk
    from vectorragquantization_amd.flat import flat_ip_topk
    q = torch.from_numpy(np.ascontiguousarray(qf)).to(dev)
    if mode == "float_ip":
        cnt, rows, sc = flat_ip_topk(Xd, None, None, None, q, k, row_offset=row_offset, flags=flags, workspace=workspace)
    elif mode == "binary":
        cnt, rows, sc = gemm_topk("binary", q, k, codes=Xd, row_offset=row_offset, flags=flags, workspace=workspace)
    else:
        cnt, rows, sc = gemm_topk("int8_cosine", q, k, x8=Xd, norms=norms, row_offset=row_offset, flags=flags,
                                  workspace=workspace)
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy()


def _assert_exact(mode, X, qf, k, out, row_offset=0):
    cnt, rows, sc = out
    _, ref_rows, ref_sc = _oracle(mode, X, qf, k)
    m = min(k, X.shape[0])
    assert np.all(cnt == m), cnt
    assert np.array_equal(rows[:, :m] - row_offset, ref_rows)
    assert np.array_equal(sc[:, :m], ref_sc)
    assert np.all(rows[:, m:] == -1) and np.all(np.isnan(sc[:, m:]))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mode", MODES)
def test_exact_parity_all_dims(dev, mode, dim):
    k = 10
    qb = _plan(mode, 200_000, dim, 1024, k)[3]
    nq = qb + 1
    tile = _plan(mode, 200_000, dim, nq, k)[0]
    n = None
    for m in range(1, 200_000 // tile):               # walk up in tile steps, ragged last tile
        cand = m * tile + 7
        p = _plan(mode, cand, dim, nq, k)
        if p[2] >= 3 and cand % p[0] != 0:
            n = cand
            break
    assert n is not None, "no n <= 200000 with >= 3 chunks and a ragged last tile"
    assert _plan(mode, n, dim, nq, k)[3] == qb        # two query blocks, the second with one query
    rng = np.random.default_rng(1000 + dim)
    X, qf = _rows(rng, mode, n, dim), _grid_queries(rng, nq, dim)
    Xd, norms = _upload(mode, X, dev)
    out = _run(mode, Xd, norms, qf, k, dev)
    assert np.all(out[0] == 10)
    _assert_exact(mode, X, qf, k, out)


@pytest.mark.parametrize("dim", (384, 2048))
@pytest.mark.parametrize("mode", MODES)
def test_multi_tile_chunks(dev, mode, dim):
    """Chunks of several tiles (the running k-th key prunes across tiles) and many query blocks."""
    n, nq, k = 20_000, 300, 10
    p = _plan(mode, n, dim, nq, k)
    assert p[1] >= 3 * p[0] and p[2] >= 3
    rng = np.random.default_rng(7 + dim)
    X, qf = _rows(rng, mode, n, dim), _grid_queries(rng, nq, dim)
    Xd, norms = _upload(mode, X, dev)
    _assert_exact(mode, X, qf, k, _run(mode, Xd, norms, qf, k, dev))


@pytest.mark.parametrize("mode", MODES)
def test_shape_edges(dev, mode):
    for dim in (256, 2048):
        tile = _plan(mode, 1000, dim, 1, 10)[0]
        rng = np.random.default_rng(5 + dim)
        Xall, qall = _rows(rng, mode, tile + 1, dim), _grid_queries(rng, 3, dim)
        for n in (1, tile - 1, tile, tile + 1):
            X = np.ascontiguousarray(Xall[:n])
            Xd, norms = _upload(mode, X, dev)
            for k in (1, 10):
                for nq in (1, 3):
                    out = _run(mode, Xd, norms, qall[:nq], k, dev)
                    assert np.all(out[0] == min(k, n))
                    _assert_exact(mode, X, qall[:nq], k, out)


@pytest.mark.parametrize("mode", MODES)
def test_ties_and_specials(dev, mode):
    for dim in (384, 1536):
        rng = np.random.default_rng(11 + dim)
        nq = 12
        p = _plan(mode, 3000, dim, nq, 10)
        n = 3000
        assert p[2] >= 2
        X = _rows(rng, mode, n, dim)
        a, b, c = 5, 40, p[1] + 9                     # two in the first tile, one in a later chunk
        assert b < p[0] and c < n
        X[b] = X[a]
        X[c] = X[a]
        if mode == "int8_cosine":
            zero_rows = [3, 70, 71, p[1] + 1, n - 1]
            X[zero_rows] = 0
        qf = _grid_queries(rng, nq, dim)
        # a query equal to the planted row (its top scores are the three copies, in row order)
        if mode == "binary":
            qf[0] = (np.abs(qf[0]) + G) * (2.0 * np.unpackbits(X[a]) - 1.0)
        elif mode == "int8_cosine":
            qf[0] = X[a].astype(np.float32) / 32.0
        else:
            qf[0] = X[a]
        qf[1] = 0.0
        qf[1, ::3] = -0.0                             # every score is +-0: rows 0..k-1
        Xd, norms = _upload(mode, X, dev)
        S = _oracle_scores(mode, X, qf)
        top3 = O.exhaustive_topk(S[:1], 3)[0]
        assert sorted(top3.tolist()) == [a, b, c] and S[0, a] == S[0, b] == S[0, c]
        for k in (2, 10):                             # k = 2 cuts through the tie group
            out = _run(mode, Xd, norms, qf, k, dev)
            _assert_exact(mode, X, qf, k, out)
            assert out[1][0, :2].tolist() == [a, b]
            if mode != "int8_cosine":
                assert out[1][1].tolist() == list(range(k))
        if mode == "int8_cosine":               # k reaches two of the -inf rows: after every finite row, row order
            Xs = np.ascontiguousarray(X[:1000])       # the first 1000 rows hold four of the zero rows
            Xd2, norms2 = _upload(mode, Xs, dev)
            out = _run(mode, Xd2, norms2, qf, 999, dev)
            _assert_exact(mode, Xs, qf, 999, out)
            zr = sorted(z for z in zero_rows if z < 1000)
            nfin = 1000 - len(zr)
            assert 2 <= 999 - nfin < len(zr)
            assert np.all(np.isfinite(out[2][:, :nfin])) and np.all(np.isneginf(out[2][:, nfin:999]))
            assert np.all(out[1][:, nfin:999] == np.array(zr[:999 - nfin]))


@pytest.mark.parametrize("dim", (256, 2048))
@pytest.mark.parametrize("mode", MODES)
def test_k_1024(dev, mode, dim):
    n, nq, k = 5000, 3, 1024
    rng = np.random.default_rng(13 + dim)
    X, qf = _rows(rng, mode, n, dim), _grid_queries(rng, nq, dim)
    Xd, norms = _upload(mode, X, dev)
    _assert_exact(mode, X, qf, k, _run(mode, Xd, norms, qf, k, dev))


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


@pytest.mark.parametrize("mode", MODES)
def test_gaussian_inputs_tolerance(dev, mode):
    """Unrounded unit-norm Gaussian data: the float64 sums are no longer exact, so the two sides may
    differ by their summation error -- one float32 ulp after the rounding (cosine: of the dot, carried
    through the division), 2 * d * 2^-53 * sum|q_i| for the binary mode's float64 score."""
    dim, n, nq, k = 768, 20_000, 40, 10
    rng = np.random.default_rng(17)
    X = _rows(rng, mode, n, dim, exact=False)
    qf = rng.standard_normal((nq, dim))
    qf = (qf / np.linalg.norm(qf, axis=1, keepdims=True)).astype(np.float32)
    Xd, norms = _upload(mode, X, dev)
    cnt, rows, sc = _run(mode, Xd, norms, qf, k, dev)
    S, ref_rows, ref_sc = _oracle(mode, X, qf, k)
    nrm = O.int8_row_norms(X) if mode == "int8_cosine" else None
    for q in range(nq):
        def tol(r):
            if mode == "binary":
                return np.full(len(r), 2.0 * dim * 2.0 ** -53 * np.abs(qf[q].astype(np.float64)).sum())
            if mode == "int8_cosine":
                return _ulp32(S[q, r] * nrm[r]) / nrm[r] * (1 + 2.0 ** -50)
            return _ulp32(S[q, r])
        assert cnt[q] == k
        r = rows[q]
        assert np.all(np.abs(sc[q] - S[q, r]) <= tol(r)), q            # the score of its own row
        assert np.all(np.abs(sc[q] - ref_sc[q]) <= tol(ref_rows[q])), q  # the oracle's score at the same rank
        bad = np.nonzero(r != ref_rows[q])[0]
        assert np.all(np.abs(S[q, r[bad]] - S[q, ref_rows[q][bad]]) <= tol(ref_rows[q][bad])), (q, bad)
        assert np.all(np.diff(sc[q]) <= 0), q


@pytest.mark.parametrize("mode", MODES)
def test_scan_exact_at_1024_equals_matrix_path(dev, mode):
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd.flat import flat_ip_prepare, flat_ip_topk
    dim, n, nq, k = 1024, 20_000, 40, 10
    rng = np.random.default_rng(19)
    X, qf = _rows(rng, mode, n, dim), _grid_queries(rng, nq, dim)
    Xd, norms = _upload(mode, X, dev)
    exact = _run(mode, Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_SCAN_EXACT)
    if mode == "float_ip":
        bounds = torch.zeros((2,), dtype=torch.float64, device=dev)
        x8, inv = flat_ip_prepare(Xd, bounds)
        cnt, rows, sc = flat_ip_topk(Xd, x8, inv, bounds, torch.from_numpy(qf).to(dev), k)
        torch.cuda.synchronize()
        matrix = (cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy())
    else:
        matrix = _run(mode, Xd, norms, qf, k, dev)       # forwards to vrq_gemm_topk
    assert np.array_equal(exact[0], matrix[0])
    assert np.array_equal(exact[1], matrix[1])
    assert np.array_equal(exact[2].view(np.int64), matrix[2].view(np.int64))   # score bits
    _assert_exact(mode, X, qf, k, exact)
    _assert_exact(mode, X, qf, k, matrix)


def test_row_ranges_merge_equal_single(dev):
    from vectorragquantization_amd.dist import merge_topk_shards
    dim, n, nq, k = 512, 6000, 9, 10
    for mode in MODES:
        rng = np.random.default_rng(23)
        X, qf = _rows(rng, mode, n, dim), _grid_queries(rng, nq, dim)
        X[4100] = X[17]                                   # a tie across the two ranges
        tile = _plan(mode, n, dim, nq, k)[0]
        cut = 37 * tile + 21
        Xd, norms = _upload(mode, X, dev)
        single = _run(mode, Xd, norms, qf, k, dev, row_offset=1000)
        parts = []
        for a, b in ((0, cut), (cut, n)):
            nr = norms[a:b] if norms is not None else None
            parts.append(_run(mode, Xd[a:b], nr, qf, k, dev, row_offset=1000 + a))
        cntm, rows, sc = merge_topk_shards(torch.from_numpy(np.stack([p[1] for p in parts])),
                                           torch.from_numpy(np.stack([p[2] for p in parts])), k)
        rows, sc = rows.numpy(), sc.numpy()
        assert np.array_equal(cntm.numpy(), single[0])
        assert np.array_equal(rows, single[1]) and np.array_equal(sc, single[2])
        _assert_exact(mode, X, qf, k, single, row_offset=1000)


def test_repeatable(dev):
    from vectorragquantization_amd import _native as N
    dim, n, nq, k = 768, 10_000, 20, 100
    for mode in MODES:
        rng = np.random.default_rng(29)
        X = _rows(rng, mode, n, dim, exact=False)
        qf = rng.standard_normal((nq, dim)).astype(np.float32)
        Xd, norms = _upload(mode, X, dev)
        need = N.load().vrq_gemm_topk_dim_workspace_size(_mode_id(mode), n, dim, nq, k)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        a = _run(mode, Xd, norms, qf, k, dev, workspace=ws)
        b = _run(mode, Xd, norms, qf, k, dev, workspace=ws)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                  y.view(np.int64) if y.dtype == np.float64 else y)


def test_float_index_and_class_surface(dev, tmp_path):
    from vectorragquantization_amd.embed import SyntheticCohereProvider
    from vectorragquantization_amd.flat import CohereVectorDBFloat, FloatIndexIDMap
    d = 384
    rng = np.random.default_rng(31)
    F = _grid(rng, (700, d), 0.25, 1.0)
    ids = np.arange(700, dtype=np.int64) * 3 + 5
    idx, ref = FloatIndexIDMap(d, dev), O.IndexFlatIPIDMap(d)
    for a, b in ((0, 100), (100, 101), (101, 700)):                    # three batches
        idx.add_with_ids(F[a:b], ids[a:b])
        ref.add_with_ids(F[a:b], ids[a:b])
    gone = ids[[50, 650]]
    assert idx.remove_ids(gone) == ref.remove_ids(gone) == 2
    idx.add_with_ids(F[50:51], ids[50:51])                              # re-add one: it moves to the end
    ref.add_with_ids(F[50:51], ids[50:51])
    assert idx.ntotal == ref.ntotal == 699
    assert np.array_equal(idx.reconstruct(int(ids[50])), F[50])
    idx.write(str(tmp_path / "index.faiss"))
    idx2 = FloatIndexIDMap.read(str(tmp_path / "index.faiss"), dev)
    assert idx2.d == d and idx2.ntotal == 699
    q = _grid_queries(rng, 5, d)
    Dr, Lr = ref.search(q, 20)
    for ix in (idx, idx2):
        D, L = ix.search(q, 20)
        assert np.array_equal(L, Lr) and np.array_equal(D, Dr)
    cnt, rows, sc = idx.search_rows(q, 7)
    torch.cuda.synchronize()
    assert np.array_equal(idx.id_map.cpu().numpy()[rows.cpu().numpy()], Lr[:, :7])
    with pytest.raises(ValueError, match="vrq_dim_supported"):
        FloatIndexIDMap(1000, dev)

    # the class, as test_cohere_vector_db_float_surface drives it at 1024
    prov = SyntheticCohereProvider(dim=d)
    docs = [f"document number {i} about topic {i % 7}" for i in range(300)]
    db = CohereVectorDBFloat(str(tmp_path / "db"), embedding_dim=d, provider=prov, device=dev)
    db.add_documents(list(range(300)), docs, batch_size=64, save=True)
    assert len(db) == 300
    res = db.search("document number 42 about topic 0", k=5)
    E = prov.float_embeddings(docs)
    qe = prov.float_embeddings(["document number 42 about topic 0"])
    sc, rows = O.flat_ip_search(E, qe, 5)
    assert [r["doc_id"] for r in res] == rows[0].tolist()
    assert all(abs(r["score"] - s) <= 1e-6 for r, s in zip(res, sc[0]))
    assert res[0]["doc"] == docs[rows[0][0]]
    db.remove_document(int(rows[0][0]))
    assert len(db) == 299 and int(rows[0][0]) not in [r["doc_id"] for r in db.search(docs[0], k=50)]
    db2 = CohereVectorDBFloat(str(tmp_path / "db"), embedding_dim=d, provider=prov, device=dev)
    assert len(db2) == 299 and db2.index.d == d
    assert db2.search(docs[3], k=3) == db.search(docs[3], k=3)
    with pytest.raises(ValueError, match="vrq_dim_supported"):
        CohereVectorDBFloat(str(tmp_path / "db1000"), embedding_dim=1000, provider=prov, device=dev)
