"""GPU parity of the search at embedding dims other than 1024 (256, 384, 512, 768, 1536, 2048 = code
bytes 32, 48, 64, 96, 192, 256): the Phase-I scan K1d and its merge against the C restatement of FAISS
hammings_knn_hc, the three-phase search against the reference's own golden tables (384, 1536:
tests/golden/make_golden_dims.py) and the NumPy oracle (the other dims), the stand-alone rescoring, the
1024 forwarders, and the class surface.  Integers and Phase-II scores exact, cosine within ``cos_close``,
certified Phase-III tie permutations on at most MAX_TIE_FRAC of the queries -- the checks of
tests/test_gpu_parity.py, imported from there."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests.conftest import GOLDEN, oracle_knn
from tests.test_gpu_parity import COS_RTOL, MAX_TIE_FRAC, _certify, _ref_semantics, _t, cos_close

pytestmark = pytest.mark.gpu

DIMS = (256, 384, 512, 768, 1536, 2048)
GRID = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden_dims():
    g = dict(np.load(os.path.join(GOLDEN, "search_dims.npz")))
    g.update(np.load(os.path.join(GOLDEN, "search_dims_int8_1536.npz")))
    return g


# ----------------------------------------------------------------------------- Phase I
def _hamming_gpu(codes, q, k, dev, row_offset=0):
    from vectorragquantization_amd import _native as N
    lib = N.load()
    codes_t, q_t = _t(codes, dev), _t(q, dev)
    n, cb = codes.shape
    nq = q.shape[0]
    D = torch.empty((nq, k), dtype=torch.int32, device=dev)
    R = torch.empty((nq, k), dtype=torch.int64, device=dev)
    need = lib.vrq_hamming_topk_workspace_size(n, cb, nq, k)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    N.check(lib.vrq_hamming_topk(N.ptr(codes_t), n, cb, row_offset, N.ptr(q_t), nq, k, N.ptr(D), N.ptr(R),
                                 N.ptr(ws), ws.numel(), N.stream_handle(dev)), "hamming_topk")
    torch.cuda.synchronize()
    return D.cpu().numpy(), R.cpu().numpy()


# a single ragged tile; chunk boundary + 1; many chunks with an odd tail; the largest candidate
# capacity; an odd query count
@pytest.mark.parametrize("n,nq,k", [(1, 1, 1), (37, 3, 100), (4097, 5, 100), (50_001, 16, 100), (20_000, 2, 1024),
                                    (20_000, 33, 500)])
@pytest.mark.parametrize("d", DIMS)
def test_hamming_topk_vs_faiss_restatement(dev, oracle_lib, d, n, nq, k):
    rng = np.random.default_rng(d + n + nq + k)
    codes = rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, d // 8), dtype=np.uint8)
    q[0] = codes[n // 2]                            # exact hit (dist 0)
    D0, I0 = oracle_knn(oracle_lib, codes, q, k)
    D1, I1 = _hamming_gpu(codes, q, k, dev)
    assert np.array_equal(D0, D1)
    assert np.array_equal(I0, I1)


@pytest.mark.parametrize("d", (384, 768, 2048))
def test_hamming_topk_heavy_ties_and_offset(dev, oracle_lib, d):
    rng = np.random.default_rng(11 + d)
    base = rng.integers(0, 256, (25, d // 8), dtype=np.uint8)
    codes = base[rng.integers(0, 25, 120_000)]      # every distance occurs thousands of times
    q = np.concatenate([base[:4], rng.integers(0, 256, (4, d // 8), dtype=np.uint8)])
    for k in (1, 100, 1000):
        D0, I0 = oracle_knn(oracle_lib, codes, q, k)
        D1, I1 = _hamming_gpu(codes, q, k, dev, row_offset=5_000_000)
        assert np.array_equal(D0, D1)
        assert np.array_equal(I0 + 5_000_000, I1)


@pytest.mark.parametrize("d", (384, 768, 2048))
def test_hamming_topk_all_identical_rows(dev, oracle_lib, d):
    codes = np.full((70_000, d // 8), 0x5A, dtype=np.uint8)
    q = np.zeros((3, d // 8), dtype=np.uint8)
    D0, I0 = oracle_knn(oracle_lib, codes, q, 100)
    D1, I1 = _hamming_gpu(codes, q, 100, dev)
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
    assert I1[0].tolist() == list(range(100))


def _far_corpus(d, rng, n=9000):
    """Near copies of a base code (<= 6 flipped bits) and the complement of the base as the query: every
    distance is >= d - 6 >= 1028; row 4321 is the base itself, at distance d exactly."""
    base = rng.integers(0, 256, d // 8, dtype=np.uint8)
    bits = np.tile(np.unpackbits(base), (n, 1))
    for r in range(n):
        f = rng.integers(0, d, rng.integers(1, 7))
        bits[r, f] ^= 1
    codes = np.packbits(bits, axis=1)
    codes[4321] = base
    q = np.stack([~base, ~codes[17], ~codes[8000]])
    return codes, q


@pytest.mark.parametrize("d", (1536, 2048))
def test_distances_above_1027(dev, oracle_lib, d):
    """The merge's histogram must cover every distance of the code size (the 1024-bit instance has 1028
    bins and drops larger distances): through vrq_hamming_topk and through vrq_search3_dim."""
    rng = np.random.default_rng(d)
    codes, q = _far_corpus(d, rng)
    for k in (10, 300):
        D0, I0 = oracle_knn(oracle_lib, codes, q, k)
        assert D0.min() >= 1028 and D0[0, -1] <= d
        D1, I1 = _hamming_gpu(codes, q, k, dev)
        assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
    # a top-K that reaches the row at distance d exactly: the full ranking of 400 rows, the base row last
    D0, I0 = oracle_knn(oracle_lib, codes[4000:4400], q, 400)
    D1, I1 = _hamming_gpu(codes[4000:4400], q, 400, dev)
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
    assert D1[0, -1] == d and I1[0, -1] == 321
    x8 = rng.integers(-127, 128, (codes.shape[0], d), dtype=np.int8)
    qf = _grid(rng.standard_normal((3, d)) / np.sqrt(d))
    cnt, rows, dist, s2, s3 = _search3(codes, x8, qf, q, 10, 10, 3, dev)
    ref = O.three_phase_batch(codes, x8, np.arange(codes.shape[0]), qf, q, 10, 10, 3,
                              phase1=oracle_knn(oracle_lib, codes, q, 100))
    for j in range(3):
        assert int(cnt[j]) == 10 and dist[j].min() >= 1028
        assert _certify(qf[j], q[j], codes, x8, rows[j], dist[j], s2[j], s3[j], ref[j]["row"])


# ----------------------------------------------------------------------------- 3-phase
def _grid(x):
    """float32 values on the 2^-24 grid: every partial sum of +-q_i is exact in float64 in any order."""
    return (np.round(np.asarray(x, np.float64) / GRID) * GRID).astype(np.float32)


def _search3(codes, x8, qf, qb, k, osb, osi, dev, flags=0, row_offset=0, remap=None):
    from vectorragquantization_amd.enhanced import search3
    from vectorragquantization_amd.quant import int8_row_norms
    x8_t = _t(x8, dev)
    norms = int8_row_norms(x8_t) if codes.shape[0] else torch.empty((0,), dtype=torch.float64, device=dev)
    K = min(k * osb, codes.shape[0])
    out = search3(_t(codes, dev), x8_t, norms, _t(qf.astype(np.float32), dev), _t(qb, dev), k, K, k * osi,
                  flags, row_offset, None if remap is None else _t(remap, dev))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check_against_table(cnt, rows, dist, s2, s3, ids, g, tag, codes, x8, qf, qb):
    """tests/test_gpu_parity.py's ``_check_against_table`` -- identical ids, Hamming distances and Phase-II
    scores, or a certified Phase-III tie permutation on at most MAX_TIE_FRAC of the queries -- with the
    table's cosine compared by ``cos_close`` instead of a bare 1e-5 relative bound: the 20-document table
    returns near-orthogonal rows whose scores (~3e-4) sit at the float32 summation floor of the reference's
    sdot (measured: 2.9e-9 absolute = 1.07e-5 relative on one of them), which is what ``cos_close`` floors."""
    row_of = {int(e): r for r, e in enumerate(ids.tolist())}  # IDMap2 rev_map: last add wins
    ties = 0
    for q in range(cnt.shape[0]):
        n = int(g[f"{tag}_cnt"][q])
        assert int(cnt[q]) == n
        ref_ids = g[f"{tag}_ids"][q][:n]
        ref_rows = rows[q][:n] if np.array_equal(ids[rows[q][:n]], ref_ids) else \
            np.array([row_of[int(e)] for e in ref_ids], dtype=np.int64)
        same = _certify(qf[q], qb[q], codes, x8, rows[q][:n], dist[q][:n], s2[q][:n], s3[q][:n], ref_rows)
        if same:
            assert np.array_equal(dist[q][:n], g[f"{tag}_ham"][q][:n])
            assert np.array_equal(s2[q][:n], g[f"{tag}_bin"][q][:n])
            for j, r in enumerate(rows[q][:n].tolist()):
                assert cos_close(s3[q][j], g[f"{tag}_cos"][q][j], qf[q], x8[r]), (q, j)
        ties += not same
    assert ties <= MAX_TIE_FRAC * cnt.shape[0], f"{ties} of {cnt.shape[0]} queries differ by Phase-III ties"
    return ties


@pytest.mark.parametrize("tag", ["k10", "k7", "k30"])
@pytest.mark.parametrize("d", (384, 1536))
def test_search3_vs_reference_golden(golden_dims, dev, d, tag):
    g, p = golden_dims, f"d{d}_"
    k, osb, osi = (int(v) for v in g[f"{p}{tag}_params"])
    codes, x8, qf, qb = g[p + "codes"], g[p + "int8"], g[p + "qf"], g[p + "qb"]
    cnt, rows, dist, s2, s3 = _search3(codes, x8, qf, qb, k, osb, osi, dev)
    _check_against_table(cnt, rows, dist, s2, s3, g[p + "ids"], g, p + tag, codes, x8, qf, qb)


def test_search3_vs_reference_golden_small_with_removals(golden_dims, dev):
    g, p = golden_dims, "d384_"
    codes, x8, qf, qb = g[p + "small_codes"], g[p + "small_int8"], g[p + "qf"], g[p + "qb"]
    cnt, rows, dist, s2, s3 = _search3(codes, x8, qf, qb, 10, 10, 3, dev)   # k * os_b > ntotal
    _check_against_table(cnt, rows, dist, s2, s3, g[p + "small_rows_ids"], g, p + "small", codes, x8, qf, qb)


def _synthetic(d, rng, n=20_000, nq=48, zero_row=4242):
    C = rng.standard_normal((64, d)) / np.sqrt(d)
    F = C[rng.integers(0, 64, n)] + (0.6 / np.sqrt(d)) * rng.standard_normal((n, d))
    F = (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)
    F[17] = F[3]                                          # duplicate rows -> ties in every phase
    codes, x8, _ = O.encode_batch("cohere", F, 3.0 / np.sqrt(d))
    x8[zero_row] = 0                                      # zero norm -> -inf cosine
    qf = F[rng.integers(0, n, nq)] + (0.3 / np.sqrt(d)) * rng.standard_normal((nq, d))
    qf[1] = F[zero_row]
    qf = _grid(qf / np.linalg.norm(qf, axis=1, keepdims=True))
    qb, _, _ = O.encode_batch("cohere", qf, 0.1)
    return codes, x8, qf, qb


@pytest.mark.parametrize("d", (256, 512, 768, 2048))
def test_search3_vs_oracle_synthetic(dev, d):
    codes, x8, qf, qb = _synthetic(d, np.random.default_rng(21 + d))
    n, nq = codes.shape[0], qf.shape[0]
    ref = O.three_phase_batch(codes, x8, np.arange(n, dtype=np.int64), qf, qb, 10, 10, 3)
    cnt, rows, dist, s2, s3 = _search3(codes, x8, qf, qb, 10, 10, 3, dev)
    c1, r1, d1, _, _ = _search3(codes, x8, qf, qb, 10, 10, 3, dev, flags=1)       # VRQ_SEARCH_PHASE1_ONLY
    cv = _search3(codes, x8, qf, qb, 10, 10, 3, dev, flags=4)                     # VRQ_SEARCH_SCAN_VALU: no-op
    for a, b in zip((cnt, rows, dist, s2, s3), cv):
        assert np.array_equal(a, b, equal_nan=True)
    ties = 0
    for q in range(nq):
        o = ref[q]
        assert int(c1[q]) == 100 and np.array_equal(r1[q], o["p1_rows"]) and np.array_equal(d1[q], o["p1_dist"])
        assert int(cnt[q]) == len(o["row"])
        same = _certify(qf[q], qb[q], codes, x8, rows[q], dist[q], s2[q], s3[q], o["row"])
        if same:
            assert np.array_equal(s2[q], o["binary"])
            np.testing.assert_allclose(s3[q], o["cosine"], rtol=COS_RTOL)
        ties += not same
    assert ties <= MAX_TIE_FRAC * nq
    # the zero-norm row: query 1 is its float vector, so it leads Phases I and II; with K3 = k every Phase-III
    # score is returned and its -inf sorts last
    cz, rz, _, _, sz = _search3(codes, x8, qf[:2], qb[:2], 10, 10, 1, dev)
    assert int(cz[1]) == 10 and rz[1, -1] == 4242 and sz[1, -1] == -np.inf and np.isfinite(sz[1, :-1]).all()


@pytest.mark.parametrize("d", (256, 2048))
def test_search3_edges(dev, d):
    """k * os_b > n, n = 0, and a rescore_row remap with a duplicated id."""
    rng = np.random.default_rng(5 + d)
    codes, x8, qf, qb = _synthetic(d, rng, n=61, nq=5, zero_row=50)
    ids = np.arange(61, dtype=np.int64)
    ref = O.three_phase_batch(codes, x8, ids, qf, qb, 10, 10, 3)                  # K = min(100, 61)
    cnt, rows, dist, s2, s3 = _search3(codes, x8, qf, qb, 10, 10, 3, dev)
    for q in range(5):
        assert int(cnt[q]) == 10
        _certify(qf[q], qb[q], codes, x8, rows[q], dist[q], s2[q], s3[q], ref[q]["row"])
    c1, r1, d1, _, _ = _search3(codes, x8, qf, qb, 10, 10, 3, dev, flags=1)
    assert (c1 == 61).all() and r1.shape == (5, 61) and np.array_equal(r1[0], ref[0]["p1_rows"])
    # n = 0
    e = _search3(codes[:0], x8[:0], qf, qb, 10, 10, 3, dev)
    assert (e[0] == 0).all()
    # remap: rows 7 and 30 carry one id, whose last add is row 30 -> Phases II/III of a hit on row 7 use row 30
    remap = np.arange(61, dtype=np.int64)
    remap[7] = 30
    qf2, qb2 = qf.copy(), qb.copy()
    qb2[0] = codes[7]
    qf2[0] = _grid(x8[30] / np.linalg.norm(x8[30]))                  # cosine 1 with row 30's int8 vector
    cnt, rows, dist, s2, s3 = _search3(codes, x8, qf2, qb2, 10, 10, 3, dev, remap=remap)
    assert 7 in rows[0].tolist()
    for q in range(5):
        for j, r in enumerate(rows[q].tolist()):
            ham = _ref_semantics(qf2[q], qb2[q], codes, x8, [r])[0][0]
            _, r2, r3 = _ref_semantics(qf2[q], qb2[q], codes, x8, [int(remap[r])])
            assert dist[q, j] == ham and s2[q, j] == r2[0] and cos_close(s3[q, j], r3[0], qf2[q], x8[remap[r]])


# ----------------------------------------------------------------------------- rescoring, 1024 forwarders
def _rescore(lib, suffix, dim, qf_t, codes_t, x8_t, norms, cand_t, n, dev):
    from vectorragquantization_amd import _native as N
    nq, nc = cand_t.shape
    o2 = torch.empty((nq, nc), dtype=torch.float64, device=dev)
    o3 = torch.empty((nq, nc), dtype=torch.float64, device=dev)
    N.check(getattr(lib, "vrq_rescore_binary" + suffix)(N.ptr(qf_t), nq, dim, N.ptr(codes_t), n, N.ptr(cand_t), nc,
                                                        N.ptr(o2), N.stream_handle(dev)), "rb")
    N.check(getattr(lib, "vrq_rescore_int8_cosine" + suffix)(N.ptr(qf_t), nq, dim, N.ptr(x8_t), N.ptr(norms), n,
                                                             N.ptr(cand_t), nc, N.ptr(o3), N.stream_handle(dev)), "rc")
    torch.cuda.synchronize()
    return o2.cpu().numpy(), o3.cpu().numpy()


@pytest.mark.parametrize("d", (384, 2048, 1024))
def test_rescore_dim_entry_points(dev, d):
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd.quant import int8_row_norms
    rng = np.random.default_rng(8 + d)
    n = 500
    F = rng.standard_normal((n, d)).astype(np.float32) * 0.03
    codes, x8, _ = O.encode_batch("cohere", F, 0.1)
    x8[9] = 0
    qf = _grid(rng.standard_normal((3, d)) * 0.03)
    cand = rng.integers(-1, n, (3, 20)).astype(np.int64)
    cand[0, 0] = 9
    x8_t, qf_t, codes_t, cand_t = _t(x8, dev), _t(qf, dev), _t(codes, dev), _t(cand, dev)
    norms = int8_row_norms(x8_t)
    lib = N.load()
    o2, o3 = _rescore(lib, "_dim", d, qf_t, codes_t, x8_t, norms, cand_t, n, dev)
    if d == 1024:  # the forwarders: bit-identical to the ABI-1 functions
        b2, b3 = _rescore(lib, "", d, qf_t, codes_t, x8_t, norms, cand_t, n, dev)
        assert np.array_equal(o2, b2, equal_nan=True) and np.array_equal(o3, b3, equal_nan=True)
    for q in range(3):
        for j in range(20):
            r = cand[q, j]
            if r < 0:
                assert np.isnan(o2[q, j]) and np.isnan(o3[q, j])
                continue
            _, r2, r3 = _ref_semantics(qf[q], codes[0], codes, x8, [r])
            assert o2[q, j] == r2[0]
            assert cos_close(o3[q, j], r3[0], qf[q], x8[r])
    assert o3[0, 0] == -np.inf


def test_search3_dim_at_1024_equals_search3(dev):
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd.quant import int8_row_norms
    rng = np.random.default_rng(3)
    n, nq, k, K, K3 = 5000, 8, 10, 100, 30
    F = rng.standard_normal((n, 1024)).astype(np.float32) * 0.03
    codes, x8, _ = O.encode_batch("cohere", F, 0.1)
    qf = (F[:nq] + 0.01 * rng.standard_normal((nq, 1024))).astype(np.float32)
    qb, _, _ = O.encode_batch("cohere", qf, 0.1)
    codes_t, x8_t, qf_t, qb_t = _t(codes, dev), _t(x8, dev), _t(qf, dev), _t(qb, dev)
    norms = int8_row_norms(x8_t)
    lib = N.load()
    need = lib.vrq_search3_dim_workspace_size(n, 1024, nq, K)
    assert need == lib.vrq_search3_workspace_size(n, 1024, nq, K)
    for flags in (0, N.VRQ_SEARCH_PHASE1_ONLY, N.VRQ_SEARCH_SHARD):
        kout = k if flags == 0 else K
        res = []
        for fn in (lib.vrq_search3, lib.vrq_search3_dim):
            cnt = torch.zeros((nq,), dtype=torch.int32, device=dev)
            rows = torch.zeros((nq, kout), dtype=torch.int64, device=dev)
            dist = torch.zeros((nq, kout), dtype=torch.int32, device=dev)
            s2 = torch.zeros((nq, kout), dtype=torch.float64, device=dev)
            s3 = torch.zeros((nq, kout), dtype=torch.float64, device=dev)
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)
            N.check(fn(N.ptr(codes_t), N.ptr(x8_t), N.ptr(norms), 0, n, 1024, 0, N.ptr(qf_t), N.ptr(qb_t), nq, k, K, K3,
                       flags, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), N.ptr(ws), need,
                       N.stream_handle(dev)), "search3")
            torch.cuda.synchronize()
            res.append([t.cpu().numpy() for t in (cnt, rows, dist, s2, s3)])
        for a, b in zip(*res):
            assert np.array_equal(a, b, equal_nan=True)


def test_sharded_search_stays_1024_only(dev):
    """dist.ShardedSearch's per-shard call (VRQ_SEARCH_SHARD) is refused at the other dims."""
    from vectorragquantization_amd import _native as N
    codes, x8, qf, qb = _synthetic(384, np.random.default_rng(1), n=100, nq=2, zero_row=50)
    with pytest.raises(N.VrqNativeError, match="unsupported"):
        _search3(codes, x8, qf, qb, 10, 10, 3, dev, flags=N.VRQ_SEARCH_SHARD)


# ----------------------------------------------------------------------------- classes
def test_enhanced_db_384(tmp_path, dev):
    from vectorragquantization_amd.embed import SyntheticCohereProvider
    from vectorragquantization_amd.enhanced import CohereEnhancedVectorDB
    d = 384
    rng = np.random.default_rng(44)
    codes, x8, qf, qb = _synthetic(d, rng, n=700, nq=6, zero_row=333)
    ids = np.arange(700, dtype=np.int64) * 2 + 100
    prov = SyntheticCohereProvider(dim=d, device=dev)
    db = CohereEnhancedVectorDB(str(tmp_path / "db"), embedding_dim=d, provider=prov, device=dev)
    db.add_vectors(ids[:400], x8[:400], codes[:400])
    db.add_vectors(ids[400:], x8[400:], codes[400:])
    db.remove_document(int(ids[10]), save=False)
    db.add_vectors(ids[10:11], x8[10:11], codes[10:11])             # re-add: now the last row
    assert len(db) == 700
    order = np.r_[0:10, 11:700, 10]
    c, x, e = codes[order], x8[order], ids[order]
    ref = O.three_phase_batch(c, x, e, qf, qb, 10, 10, 3)

    def check(database):
        res = database.search_vectors(qf, qb, 10, 10, 3)
        torch.cuda.synchronize()
        rows, got_ids = res.row.cpu().numpy(), res.doc_id.cpu().numpy()
        for q in range(6):
            assert int(res.count[q]) == 10
            _certify(qf[q], qb[q], c, x, rows[q], res.hamming[q].cpu().numpy(), res.binary[q].cpu().numpy(),
                     res.cosine[q].cpu().numpy(), ref[q]["row"])
            assert np.array_equal(got_ids[q], e[rows[q]])
        return got_ids
    a = check(db)
    db.save()
    db2 = CohereEnhancedVectorDB(str(tmp_path / "db"), embedding_dim=d, provider=prov, device=dev)
    assert len(db2) == 700 and np.array_equal(check(db2), a)


@pytest.mark.parametrize("cls,mode,d", [("VectorDBInt8Global", "int8g", 768), ("VectorDBInt4", "int4", 384),
                                        ("VectorDBInt8", "int8", 1536), ("VectorDBInt16Global", "int16g", 2048),
                                        ("VectorDBInt4Global", "int4g", 2048)])
def test_vectordb_classes_other_dims(tmp_path, dev, cls, mode, d):
    from vectorragquantization_amd import vectordb
    from vectorragquantization_amd.embed import TableProvider
    rng = np.random.default_rng(d)
    n = 1500
    C = rng.standard_normal((32, d)) / np.sqrt(d)
    F = (C[rng.integers(0, 32, n)] + (0.5 / np.sqrt(d)) * rng.standard_normal((n, d))).astype(np.float32)
    Q = (F[rng.integers(0, n, 12)] + (0.1 / np.sqrt(d)) * rng.standard_normal((12, d))).astype(np.float32)
    db = getattr(vectordb, cls)(str(tmp_path / "db"), embedding_dim=d, provider=TableProvider({}), device=dev)
    db.add_vectors(list(range(n)), F)
    ref = O.QuantVectorDB(mode, db.limit if db.limit is not None else 0.0, d)
    ref.add(list(range(n)), F)
    # the codes the class stored on the device are the oracle's (ref.index.xb is O.encode_batch(mode, F,
    # limit)[0], added once in this order): otherwise a wrong code moves both sides' candidates only by luck
    assert np.array_equal(db.index.codes.cpu().numpy(), ref.index.xb)
    for cf in (False, True):
        ids, _, ham, sc = db.search_vectors(Q, 10, 10, cf)
        torch.cuda.synchronize()
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        for j in range(12):
            exp = ref.search(Q[j], 10, 10, cf)
            assert ids[j].tolist() == [e for e, _ in exp]
            assert np.allclose(sc[j], [s for _, s in exp], rtol=1e-5, atol=0)


def test_binary_index_1536(tmp_path, dev):
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    rng = np.random.default_rng(9)
    codes = rng.integers(0, 256, (3000, 192), dtype=np.uint8)
    ids = rng.permutation(10_000)[:3000].astype(np.int64)
    a, b = BinaryIndexIDMap2(1536, dev), O.IndexBinaryIDMap2(1536)
    for s in range(0, 3000, 700):
        a.add_with_ids(codes[s:s + 700], ids[s:s + 700])
        b.add_with_ids(codes[s:s + 700], ids[s:s + 700])
    q = np.concatenate([codes[[5, 17, 2999]], ~codes[[5]]])      # the complement: distances around 1536 - 768
    for k in (1, 10, 100):
        Da, La = a.search(q, k)
        Db, Lb = b.search(q, k)
        assert np.array_equal(Da, Db) and np.array_equal(La, Lb)
    a.write(str(tmp_path / "index.bin"))
    c = BinaryIndexIDMap2.read(str(tmp_path / "index.bin"), dev)
    assert c.d == 1536 and np.array_equal(c.codes.cpu().numpy(), codes)
    assert np.array_equal(c.id_map.cpu().numpy(), ids)
    Dc, Lc = c.search(q, 10)
    Db, Lb = b.search(q, 10)
    assert np.array_equal(Dc, Db) and np.array_equal(Lc, Lb)
