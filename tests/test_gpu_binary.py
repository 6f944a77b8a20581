"""GPU parity of the signed-binary path: the ``VRQ_ENC_SIGNED_BINARY`` encoder and the
``VRQ_RESCORE_SIGNED_BINARY`` rescoring against the reference's golden tables and exact arithmetic, the
fused two-phase search ``vrq_search2`` bit for bit against the composed path it replaces
(``vrq_hamming_topk`` -> ``rescore_row`` gather -> ``vrq_rescore_dequant`` -> stable sort -> first k) on every
scan that can feed it, and the ``CohereVectorDBBinary`` class against the tables the reference class itself
produced (tests/golden/make_golden_binary.py)."""
import logging
import math

import numpy as np
import pytest
import torch

import binary_oracle as B
from oracle import oracle_np as O
from tests.test_vectordb_golden import check_table

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
F32, SBIN, INT4L, INT8G = 16, 17, 4, 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def G():
    return B.load_golden()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ----------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("d", B.ENCODER_DIMS)   # 1024: the dedicated kernel; 384: the generic one
def test_sbin_encoder_vs_reference_golden(G, dev, d):
    from vectorragquantization_amd.quant import encode
    X, ref = G[f"x_{d}"], G[f"sbin_{d}"]
    r = encode("sbin", X, device=dev)
    assert r["q"] is None and r["minmax"] is None
    got = r["codes"].cpu().numpy()
    assert np.array_equal(got, ref)
    planted = int(G[f"planted_{d}"])
    gt = encode("int8g", X, 0.3, dev)["codes"].cpu().numpy()      # packbits(x > mean)
    assert all(not np.array_equal(a, b) for a, b in zip(got[-planted:], gt[-planted:]))
    one = encode("sbin", X[3], device=dev)["codes"].cpu().numpy()  # a single 1-D vector
    assert one.shape == (1, d // 8) and np.array_equal(one[0], ref[3])


def test_sbin_encoder_batch_d1024(dev):
    """9001 vectors: more than one launch wave per CU, an odd tail, a flat row (all ones), rows with many
    elements at the mean; bit-exact against NumPy row by row."""
    from vectorragquantization_amd.quant import encode
    rng = np.random.default_rng(78)
    n = 9001
    X = (rng.standard_normal((n, 1024)) * rng.uniform(0.01, 2.0, (n, 1))).astype(np.float32)
    X[17] = 0.25
    X[4000] = np.tile(np.array([0.0, 0.5, 0.0, -0.5], np.float32), 256)
    X[8999] = np.round(X[8999] * 8) / 8
    got = encode("sbin", X, device=dev)["codes"].cpu().numpy()
    assert np.array_equal(got, B.sbin_codes(X))
    assert np.all(got[17] == 255) and np.all(got[4000] == 0b11101110)


# ----------------------------------------------------------------------------- rescoring
def _rescore(lib, N, mode, qf_t, d, q_t, mm_t, limit, n, cand_t, dev):
    out = torch.empty(cand_t.shape, dtype=torch.float64, device=dev)
    N.check(lib.vrq_rescore_dequant(mode, N.ptr(qf_t), qf_t.shape[0], d, N.ptr(q_t), N.ptr(mm_t), limit, n,
                                    N.ptr(cand_t), cand_t.shape[1], N.ptr(out), N.stream_handle(dev)), "rescore")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("d", [256, 1536])
def test_rescore_signed_binary_exact(dev, d):
    from vectorragquantization_amd import _native as N
    rng = np.random.default_rng(d)
    n, nq, nc = 500, 3, 70
    codes = rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
    codes[5], codes[6] = 0, 255
    qf = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(0, n, (nq, nc)).astype(np.int64)
    cand[:, 0], cand[:, 1], cand[:, 2], cand[1, 9] = 5, 6, n - 1, -1
    got = _rescore(N.load(), N, SBIN, _t(qf, dev), d, _t(codes, dev), None, 0.0, n, _t(cand, dev), dev)
    pm = B.signed_rows(codes, d).astype(np.float64)
    for qi in range(nq):
        for j in range(nc):
            if cand[qi, j] < 0:
                assert np.isnan(got[qi, j])
                continue
            want = np.float32(math.fsum((qf[qi].astype(np.float64) * pm[cand[qi, j]]).tolist()))
            assert got[qi, j] == float(want), (qi, j)


@pytest.mark.parametrize("mode,name", [(INT8G, "int8g"), (INT4L, "int4")])
def test_rescore_existing_modes_unchanged(dev, mode, name):
    """The shared dot-product function keeps the existing modes on the oracle's ``dequant_scores``."""
    from vectorragquantization_amd import _native as N
    rng = np.random.default_rng(5)
    n, nq, d, lim = 300, 4, 1024, 0.3
    X = (rng.standard_normal((n, d)) * 0.05).astype(np.float32)
    X[9] = 0.125                                                       # min == max
    _, q, mm = O.encode_batch(name, X, lim)
    qf = rng.standard_normal((nq, d)).astype(np.float32)
    cand = np.tile(np.arange(-1, n, dtype=np.int64), (nq, 1))
    got = _rescore(N.load(), N, mode, _t(qf, dev), d, _t(q, dev), None if mm is None else _t(mm, dev), lim, n,
                   _t(cand, dev), dev)
    assert np.all(np.isnan(got[:, 0]))
    assert np.array_equal(got[:, 1:], O.dequant_scores(qf, O.dequantize(name, q, mm, lim)))


# ----------------------------------------------------------------------------- fused vs composed
class Corpus:
    """Random codes / stored rows for every rescoring mode on the device, with planted Phase-I hits: row
    `hit0` carries query 0's code (distance 0) and min == max, rows `hit1` / `hit2` are one / two bits away."""

    def __init__(self, dev, dim, n, nq, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        cb = dim // 8
        self.dim, self.n, self.nq, self.dev = dim, n, nq, dev
        self.codes = torch.randint(0, 256, (n, cb), dtype=torch.uint8, device=dev, generator=g)
        self.qb = torch.randint(0, 256, (nq, cb), dtype=torch.uint8, device=dev, generator=g)
        self.qf = torch.randn((nq, dim), dtype=torch.float32, device=dev, generator=g)
        self.hit0, self.hit1, self.hit2 = n // 3, n - 1, 1
        self.codes[self.hit0] = self.qb[0]
        self.codes[self.hit1] = self.qb[0]
        self.codes[self.hit1, 0] ^= 1
        self.codes[self.hit2] = self.qb[0]
        self.codes[self.hit2, cb - 1] ^= 0x81
        self.f = torch.randn((n, dim), dtype=torch.float32, device=dev, generator=g)
        self.q4 = torch.randint(-128, 128, (n, dim // 2), dtype=torch.int8, device=dev, generator=g)
        self.mm = torch.rand((n, 2), dtype=torch.float64, device=dev, generator=g) - 0.5
        self.mm[self.hit0] = 0.25

    def stored(self, mode):
        """(q, minmax, limit) of a rescoring mode."""
        if mode == SBIN:
            return self.codes, None, 0.0
        if mode == F32:
            return self.f, None, 0.0
        return self.q4, self.mm, 0.0


def _composed(lib, N, mode, c, k, K, rr=None, row_offset=0):
    """The path ``quant.vectordb_search`` takes, padded to k columns."""
    dev, n, nq, d = c.dev, c.n, c.nq, c.dim
    q, mm, lim = c.stored(mode)
    Kp = min(K, n)
    dist = torch.empty((nq, Kp), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, Kp), dtype=torch.int64, device=dev)
    ws = torch.empty((max(8, lib.vrq_hamming_topk_workspace_size(n, d // 8, nq, Kp)),), dtype=torch.uint8, device=dev)
    N.check(lib.vrq_hamming_topk(N.ptr(c.codes), n, d // 8, 0, N.ptr(c.qb), nq, Kp, N.ptr(dist), N.ptr(rows),
                                 N.ptr(ws), ws.numel(), N.stream_handle(dev)), "vrq_hamming_topk")
    cand = rows if rr is None else torch.where(rows >= 0, rr[rows.clamp_min(0)], rows).contiguous()
    score = torch.empty((nq, Kp), dtype=torch.float64, device=dev)
    N.check(lib.vrq_rescore_dequant(mode, N.ptr(c.qf), nq, d, N.ptr(q), N.ptr(mm), lim, n, N.ptr(cand), Kp,
                                    N.ptr(score), N.stream_handle(dev)), "vrq_rescore_dequant")
    key = torch.where(rows >= 0, score + 0.0, torch.full_like(score, float("-inf")))
    o = torch.sort(-key, dim=1, stable=True).indices[:, :k]
    R = np.full((nq, k), -1, np.int64)
    D = np.full((nq, k), INT32_MAX, np.int32)
    S = np.full((nq, k), np.nan)
    kk = o.shape[1]
    R[:, :kk] = torch.gather(rows, 1, o).cpu().numpy() + row_offset
    D[:, :kk] = torch.gather(dist, 1, o).cpu().numpy()
    S[:, :kk] = torch.gather(score, 1, o).cpu().numpy()
    return np.full(nq, min(k, Kp), np.int32), R, D, S, rows.cpu().numpy()


def _fused(lib, N, mode, c, k, K, flags=0, rr=None, row_offset=0, split=False):
    dev, n, nq, d = c.dev, c.n, c.nq, c.dim
    q, mm, lim = c.stored(mode)
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    R = torch.full((nq, max(k, 1)), -7, dtype=torch.int64, device=dev)
    D = torch.full((nq, max(k, 1)), -7, dtype=torch.int32, device=dev)
    S = torch.full((nq, max(k, 1)), -7.0, dtype=torch.float64, device=dev)
    need = lib.vrq_search2_workspace_size(n, d, nq, K)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    st = N.stream_handle(dev)
    if split:   # the two launches it is made of
        N.check(lib.vrq_search3_dim_scan(N.ptr(c.codes), n, d, N.ptr(c.qb), nq, K, flags, N.ptr(ws), need, st), "scan")
        N.check(lib.vrq_search2_finish(mode, N.ptr(c.codes), N.ptr(q), N.ptr(mm), lim, N.ptr(rr), n, d, row_offset,
                                       N.ptr(c.qf), nq, k, K, flags, N.ptr(cnt), N.ptr(R), N.ptr(D), N.ptr(S),
                                       N.ptr(ws), need, st), "vrq_search2_finish")
    else:
        N.check(lib.vrq_search2(mode, N.ptr(c.codes), N.ptr(q), N.ptr(mm), lim, N.ptr(rr), n, d, row_offset,
                                N.ptr(c.qf), N.ptr(c.qb), nq, k, K, flags, N.ptr(cnt), N.ptr(R), N.ptr(D), N.ptr(S),
                                N.ptr(ws), need, st), "vrq_search2")
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), R[:, :k].cpu().numpy(), D[:, :k].cpu().numpy(), S[:, :k].cpu().numpy()


def _same(got, want):
    for name, a, b in zip(("count", "rows", "dist", "score"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=name == "score"), name


_CORPORA = {}


def _corpus(dev, dim, n, nq):
    key = (dim, n, nq)
    if key not in _CORPORA:
        _CORPORA.clear()          # one corpus resident at a time
        _CORPORA[key] = Corpus(dev, dim, n, nq, seed=dim + nq)
    return _CORPORA[key]


MFMA_FLAG = 8
# (dim, n, nq, K, flags, matrix-core scan expected): the smallest shapes that reach each code path
SHAPES = [(256, 1000, 1, 100, 0, False),          # K1d, two-piece codes
          (1536, 1000, 33, 100, 0, False),        # two-slab codes, more queries than one 32-query block
          (1024, 1000, 5, 100, 0, False),         # the wavefront scan at 1024
          (512, 70_001, 33, 100, MFMA_FLAG, True),   # K1rd: the single suffix list
          (1024, 70_001, 129, 100, 0, True)]      # the default matrix-core scan at 1024


@pytest.mark.parametrize("mode", [SBIN, F32, INT4L])
@pytest.mark.parametrize("dim,n,nq,K,flags,matrix", SHAPES)
def test_search2_equals_composed(dev, dim, n, nq, K, flags, matrix, mode):
    from vectorragquantization_amd import _native as N
    lib = N.load()
    kind = lib.vrq_scan_kind(n, dim, nq, K, flags, None)
    assert kind == (N.VRQ_SCAN_KIND_MFMA if matrix else N.VRQ_SCAN_KIND_VALU)
    c = _corpus(dev, dim, n, nq)
    k = 10
    want = _composed(lib, N, mode, c, k, K)
    assert list(want[4][0, :3]) == [c.hit0, c.hit1, c.hit2]            # the planted min == max row is a candidate
    got = _fused(lib, N, mode, c, k, K, flags)
    _same(got, want[:4])
    assert np.all(got[0] == k) and np.all(np.diff(got[3], axis=1) <= 0)
    _same(_fused(lib, N, mode, c, k, K, flags, split=True), want[:4])


@pytest.mark.parametrize("mode", [SBIN, INT4L])
def test_search2_large_k_instance(dev, mode):
    """K = k = 300: the general LDS instance and the bitonic branch of the stable sort (more than 256 scores)."""
    from vectorragquantization_amd import _native as N
    lib = N.load()
    c = _corpus(dev, 384, 1000, 3)
    _same(_fused(lib, N, mode, c, 300, 300), _composed(lib, N, mode, c, 300, 300)[:4])
    _same(_fused(lib, N, mode, c, 7, 300, N.VRQ_SEARCH_SCAN_VALU), _composed(lib, N, mode, c, 7, 300)[:4])


def test_search2_edges(dev):
    from vectorragquantization_amd import _native as N
    lib = N.load()
    # n = 37 < K: count 37 and padding
    c = Corpus(dev, 256, 37, 2, seed=1)
    got = _fused(lib, N, SBIN, c, 50, 100)
    _same(got, _composed(lib, N, SBIN, c, 50, 100)[:4])
    assert np.all(got[0] == 37) and np.all(got[1][:, 37:] == -1) and np.all(got[2][:, 37:] == INT32_MAX)
    assert np.all(np.isnan(got[3][:, 37:])) and np.all(got[1][:, :37] >= 0)
    # k = 0: only the counts are written
    got = _fused(lib, N, SBIN, c, 0, 100)
    assert np.all(got[0] == 0) and got[1].shape == (2, 0)
    c = _corpus(dev, 256, 1000, 1)
    # row_offset beyond 32 bits
    off = 10**10
    got = _fused(lib, N, F32, c, 10, 100, row_offset=off)
    _same(got, _composed(lib, N, F32, c, 10, 100, row_offset=off)[:4])
    assert got[1].min() >= off
    # a rescore_row that redirects two candidate rows
    rr = torch.arange(c.n, dtype=torch.int64, device=dev)
    rr[c.hit0], rr[c.hit1] = 17, c.hit2
    for mode in (SBIN, F32, INT4L):
        plain = _fused(lib, N, mode, c, 100, 100)
        got = _fused(lib, N, mode, c, 100, 100, rr=rr)
        _same(got, _composed(lib, N, mode, c, 100, 100, rr=rr)[:4])
        assert np.array_equal(np.sort(got[1]), np.sort(plain[1])) and not np.array_equal(got[3], plain[3])
    # both forcing flags give the same answer below the matrix scan's row minimum
    _same(_fused(lib, N, SBIN, c, 10, 100, N.VRQ_SEARCH_SCAN_MFMA), _fused(lib, N, SBIN, c, 10, 100))


@pytest.mark.parametrize("dim", [256, 1024])
def test_search2_exact_ties_keep_phase1_order(dev, dim):
    """A query of equal magnitudes at mode 17: the score is c * (dim - 2 * distance), so all candidates at
    one distance tie exactly and the stable sort must leave them in Phase-I (dist, row) order."""
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd.quant import encode
    lib = N.load()
    c = Corpus(dev, dim, 1000, 2, seed=dim)
    sign = torch.where(torch.rand((2, dim), device=dev) < 0.5, -1.0, 1.0)
    c.qf = (0.375 * sign).to(torch.float32).contiguous()
    c.qb = encode("sbin", c.qf, device=dev)["codes"]
    assert np.array_equal(c.qb.cpu().numpy(), np.packbits(c.qf.cpu().numpy() > 0, axis=1))
    want = _composed(lib, N, SBIN, c, 60, 100)
    got = _fused(lib, N, SBIN, c, 60, 100)
    _same(got, want[:4])
    assert np.array_equal(got[1], want[4][:, :60])                       # = the first k of Phase I
    assert np.array_equal(got[3], 0.375 * (dim - 2.0 * got[2]))
    assert max(np.unique(got[3][0], return_counts=True)[1]) > 1          # ties are present


# ----------------------------------------------------------------------------- the class
def _build(G, d, folder, dev):
    from vectorragquantization_amd import CohereVectorDBBinary
    from vectorragquantization_amd.embed import TableProvider
    F = G[f"d{d}_F"]
    table = {f"t{i}": F[i] for i in range(F.shape[0])}
    db = CohereVectorDBBinary(folder, embedding_dim=d, provider=TableProvider(table), device=dev)
    B.apply_sequence(G, d, lambda i, X, t: db.add_documents(i, t, batch_size=64, save=False),
                     lambda e: db.remove_document(e, save=False))
    return db


def _run(db, Qv, k, osb, cf):
    ids, _, _, sc = db.search_vectors(Qv, k, osb, cf)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


@pytest.mark.parametrize("d", B.SEARCH_DIMS)
def test_class_vs_reference_golden(G, dev, d, tmp_path):
    db = _build(G, d, str(tmp_path / "db"), dev)
    p = f"d{d}_"
    assert db.config == {"version": "1.0", "model": "cohere-embed-english-v3.0", "embedding_dim": d}
    assert len(db) == G[p + "id_map"].shape[0]
    assert np.array_equal(db.index.id_map.cpu().numpy(), G[p + "id_map"])
    assert np.array_equal(db.index.codes.cpu().numpy(), G[p + "codes"])
    ref = B.BinaryOracleDB(d)                                  # tie certification only
    B.apply_sequence(G, d, ref.add, ref.remove)
    Qv = G[p + "QF"]
    for cname, (k, osb) in B.SEARCHES.items():
        for cf in (False, True):
            key = f"{p}{cname}_{'f32' if cf else 'q'}"
            gi, gs = _run(db, Qv, k, osb, cf)
            check_table(gi, gs, G[key + "_ids"], G[key + "_score"], G[key + "_cnt"],
                        lambda q, e: ref.score_of(Qv[q], e, cf))
    # the single-query surface returns the reference's dicts; the identical pair comes out lower row first
    ids = G[p + "ids"]
    for cf in (False, True):
        r = db.search("t7", k=5, compare_float32=cf)
        assert [set(h) for h in r] == [{"doc_id", "score", "doc"}] * 5
        assert (r[0]["doc_id"], r[1]["doc_id"]) == (int(ids[7]), int(ids[200])) and r[0]["score"] == r[1]["score"]
        assert (r[0]["doc"], r[1]["doc"]) == ("t7", "t200") and isinstance(r[0]["score"], float)
    # the id added twice rescoring reads its last vector (t6's), which ties document 6 itself: lower row first
    r = db.search("t6", k=3)
    assert (r[0]["doc_id"], r[1]["doc_id"]) == (int(ids[6]), B.NEW_ID) and r[0]["score"] == r[1]["score"]
    assert r[1]["doc"] == "t6"
    assert db.search("unknown text") == []


def test_class_save_reopen(G, dev, tmp_path, caplog):
    from vectorragquantization_amd import CohereVectorDBBinary
    d = 256
    folder = str(tmp_path / "db")
    db = _build(G, d, folder, dev)
    db.save()
    db2 = CohereVectorDBBinary(folder, embedding_dim=d, provider=db.provider, device=dev)
    assert len(db2) == len(db) and db2.texts == db.texts
    assert np.array_equal(db2.index.id_map.cpu().numpy(), db.index.id_map.cpu().numpy())
    Qv = G[f"d{d}_QF"]
    a, b = _run(db, Qv, 10, 10, False), _run(db2, Qv, 10, 10, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(KeyError):
        db2.search_vectors(Qv[:2], 10, 10, compare_float32=True)
    with pytest.raises(KeyError):
        db2.search("t7", compare_float32=True)
    with caplog.at_level(logging.WARNING):
        db2.remove_document(123456789, save=False)
    assert "not found" in caplog.text and len(db2) == len(db)
    db2.remove_document(int(G[f"d{d}_ids"][7]), save=False)     # a present one goes, float row or not
    assert len(db2) == len(db) - 1
    empty = CohereVectorDBBinary(str(tmp_path / "new"), embedding_dim=d, provider=db.provider, device=dev)
    assert len(empty) == 0 and empty.search("t7") == []
