"""The sharded search at every embedding dim and for the two-phase classes, in one process: three uneven
shards of one corpus searched by ``vrq_shard_search3`` / ``vrq_shard_search2`` and merged on the device by
``vrq_merge_shards`` / ``vrq_merge_shards2`` must equal the single-index call over the whole corpus
(``vrq_search3_dim`` / ``vrq_search2``) bit for bit: both sides score a row with the same device functions and
the merge reproduces the single index's order.  One configuration per family is also checked against the CPU
oracle, so the GPU does not only agree with itself.

Corpus (per dim): 70 000 rows in shards [0, 66 000) (>= 65 536 rows: the matrix-core scan K1rd where the
shape allows, the wavefront scan when forced), [66 000, 66 050) (fewer rows than K: count < K and padding) and
[66 050, 70 000); rows 66 000-66 049 duplicate rows 0-49 ((dist, row) and score ties across shards); one zero
int8 row (s3 = -inf); query 0 is all zero (every score ties).  nq = 40; K = 100 is the small LDS instance of
the finish and merge kernels, K = 1000 the general one."""
import numpy as np
import pytest
import torch

import binary_oracle as B
from oracle import oracle_np as O
from tests.conftest import oracle_knn
from tests.test_gpu_dims import _far_corpus, _grid
from tests.test_gpu_parity import MAX_TIE_FRAC, _certify, _t

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
DIMS = (256, 384, 1536, 2048)       # the shortest code, the two dims with reference goldens, the longest code
N_ROWS, NQ = 70_000, 40
SHARDS = ((0, 66_000), (66_000, 66_050), (66_050, 70_000))
ZERO_ROW = 67_000
VALU, MFMA = 4, 8                   # VRQ_SEARCH_SCAN_VALU / VRQ_SEARCH_SCAN_MFMA
# (k, flags): K = 10 k.  The matrix-core scan needs K <= 128, so K = 1000 runs the wavefront scan only.
SIZES = [(10, 0), (10, VALU), (10, MFMA), (100, 0), (100, VALU)]
MODES = ("sbin", "int8g", "int4", "f32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


class Corpus:
    def __init__(self, dev, d):
        from vectorragquantization_amd.quant import encode, int8_row_norms
        g = torch.Generator(device=dev).manual_seed(1000 + d)
        rs = d ** -0.5
        C = torch.randn((64, d), generator=g, device=dev) * rs
        F = C[torch.randint(0, 64, (N_ROWS,), generator=g, device=dev)]
        F = F + 0.6 * rs * torch.randn((N_ROWS, d), generator=g, device=dev)
        F = F / F.norm(dim=1, keepdim=True)
        F[66_000:66_050] = F[0:50]
        self.F = F.contiguous()
        self.limit = 3.0 * rs
        e = encode("cohere", self.F, self.limit, dev)
        self.codes, self.x8 = e["codes"], e["q"]
        self.x8[ZERO_ROW] = 0
        self.norms = int8_row_norms(self.x8)
        e4 = encode("int4", self.F, device=dev)
        self.q4, self.mm = e4["q"], e4["minmax"]
        qf = F[torch.randint(0, N_ROWS, (NQ,), generator=g, device=dev)]
        qf = qf + 0.3 * rs * torch.randn((NQ, d), generator=g, device=dev)
        qf[1:6] = F[0:5] + 0.01 * rs * torch.randn((5, d), generator=g, device=dev)   # near the duplicated rows
        qf[6] = F[ZERO_ROW] + 0.01 * rs * torch.randn((d,), generator=g, device=dev)  # near the zero int8 row
        qf = qf / qf.norm(dim=1, keepdim=True)
        qf = (torch.round(qf.double() * 2.0 ** 24) / 2.0 ** 24).float()               # exact f64 partial sums
        qf[0] = 0.0
        self.qf = qf.contiguous()
        self.qb = encode("cohere", self.qf, 0.1, dev)["codes"]
        self.d, self.dev = d, dev
        self.ref3, self.ref2, self.sh3, self.sh2 = {}, {}, {}, {}

    def stored(self, mode):
        """(q, minmax, limit) of a two-phase rescoring mode; Phase I runs over the same codes for all of them."""
        return {"sbin": (self.codes, None, 0.0), "int8g": (self.x8, None, self.limit),
                "int4": (self.q4, self.mm, 0.0), "f32": (self.F, None, 0.0)}[mode]

    # the single-index results (the comparison side), one call per configuration
    def single3(self, k):
        from vectorragquantization_amd.enhanced import search3
        if k not in self.ref3:
            out = search3(self.codes, self.x8, self.norms, self.qf, self.qb, k, 10 * k, 3 * k)
            torch.cuda.synchronize()
            self.ref3[k] = [t.cpu().numpy() for t in out]
        return self.ref3[k]

    def single2(self, mode, k):
        from vectorragquantization_amd.quant import search2
        if (mode, k) not in self.ref2:
            q, mm, lim = self.stored(mode)
            out = search2(mode, self.codes, q, self.qf, self.qb, k, 10, mm, lim)
            torch.cuda.synchronize()
            self.ref2[(mode, k)] = [t.cpu().numpy() for t in out]
        return self.ref2[(mode, k)]

    # the per-shard calls, stacked [S, nq(, K)]
    def shards3(self, K, flags):
        from vectorragquantization_amd.dist import shard_search3
        if (K, flags) not in self.sh3:
            self.sh3.clear()
            per = [shard_search3(self.codes[a:b], self.x8[a:b], self.norms[a:b], self.qf, self.qb, K, flags, a)
                   for a, b in SHARDS]
            self.sh3[(K, flags)] = [torch.stack(t) for t in zip(*per)]
        return self.sh3[(K, flags)]

    def shards2(self, mode, K, flags):
        from vectorragquantization_amd.dist import shard_search2
        if (mode, K, flags) not in self.sh2:
            self.sh2.clear()
            q, mm, lim = self.stored(mode)
            per = [shard_search2(mode, self.codes[a:b], q[a:b], self.qf, self.qb, K, None if mm is None else mm[a:b],
                                 lim, flags, a) for a, b in SHARDS]
            self.sh2[(mode, K, flags)] = [torch.stack(t) for t in zip(*per)]
        return self.sh2[(mode, K, flags)]


_CORPORA = {}


def _corpus(dev, d):
    if d not in _CORPORA:
        _CORPORA[d] = Corpus(dev, d)
    return _CORPORA[d]


def _scan_kinds(d, K):
    """The scan each forcing flag selects on the large shard (the other two always take the wavefront scan)."""
    from vectorragquantization_amd import _native as N
    lib = N.load()
    n0 = SHARDS[0][1]
    assert lib.vrq_scan_kind(n0, d, NQ, K, VALU, None) == N.VRQ_SCAN_KIND_VALU
    for flags in (0, MFMA):
        assert lib.vrq_scan_kind(n0, d, NQ, K, flags, None) == \
            (N.VRQ_SCAN_KIND_MFMA if K <= 128 else N.VRQ_SCAN_KIND_VALU)
    assert lib.vrq_scan_kind(SHARDS[2][1] - SHARDS[2][0], d, NQ, K, MFMA, None) == N.VRQ_SCAN_KIND_VALU


# ----------------------------------------------------------------------------- merged == single index
@pytest.mark.timeout(120)
@pytest.mark.parametrize("k,flags", SIZES)
@pytest.mark.parametrize("d", DIMS)
def test_three_phase_shards_merged_equal_single_index(dev, d, k, flags):
    from vectorragquantization_amd.dist import merge_shards
    c = _corpus(dev, d)
    K = 10 * k
    _scan_kinds(d, K)
    cnt, rows, dist, s2, s3 = c.shards3(K, flags)
    got = merge_shards(cnt, rows, dist, s2, s3, k, 3 * k)
    torch.cuda.synchronize()
    want = c.single3(k)
    assert np.all(want[0] == k)
    for name, a, b in zip(("count", "rows", "dist", "s2", "s3"), got, want):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), name
    src = got[5].cpu().numpy()                                     # s*K + p of each result in the stacked inputs
    flat = rows.permute(1, 0, 2).reshape(NQ, -1).cpu().numpy()
    assert np.array_equal(np.take_along_axis(flat, src.astype(np.int64), 1), want[1])
    if k == 10:  # the planted cases are in the results
        assert any(r in want[1][q] and r + 66_000 in want[1][q] for q in range(1, 6) for r in range(5))
        assert np.all(want[3][0] == 0.0) and np.all((want[4][0] == 0.0) | (want[4][0] == -np.inf))  # the zero query


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,flags", SIZES)
@pytest.mark.parametrize("d", DIMS)
def test_two_phase_shards_merged_equal_single_index(dev, d, k, flags, mode):
    from vectorragquantization_amd.quant import merge_shards2
    c = _corpus(dev, d)
    K = 10 * k
    cnt, rows, dist, sc = c.shards2(mode, K, flags)
    oc, orow, od, osc, src = (t.cpu().numpy() for t in merge_shards2(cnt, rows, dist, sc, k))
    want = c.single2(mode, k)
    assert np.all(oc == k) and oc.dtype == np.int32
    for name, a, b in zip(("rows", "dist", "score"), (orow, od, osc), want):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), name
    flat = rows.permute(1, 0, 2).reshape(NQ, -1).cpu().numpy()
    assert np.array_equal(np.take_along_axis(flat, src.astype(np.int64), 1), want[0])
    assert np.all(np.diff(osc, axis=1) <= 0)
    # the zero query: every score ties, so the result is in Phase-I (dist, row) order
    assert np.all(osc[0] == 0.0) and np.all(np.diff((od[0].astype(np.int64) << 40) | orow[0]) > 0)


# ----------------------------------------------------------------------------- the per-shard outputs themselves
@pytest.mark.timeout(120)
@pytest.mark.parametrize("d", DIMS)
def test_per_shard_outputs(dev, d):
    """Shard 1 (50 rows < K): count, padding, (dist, row) order and the global rows; shard 0: the sharded scores
    are the single index's; the three scans give identical outputs."""
    c = _corpus(dev, d)
    K = 100
    a, b = SHARDS[1]
    three = [t.cpu().numpy() for t in c.shards3(K, 0)]
    two = [t.cpu().numpy() for t in c.shards2("sbin", K, 0)]
    for cnt, rows, dist, *scores in (three, two):
        assert np.all(cnt[1] == b - a) and np.all(cnt[0] == K) and np.all(cnt[2] == K)
        assert np.all(rows[1][:, b - a:] == -1) and np.all(dist[1][:, b - a:] == INT32_MAX)
        for s in scores:
            assert np.all(np.isnan(s[1][:, b - a:])) and not np.isnan(s[1][:, :b - a]).any()
            assert not np.isnan(s[0]).any() and not np.isnan(s[2]).any()
        for s, (lo, hi) in enumerate(SHARDS):
            m = int(cnt[s][0])
            r, dd = rows[s][:, :m], dist[s][:, :m].astype(np.int64)
            assert r.min() >= lo and r.max() < hi
            key = (dd << 40) | r
            assert np.all(np.diff(key, axis=1) > 0)                # ascending (dist, row), no row twice
    assert np.array_equal(three[1], two[1]) and np.array_equal(three[2], two[2])      # the same Phase I
    pos = np.nonzero(three[1][2][6] == ZERO_ROW)[0]                # query 6 sits on the zero int8 row (shard 2)
    assert pos.size == 1 and three[4][2][6][pos[0]] == -np.inf and np.isfinite(three[3][2][6][pos[0]])
    assert np.isfinite(np.delete(three[4][2][6], pos[0])).all()
    # the candidates of the large shard carry the scores the single index gives the same rows
    want = c.single3(10)
    for q in range(NQ):
        at = {int(r): j for j, r in enumerate(three[1][0][q])}
        for j, r in enumerate(want[1][q].tolist()):
            if r in at:
                assert three[3][0][q][at[r]] == want[3][q][j] and three[4][0][q][at[r]] == want[4][q][j]
    for flags in (VALU, MFMA):
        for x, y in zip(three, [t.cpu().numpy() for t in c.shards3(K, flags)]):
            assert np.array_equal(x, y, equal_nan=True)
        for x, y in zip(two, [t.cpu().numpy() for t in c.shards2("sbin", K, flags)]):
            assert np.array_equal(x, y, equal_nan=True)


# ----------------------------------------------------------------------------- against the CPU oracle
@pytest.mark.timeout(120)
def test_three_phase_merged_vs_oracle(dev, oracle_lib):
    from vectorragquantization_amd.dist import merge_shards
    d, k = 384, 10
    c = _corpus(dev, d)
    cnt, rows, dist, s2, s3 = c.shards3(10 * k, MFMA)
    got = [t.cpu().numpy() for t in merge_shards(cnt, rows, dist, s2, s3, k, 3 * k)]
    codes, x8, qf, qb = (t.cpu().numpy() for t in (c.codes, c.x8, c.qf, c.qb))
    ref = O.three_phase_batch(codes, x8, np.arange(N_ROWS, dtype=np.int64), qf, qb, k, 10, 3,
                              phase1=oracle_knn(oracle_lib, codes, qb, 10 * k))
    ties = 0
    for q in range(NQ):
        assert int(got[0][q]) == k
        same = _certify(qf[q], qb[q], codes, x8, got[1][q], got[2][q], got[3][q], got[4][q], ref[q]["row"])
        if same:
            assert np.array_equal(got[3][q], ref[q]["binary"])
        ties += not same
    assert ties <= MAX_TIE_FRAC * NQ
    assert np.array_equal(got[1][0], ref[0]["row"])                # the zero query: the first k of Phase I
    assert np.array_equal(got[1][0], ref[0]["p1_rows"][:k])


@pytest.mark.timeout(120)
def test_two_phase_merged_vs_oracle(dev, oracle_lib):
    """mode sbin: the score is the exact dot of the query with the +-1 row, rounded once to float32."""
    from vectorragquantization_amd.quant import merge_shards2
    d, k = 384, 10
    c = _corpus(dev, d)
    cnt, rows, dist, sc = c.shards2("sbin", 10 * k, MFMA)
    oc, orow, od, osc, _ = (t.cpu().numpy() for t in merge_shards2(cnt, rows, dist, sc, k))
    codes, qf, qb = (t.cpu().numpy() for t in (c.codes, c.qf, c.qb))
    D, I = oracle_knn(oracle_lib, codes, qb, 10 * k)
    for q in range(NQ):
        signed = B.signed_rows(codes[I[q]], d)
        cand = [(int(I[q, j]), int(D[q, j]), B.exact_dot(qf[q], signed[j])) for j in range(10 * k)]
        top = sorted(cand, key=lambda t: -t[2])[:k]                # CohereVectorDBBinary.py:236: stable, descending
        assert int(oc[q]) == k
        assert orow[q].tolist() == [t[0] for t in top]
        assert od[q].tolist() == [t[1] for t in top]
        assert osc[q].tolist() == [t[2] for t in top]


# ----------------------------------------------------------------------------- distances past 1027, dim 1024
@pytest.mark.timeout(120)
@pytest.mark.parametrize("d", (1536, 2048))
def test_merges_cover_distances_above_1027(dev, d):
    """The merges take no dim: their histogram must hold every distance of the longest code (a 1024-bit
    instance drops candidates at distance >= 1028)."""
    from vectorragquantization_amd.dist import merge_shards, shard_search2, shard_search3
    from vectorragquantization_amd.enhanced import search3
    from vectorragquantization_amd.quant import int8_row_norms, merge_shards2, search2
    rng = np.random.default_rng(d)
    codes, qb = _far_corpus(d, rng)
    n = codes.shape[0]
    x8 = _t(rng.integers(-127, 128, (n, d), dtype=np.int8), dev)
    qf = _t(_grid(rng.standard_normal((3, d)) / np.sqrt(d)), dev)
    codes, qb, norms = _t(codes, dev), _t(qb, dev), int8_row_norms(x8)
    k, K = 10, 100
    cuts = ((0, 4500), (4500, n))
    per = [shard_search3(codes[a:b], x8[a:b], norms[a:b], qf, qb, K, 0, a) for a, b in cuts]
    got = merge_shards(*(torch.stack(t) for t in zip(*per)), k, 3 * k)
    want = search3(codes, x8, norms, qf, qb, k, K, 3 * k)
    assert int(want[2].min()) >= 1028 and bool((want[0] == k).all())
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    per = [shard_search2("sbin", codes[a:b], codes[a:b], qf, qb, K, None, 0.0, 0, a) for a, b in cuts]
    oc, orow, od, osc, _ = merge_shards2(*(torch.stack(t) for t in zip(*per)), k)
    want = search2("sbin", codes, codes, qf, qb, k, 10)
    assert bool((oc == k).all())
    for a, b in zip((orow, od, osc), want):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


@pytest.mark.timeout(120)
def test_shard_search3_at_1024_forwards(dev):
    """vrq_shard_search3 at dim 1024 is vrq_search3 with VRQ_SEARCH_SHARD, bit for bit."""
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd.dist import shard_search3
    from vectorragquantization_amd.enhanced import search3
    from vectorragquantization_amd.quant import encode, int8_row_norms
    g = torch.Generator(device=dev).manual_seed(7)
    n, nq, K = 30_000, 9, 100
    F = torch.randn((n, 1024), generator=g, device=dev) * 0.03
    e = encode("cohere", F, 0.1, dev)
    codes, x8 = e["codes"], e["q"]
    norms = int8_row_norms(x8)
    qf = (F[:nq] + 0.01 * torch.randn((nq, 1024), generator=g, device=dev)).contiguous()
    qb = encode("cohere", qf, 0.1, dev)["codes"]
    want = search3(codes, x8, norms, qf, qb, 10, K, 30, N.VRQ_SEARCH_SHARD, 5_000_000)
    got = shard_search3(codes, x8, norms, qf, qb, K, 0, 5_000_000)
    torch.cuda.synchronize()
    assert bool((got[0] == K).all()) and int(got[1].min()) >= 5_000_000
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
