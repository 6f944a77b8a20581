"""Every Phase-II / Phase-III / flat-IP score the library returns, against exact rational arithmetic
(tests/exact_score_model.py), on queries OFF the grid on which every float64 summation order agrees.

Each entry point runs on a corpus small enough that every row is a candidate and every score comes back (the
fused calls with k = K3 = K = n), per dim of GPU_DIMS and query family (a)-(f) of the model:
  * Phase II, and flat IP before its rounding: bit-equal to ``exact_dot`` under ``order_free``; otherwise
    |got - exact| <= ``sum_bound`` (derived, not tuned).
  * Phase III and flat IP: a member of ``phase3_values`` -- bit-exact wherever that set has one element (at least
    99 % of the pairs, a condition on the fixtures that tests/test_exact_score_model.py checks); the float32
    half-ulp ties of family (e) to even, family (f) +-0 / norm, the zero row -inf.
  * Order: rebuilt from the call's own output -- Phase I by (dist, row), the stable descending sort by s2, the
    stable descending sort by s3 (-0.0 ties +0.0, -inf last) -- and equal to the returned order exactly, whatever
    the last bits of s2 are off the grid.
  * Cross-path identity: asserted where ``order_free`` holds, recorded per family elsewhere (the wave order of
    vrq_rescore_* / vrq_search3_large and the nibble order of vrq_search3* differ in the last bits of s2 there).
These kernels include vrq_rescore_binary_dim / vrq_rescore_int8_cosine_dim, the reference of
test_gpu_large_k.py, test_gpu_shard_large_k.py and test_gpu_filtered.py.

The int8 and float32 corpora are zero at the four dims where family (d) carries +-2^60 (a product with 2^60 would
push ``sum_bound`` past the float32 spacing: the reference itself would be ambiguous); Phase II takes the pairs in
full.  Families (b)-(d) hold no NaN or Inf; queries with NaN or Inf are out of scope here.  The library's smallest dim is
256 (the model also covers 128).  The figures of DESIGN.md section 3 are this module's report (printed at the end
of the module; written as JSON to the file VRQ_EXACT_SCORES_REPORT names, if set)."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests import exact_score_model as M
from vectorragquantization_amd import _native as N

pytestmark = pytest.mark.gpu

GPU_DIMS = (256, 384, 768, 1024, 1536, 2048)
N_ROWS = 300            # K in (256, 1024]: Phase II's second 256-candidate pass, the bitonic stable_desc_order
N_SMALL = 100           # K <= 128: the small LDS instance
N_FLAT = 24             # float32 rows: the 12 integer-valued ones + 12 standard-normal
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
REPORT, IDENT, NOTES = {}, {}, []
_CASES, _OUT = {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    N.load()
    yield torch.device("cuda", 0)
    _emit_report()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ----------------------------------------------------------------------------- fixtures and their exact facts
class Case:
    """One dim: the queries of every family, a corpus of N_ROWS (codes, int8) rows and N_FLAT float32 rows on
    the device, and per (query, row) the exact dot, the bound (0 under order_free) and the Phase-III set."""

    def __init__(self, dim, dev):
        self.dim, self.dev = dim, dev
        self.Q, self.fam, _ = M.all_queries(dim)
        self.nq = self.Q.shape[0]
        self.codes = M.code_rows(dim, N_ROWS - M.N_SPECIAL)
        self.x8 = M.int8_rows(dim, N_ROWS - M.N_SPECIAL)
        self.xf = M.float_rows(dim, N_FLAT - 12)
        assert self.codes.shape[0] == self.x8.shape[0] == N_ROWS and self.xf.shape[0] == N_FLAT
        rng = np.random.default_rng(dim)
        self.qb = rng.integers(0, 256, (self.nq, dim // 8), dtype=np.uint8)
        self.qb[0], self.qb[1] = self.codes[40], self.codes[0]          # distance 0; heavy ties of the constant codes
        self.ham = POP[self.codes[None, :, :] ^ self.qb[:, None, :]].sum(2)
        self.free2 = [M.order_free(q, 1) for q in self.Q]
        self.free3 = [M.order_free(q, 128) for q in self.Q]
        g = M.gamma(dim - 1)
        self.ex2 = [M.exact_dots(q, self.codes) for q in self.Q]
        self.bd2 = [[0 if f else g * a for a in M.exact_dots(q, self.codes, absolute=True)]
                    for q, f in zip(self.Q, self.free2)]
        self.ex3 = [M.exact_dots(q, self.x8) for q in self.Q]
        self.bd3 = [[0 if f else g * a for a in M.exact_dots(q, self.x8, absolute=True)]
                    for q, f in zip(self.Q, self.free3)]
        # device side; the norms come from the library and equal the oracle's
        from vectorragquantization_amd.quant import int8_row_norms
        self.codes_t, self.x8_t, self.xf_t = _t(self.codes, dev), _t(self.x8, dev), _t(self.xf, dev)
        self.Q_t, self.qb_t = _t(self.Q, dev), _t(self.qb, dev)
        self.norms_t = int8_row_norms(self.x8_t)
        torch.cuda.synchronize()
        self.norms = self.norms_t.cpu().numpy()
        assert np.array_equal(self.norms, O.int8_row_norms(self.x8))
        assert self.norms.tolist() == [M.int8_norm(x) for x in self.x8] and self.norms[M.ZERO_ROW] == 0.0
        self.v3 = [[M.phase3_values(None, None, float(self.norms[r]), exact=self.ex3[i][r], bound=self.bd3[i][r])
                    for r in range(N_ROWS)] for i in range(self.nq)]
        # flat IP: the first 12 rows are integer-valued (order_free(q, 128) applies), the rest float32 proper
        xi = self.xf[:12].astype(np.int8)
        assert np.array_equal(xi.astype(np.float32), self.xf[:12])
        self.exf, self.bdf = [], []
        for q, f in zip(self.Q, self.free3):
            ex = M.exact_dots(q, xi) + [M.exact_dot(q, x) for x in self.xf[12:]]
            ab = M.exact_dots(q, xi, absolute=True) + [M.abs_dot(q, x) for x in self.xf[12:]]
            self.exf.append(ex)
            self.bdf.append([0 if (f and r < 12) else g * a for r, a in enumerate(ab)])
        self.vf = [[M.phase3_values(None, None, None, exact=self.exf[i][r], bound=self.bdf[i][r])
                    for r in range(N_FLAT)] for i in range(self.nq)]
        for sets in (self.v3, self.vf):                  # the fixtures' condition, on this corpus too
            flat = [v for row in sets for v in row]
            assert all(v is not None for v in flat) and sum(len(v) == 2 for v in flat) <= 0.01 * len(flat)


def _case(dim, dev):
    if dim not in _CASES:
        _CASES[dim] = Case(dim, dev)
    return _CASES[dim]


# ----------------------------------------------------------------------------- the assertions
def _stat(entry, fam):
    return REPORT.setdefault((entry, fam), {"pairs3": 0, "unique3": 0, "pairs2": 0, "max_ratio": 0.0})


def check_sums(entry, c, got, rows, exact, bound, free):
    """Phase II (or any float64 sum before a rounding): got[i][j] is the sum of query i and row rows[i][j]."""
    for i in range(c.nq):
        st = _stat(entry, c.fam[i])
        for j, r in enumerate(rows[i]):
            g, ex, bd = float(got[i][j]), exact[i][r], bound[i][r]
            assert np.isfinite(g), (entry, c.dim, c.fam[i], i, r)
            err = abs(Fraction(g) - ex)
            if free[i]:
                assert err == 0, (entry, c.dim, c.fam[i], i, r, g, float(ex))
            else:
                assert err <= bd, (entry, c.dim, c.fam[i], i, r, g, float(ex), float(err / bd))
                st["max_ratio"] = max(st["max_ratio"], float(err / bd))
            st["pairs2"] += 1


def check_rounded(entry, c, got, rows, values):
    """Phase III / flat IP: got[i][j] must be one of values[i][rows[i][j]]."""
    for i in range(c.nq):
        st = _stat(entry, c.fam[i])
        for j, r in enumerate(rows[i]):
            vals = values[i][r]
            assert float(got[i][j]) in vals, (entry, c.dim, c.fam[i], i, r, float(got[i][j]), vals)
            st["pairs3"] += 1
            st["unique3"] += len(vals) == 1


def check_special_rows(c, s3_by_row):
    """Family (e): the float32 ties to even; family (f): +-0 / norm; the zero row: -inf.  s3_by_row[i][r]."""
    e0, f0 = c.fam.index("e"), c.fam.index("f")
    for qi, r, want in M.TIE_EXPECT:
        assert s3_by_row[e0 + qi][r] == np.float64(np.float32(want)) / c.norms[r], (c.dim, qi, r)
    assert s3_by_row[f0][2] == 0.0
    assert all(s3_by_row[i][M.ZERO_ROW] == -np.inf for i in range(c.nq))


def desc_stable(keys):
    """Positions in stable descending order: -0.0 ties +0.0, -inf last (Python's sorted(reverse=True) on a key)."""
    return np.argsort(-(np.asarray(keys, np.float64) + 0.0), kind="stable")


def check_three_phase_order(c, n, rows, dist, s2, s3):
    """The returned order of a k = K3 = K = n search, rebuilt from the call's own output."""
    for i in range(c.nq):
        r = rows[i].astype(np.int64)
        assert sorted(r.tolist()) == list(range(n)), (c.dim, i)
        assert np.array_equal(dist[i], c.ham[i, r])
        by2, by3 = np.empty(n), np.empty(n)
        by2[r], by3[r] = s2[i], s3[i]
        p1 = np.lexsort((np.arange(n), c.ham[i, :n]))                     # Phase I: (dist, row)
        p2 = p1[desc_stable(by2[p1])]                                    # stable by s2 desc
        p3 = p2[desc_stable(by3[p2])]                                    # stable by s3 desc
        assert np.array_equal(r, p3), (c.dim, c.fam[i], i)


def by_row(n, rows, sc):
    out = np.full((len(rows), n), np.nan)
    for i in range(len(rows)):
        out[i, rows[i].astype(np.int64)] = sc[i]
    return out


# ----------------------------------------------------------------------------- the calls
def _rescore(c, suffix, n):
    """(s2, s3) f64[nq, n + 3] of every row, a negative candidate and two >= n, through vrq_rescore_*<suffix>."""
    key = (c.dim, "rescore" + suffix, n)
    if key not in _OUT:
        lib = N.load()
        cand = np.tile(np.r_[np.arange(n), -1, n, n + 12345].astype(np.int64), (c.nq, 1))
        cand_t = _t(cand, c.dev)
        o2 = torch.zeros(cand.shape, dtype=torch.float64, device=c.dev)
        o3 = torch.zeros(cand.shape, dtype=torch.float64, device=c.dev)
        st = N.stream_handle(c.dev)
        N.check(getattr(lib, "vrq_rescore_binary" + suffix)(N.ptr(c.Q_t), c.nq, c.dim, N.ptr(c.codes_t), n,
                                                            N.ptr(cand_t), cand.shape[1], N.ptr(o2), st), "binary")
        N.check(getattr(lib, "vrq_rescore_int8_cosine" + suffix)(N.ptr(c.Q_t), c.nq, c.dim, N.ptr(c.x8_t),
                                                                 N.ptr(c.norms_t), n, N.ptr(cand_t), cand.shape[1],
                                                                 N.ptr(o3), st), "cosine")
        torch.cuda.synchronize()
        _OUT[key] = (o2.cpu().numpy(), o3.cpu().numpy())
    return _OUT[key]


def _search3(c, name, n, K, flags=0):
    """(cnt, rows, dist, s2, s3) of ``name`` over the first n rows with k = K3 = K."""
    key = (c.dim, name, n, K, flags)
    if key not in _OUT:
        lib = N.load()
        shard = name == "vrq_shard_search3"
        size = {"vrq_search3": "vrq_search3_workspace_size", "vrq_search3_dim": "vrq_search3_dim_workspace_size",
                "vrq_search3_large": "vrq_search3_large_workspace_size",
                "vrq_shard_search3": "vrq_shard_search3_workspace_size"}[name]
        need = getattr(lib, size)(n, c.dim, c.nq, K)
        assert need > 0
        ws = torch.empty((need,), dtype=torch.uint8, device=c.dev)
        cnt = torch.full((c.nq,), -7, dtype=torch.int32, device=c.dev)
        rows = torch.full((c.nq, K), -7, dtype=torch.int64, device=c.dev)
        dist = torch.full((c.nq, K), -7, dtype=torch.int32, device=c.dev)
        s2 = torch.zeros((c.nq, K), dtype=torch.float64, device=c.dev)
        s3 = torch.zeros((c.nq, K), dtype=torch.float64, device=c.dev)
        head = (N.ptr(c.codes_t), N.ptr(c.x8_t), N.ptr(c.norms_t), 0, n, c.dim, 0, N.ptr(c.Q_t), N.ptr(c.qb_t), c.nq)
        tail = (N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), N.ptr(ws), need, N.stream_handle(c.dev))
        mid = (K, flags) if shard else (K, K, K, flags)
        N.check(getattr(lib, name)(*head, *mid, *tail), name)
        torch.cuda.synchronize()
        _OUT[key] = [t.cpu().numpy() for t in (cnt, rows, dist, s2, s3)]
    return _OUT[key]


def _check_search3(entry, c, n, out, phase1_order=False):
    cnt, rows, dist, s2, s3 = out
    assert (cnt == n).all()
    assert (rows[:, n:] == -1).all() and np.isnan(s2[:, n:]).all() and np.isnan(s3[:, n:]).all()
    rows, dist, s2, s3 = rows[:, :n], dist[:, :n], s2[:, :n], s3[:, :n]
    check_sums(entry + " s2", c, s2, rows, c.ex2, c.bd2, c.free2)
    check_rounded(entry + " s3", c, s3, rows, c.v3)
    check_special_rows(c, by_row(n, rows, s3))
    if phase1_order:
        for i in range(c.nq):
            assert np.array_equal(rows[i], np.lexsort((np.arange(n), c.ham[i, :n])))
            assert np.array_equal(dist[i], c.ham[i, rows[i]])
    else:
        check_three_phase_order(c, n, rows, dist, s2, s3)
    return by_row(n, rows, s2), by_row(n, rows, s3)


# ----------------------------------------------------------------------------- stand-alone rescoring
@pytest.mark.parametrize("dim", GPU_DIMS)
def test_rescore_entry_points(dev, dim):
    c = _case(dim, dev)
    for suffix in ("_dim", "") if dim == 1024 else ("_dim",):
        s2, s3 = _rescore(c, suffix, N_ROWS)
        assert np.isnan(s2[:, N_ROWS:]).all() and np.isnan(s3[:, N_ROWS:]).all()      # negative and >= n: NaN
        rows = np.tile(np.arange(N_ROWS), (c.nq, 1))
        check_sums(f"vrq_rescore_binary{suffix}", c, s2[:, :N_ROWS], rows, c.ex2, c.bd2, c.free2)
        check_rounded(f"vrq_rescore_int8_cosine{suffix}", c, s3[:, :N_ROWS], rows, c.v3)
        check_special_rows(c, s3)
    # a shorter corpus: a candidate past ITS end is NaN although the row exists in memory
    t2, t3 = _rescore(c, "_dim", N_SMALL)
    assert np.isnan(t2[:, N_SMALL:]).all() and np.isnan(t3[:, N_SMALL:]).all()
    assert np.array_equal(t2[:, :N_SMALL], s2[:, :N_SMALL]) and np.array_equal(t3[:, :N_SMALL], s3[:, :N_SMALL])


# ----------------------------------------------------------------------------- the fused search
def _routes(c, n, K):
    """The Phase-I routes the plan admits for the shape: (label, flags of tests/test_gpu_phase1_routes.py)."""
    lib = N.load()
    out = [("default", 0), ("wavefront", N.VRQ_SEARCH_SCAN_VALU)]
    if c.dim == 1024 and lib.vrq_scan_kind(n, c.dim, c.nq, K, N.VRQ_SEARCH_SCAN_MFMA, None) == N.VRQ_SCAN_KIND_MFMA:
        out.append(("matrix", N.VRQ_SEARCH_SCAN_MFMA))      # (the whole call takes this flag at 1024 only)
    return out


@pytest.mark.parametrize("n", (N_SMALL, N_ROWS), ids=("small_instance", "big_instance"))
@pytest.mark.parametrize("dim", GPU_DIMS)
def test_search3_every_row(dev, dim, n):
    c = _case(dim, dev)
    name = "vrq_search3" if dim == 1024 else "vrq_search3_dim"
    first = None
    for label, flags in _routes(c, n, n):
        got = _check_search3(f"{name} K={n}", c, n, _search3(c, name, n, n, flags))
        if first is None:
            first = got
        assert np.array_equal(first[0], got[0]) and np.array_equal(first[1], got[1]), label   # one finish, any scan
    NOTES.append(f"{name} dim {dim} n {n}: routes {[r for r, _ in _routes(c, n, n)]}")


def test_search3_matrix_route_1024(dev):
    """The matrix-core scan's sorted list feeds the 1024 finish by another branch, and exists from 65 536 rows:
    K = k = K3 = 100 (the route takes K <= 128) of 65 543 rows, so every CANDIDATE comes back; its scores and the
    order of the 100 are checked as above, and both routes must return the same bits."""
    c = _case(1024, dev)
    lib = N.load()
    n, K = 65_543, N_SMALL
    rng = np.random.default_rng(4)
    codes = np.concatenate([c.codes, rng.integers(0, 256, (n - N_ROWS, 128), dtype=np.uint8)])
    x8 = np.concatenate([c.x8, rng.integers(-128, 128, (n - N_ROWS, 1024)).astype(np.int8)])
    x8[:, list(M.big_positions(1024))] = 0
    codes_t, x8_t = _t(codes, dev), _t(x8, dev)
    from vectorragquantization_amd.quant import int8_row_norms
    norms_t = int8_row_norms(x8_t)
    norms = norms_t.cpu().numpy()
    res = {}
    for label, flags in (("wavefront", N.VRQ_SEARCH_SCAN_VALU), ("matrix", N.VRQ_SEARCH_SCAN_MFMA)):
        kind = N.VRQ_SCAN_KIND_MFMA if label == "matrix" else N.VRQ_SCAN_KIND_VALU
        assert lib.vrq_scan_kind(n, 1024, c.nq, K, flags, None) == kind
        need = lib.vrq_search3_workspace_size(n, 1024, c.nq, K)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        cnt = torch.zeros((c.nq,), dtype=torch.int32, device=dev)
        rows = torch.zeros((c.nq, K), dtype=torch.int64, device=dev)
        dist = torch.zeros((c.nq, K), dtype=torch.int32, device=dev)
        s2 = torch.zeros((c.nq, K), dtype=torch.float64, device=dev)
        s3 = torch.zeros((c.nq, K), dtype=torch.float64, device=dev)
        N.check(lib.vrq_search3(N.ptr(codes_t), N.ptr(x8_t), N.ptr(norms_t), 0, n, 1024, 0, N.ptr(c.Q_t), N.ptr(c.qb_t),
                                c.nq, K, K, K, flags, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3),
                                N.ptr(ws), need, N.stream_handle(dev)), "vrq_search3")
        torch.cuda.synchronize()
        res[label] = [t.cpu().numpy() for t in (cnt, rows, dist, s2, s3)]
    for a, b in zip(res["wavefront"], res["matrix"]):
        assert np.array_equal(a, b)
    cnt, rows, dist, s2, s3 = res["matrix"]
    assert (cnt == K).all()
    g = M.gamma(1023)
    for i, q in enumerate(c.Q):
        r = rows[i]
        ham = POP[codes ^ c.qb[i]].sum(1)
        p1 = np.lexsort((np.arange(n), ham))[:K]                          # the K candidates, (dist, row)
        assert sorted(r.tolist()) == sorted(p1.tolist()) and np.array_equal(dist[i], ham[r])
        ex2, ab2 = M.exact_dots(q, codes[r]), M.exact_dots(q, codes[r], absolute=True)
        ex3, ab3 = M.exact_dots(q, x8[r]), M.exact_dots(q, x8[r], absolute=True)
        st = _stat("vrq_search3 matrix route", c.fam[i])
        pos = {int(v): j for j, v in enumerate(r)}
        for j in range(K):
            err = abs(Fraction(float(s2[i, j])) - ex2[j])
            bd = 0 if c.free2[i] else g * ab2[j]
            assert err <= bd, (c.fam[i], i, j)
            if bd:
                st["max_ratio"] = max(st["max_ratio"], float(err / bd))
            vals = M.phase3_values(None, None, float(norms[r[j]]), exact=ex3[j], bound=0 if c.free3[i] else g * ab3[j])
            assert float(s3[i, j]) in vals, (c.fam[i], i, j)
            st["pairs2"] += 1
            st["pairs3"] += 1
            st["unique3"] += len(vals) == 1
        p2 = p1[desc_stable([s2[i, pos[int(v)]] for v in p1])]
        p3 = p2[desc_stable([s3[i, pos[int(v)]] for v in p2])]
        assert np.array_equal(r, p3), (c.fam[i], i)


@pytest.mark.parametrize("n", (N_SMALL, N_ROWS), ids=("small_instance", "big_instance"))
@pytest.mark.parametrize("dim", GPU_DIMS)
def test_shard_form(dev, dim, n):
    """vrq_shard_search3 (at 1024: vrq_search3 with VRQ_SEARCH_SHARD): all K candidates in Phase-I order with both
    scores -- Phase III in the shard loop of the finish, not in finish_query."""
    c = _case(dim, dev)
    s2, s3 = _check_search3(f"vrq_shard_search3 K={n}", c, n, _search3(c, "vrq_shard_search3", n, n), phase1_order=True)
    if dim == 1024:
        flagged = _search3(c, "vrq_search3", n, n, N.VRQ_SEARCH_SHARD)
        for a, b in zip(flagged, _search3(c, "vrq_shard_search3", n, n)):
            assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("dim", GPU_DIMS)
def test_search3_large(dev, dim):
    """K = 1025 over 300 rows: the counting scan and the large finish (one wave per score, the stand-alone
    rescoring's scorers) with every row a candidate."""
    c = _case(dim, dev)
    _check_search3("vrq_search3_large K=1025", c, N_ROWS, _search3(c, "vrq_search3_large", N_ROWS, 1025))


# ----------------------------------------------------------------------------- the exhaustive paths
def _gemm(c, mode, flags=0):
    key = (c.dim, "gemm", mode, flags)
    if key not in _OUT:
        from vectorragquantization_amd.enhanced import gemm_topk
        served = "exact scan K5d"
        if c.dim == 1024 and not flags & N.VRQ_GEMM_SCAN_EXACT:
            try:        # which internal path serves the queries: the call reports an unserved query on request
                gemm_topk(mode, c.Q_t, N_ROWS, codes=c.codes_t, x8=c.x8_t, norms=c.norms_t,
                          flags=flags | N.VRQ_GEMM_NO_FALLBACK)
                served = "matrix pass + finish"
            except N.VrqNativeError:
                served = "exact fallback for some queries"
        cnt, rows, sc = gemm_topk(mode, c.Q_t, N_ROWS, codes=c.codes_t, x8=c.x8_t, norms=c.norms_t, flags=flags)
        torch.cuda.synchronize()
        _OUT[key] = (cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy(), served)
    return _OUT[key]


def _check_topk_order(c, n, rows, sc):
    for i in range(c.nq):
        r = rows[i].astype(np.int64)
        assert sorted(r.tolist()) == list(range(n)), (c.dim, i)
        by = np.empty(n)
        by[r] = sc[i]
        assert np.array_equal(r, desc_stable(by)), (c.dim, c.fam[i], i)    # (score desc, row asc)


@pytest.mark.parametrize("mode", ("binary", "int8_cosine"))
@pytest.mark.parametrize("dim", GPU_DIMS)
def test_gemm_topk_every_row(dev, dim, mode):
    """k = n = 300: vrq_gemm_topk at 1024 (the matrix pass with its finish or its exact fallback, whichever the
    call takes: noted in the report) and vrq_gemm_topk_dim's exact scan K5d at every dim, 1024 included."""
    c = _case(dim, dev)
    for flags in (0, N.VRQ_GEMM_SCAN_EXACT) if dim == 1024 else (0,):
        cnt, rows, sc, served = _gemm(c, mode, flags)
        entry = ("vrq_gemm_topk" if dim == 1024 and not flags else "vrq_gemm_topk_dim") + " " + mode
        NOTES.append(f"{entry} dim {dim}: served by {served}")
        assert (cnt == N_ROWS).all()
        if mode == "binary":
            check_sums(entry, c, sc, rows, c.ex2, c.bd2, c.free2)
        else:
            check_rounded(entry, c, sc, rows, c.v3)
            check_special_rows(c, by_row(N_ROWS, rows, sc))
        _check_topk_order(c, N_ROWS, rows, sc)


def _flat(c, flags=0):
    key = (c.dim, "flat", flags)
    if key not in _OUT:
        from vectorragquantization_amd.flat import flat_ip_prepare, flat_ip_topk
        x8 = inv = bounds = None
        served = "exact scan K5d"
        if c.dim == 1024 and not flags:
            bounds = torch.zeros((2,), dtype=torch.float64, device=c.dev)
            x8, inv = flat_ip_prepare(c.xf_t, bounds)
            try:
                flat_ip_topk(c.xf_t, x8, inv, bounds, c.Q_t, N_FLAT, flags=N.VRQ_GEMM_NO_FALLBACK)
                served = "matrix pass + finish"
            except N.VrqNativeError:
                served = "exact fallback for some queries"
        cnt, rows, sc = flat_ip_topk(c.xf_t, x8, inv, bounds, c.Q_t, N_FLAT, flags=flags)
        torch.cuda.synchronize()
        _OUT[key] = (cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy(), served)
    return _OUT[key]


@pytest.mark.parametrize("dim", GPU_DIMS)
def test_flat_ip_every_row(dev, dim):
    """vrq_flat_ip_topk (1024) and vrq_flat_ip_topk_dim with k = n: the exact float32 x float32 dot rounded once."""
    c = _case(dim, dev)
    for flags in (0, N.VRQ_GEMM_SCAN_EXACT) if dim == 1024 else (0,):
        cnt, rows, sc, served = _flat(c, flags)
        entry = "vrq_flat_ip_topk" if dim == 1024 and not flags else "vrq_flat_ip_topk_dim"
        NOTES.append(f"{entry} dim {dim}: served by {served}")
        assert (cnt == N_FLAT).all()
        check_rounded(entry, c, sc, rows, c.vf)
        assert (sc == sc.astype(np.float32).astype(np.float64)).all()       # float32 values
        by = by_row(N_FLAT, rows, sc)
        e0, f0 = c.fam.index("e"), c.fam.index("f")
        for qi, r, want in M.TIE_EXPECT:                                     # (rows 0-2 are the tie rows as floats)
            assert by[e0 + qi][r] == want
        assert by[f0][2] == 0.0
        _check_topk_order(c, N_FLAT, rows, sc)


# ----------------------------------------------------------------------------- cross-path identity
# (statement, where it is made, Phase, path A, path B).  A path: a function of the case -> scores by row [nq, 300].
def _p_rescore(suffix, which):
    return lambda c: _rescore(c, suffix, N_ROWS)[which][:, :N_ROWS]


def _p_search(name, K, which, flags=0):
    def f(c):
        cnt, rows, dist, s2, s3 = _search3(c, name, N_ROWS, K, flags)
        return by_row(N_ROWS, rows[:, :N_ROWS], (s2, s3)[which][:, :N_ROWS])
    return f


def _p_gemm(mode, flags=0):
    def f(c):
        cnt, rows, sc, _ = _gemm(c, mode, flags)
        return by_row(N_ROWS, rows, sc)
    return f


def _identities(dim):
    s3name = "vrq_search3" if dim == 1024 else "vrq_search3_dim"
    out = []
    for which, ph in ((0, "II"), (1, "III")):
        mode = ("binary", "int8_cosine")[which]
        out += [
            (f"shard form = fused search, Phase {ph} (vrq.h, DESIGN 5)", which,
             _p_search("vrq_shard_search3", N_ROWS, which), _p_search(s3name, N_ROWS, which)),
            (f"large finish = stand-alone rescoring, Phase {ph} (vrq.h, select_rescore.hip)", which,
             _p_search("vrq_search3_large", 1025, which), _p_rescore("_dim", which)),
            (f"large finish = fused search, Phase {ph} (INTEGRATION, select_rescore.hip)", which,
             _p_search("vrq_search3_large", 1025, which), _p_search(s3name, N_ROWS, which)),
            (f"exhaustive scan K5d = stand-alone rescoring, Phase {ph} (exhaustive_dim.hip)", which,
             _p_gemm(mode, N.VRQ_GEMM_SCAN_EXACT if dim == 1024 else 0), _p_rescore("_dim", which)),
        ]
        if dim == 1024:
            out += [
                (f"_dim forwarders = ABI-1 calls, Phase {ph} (vrq.h)", which,
                 _p_rescore("_dim", which), _p_rescore("", which)),
                (f"_dim forwarders = ABI-1 calls, Phase {ph} (vrq.h)", which,
                 _p_search("vrq_search3_dim", N_ROWS, which), _p_search("vrq_search3", N_ROWS, which)),
                (f"vrq_gemm_topk = fused search, Phase {ph} (vrq.h, exact_scores.h)", which,
                 _p_gemm(mode), _p_search("vrq_search3", N_ROWS, which)),
            ]
    return out


@pytest.mark.parametrize("dim", GPU_DIMS)
def test_cross_path_identity(dev, dim):
    """Every pair of paths a document or a source comment calls bit-identical: identical wherever ``order_free``
    holds (asserted); off the grid the outcome is recorded per family for the report, not asserted -- there the
    statement holds only between paths that share a summation order, within ``sum_bound`` otherwise."""
    c = _case(dim, dev)
    for name, which, pa, pb in _identities(dim):
        a, b = pa(c), pb(c)
        free = (c.free2, c.free3)[which]
        for i in range(c.nq):
            same = np.array_equal(a[i], b[i])
            if free[i]:
                assert same, (name, dim, c.fam[i], i)
            else:
                h = IDENT.setdefault((name, c.fam[i]), [0, 0])
                h[0] += int((a[i] == b[i]).sum())
                h[1] += a.shape[1]


# ----------------------------------------------------------------------------- the report
def _emit_report():
    lines = ["entry point | family | Phase-III pairs | unique value | sums | max |got - exact| / sum_bound"]
    for (entry, fam), st in sorted(REPORT.items()):
        u = f"{st['unique3']}/{st['pairs3']}" if st["pairs3"] else "-"
        lines.append(f"{entry} | {fam} | {st['pairs3']} | {u} | {st['pairs2']} | {st['max_ratio']:.3g}")
    lines.append("identity | family | pairs with equal bits off the grid")
    for (name, fam), (held, total) in sorted(IDENT.items()):
        lines.append(f"{name} | {fam} | {held}/{total}")
    lines += sorted(set(NOTES))
    print("\n" + "\n".join(lines))
    path = os.environ.get("VRQ_EXACT_SCORES_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"scores": [{"entry": e, "family": fm, **st} for (e, fm), st in sorted(REPORT.items())],
                       "identities": [{"identity": nm, "family": fm, "equal": h, "pairs": t}
                                      for (nm, fm), (h, t) in sorted(IDENT.items())],
                       "notes": sorted(set(NOTES))}, f, indent=1)
