"""GPU checks of the search with more than 1024 Phase-I candidates (vrq_*_large: the counting scan K1h and
the large finish).  Every comparison is exact.  Reference distances are plain torch ops on the device (xor +
a byte-popcount table) ordered by (dist, row); reference scores are the stand-alone vrq_rescore_*_dim /
vrq_rescore_dequant calls on the Phase-I rows, ordered by NumPy stable sorts -- no kernel under test.  Those
reference kernels (vrq_rescore_binary_dim / vrq_rescore_int8_cosine_dim) are pinned against exact rational
arithmetic by tests/test_gpu_exact_scores.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
POP = np.array([bin(i).count("1") for i in range(256)], np.int16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _N():
    from vectorragquantization_amd import _native as N
    return N, N.load()


def _plan(n, dim, nq, K):
    N, lib = _N()
    info = np.zeros(8, np.int64)
    assert lib.vrq_scan_large_plan(n, dim, nq, K, info.ctypes.data) == N.VRQ_OK
    return [int(x) for x in info]


# ----------------------------------------------------------------------------- references
def ref_phase1(codes_t, q_t, K):
    """(dist i32[nq, K], rows i64[nq, K]) in (dist, row) order, padded INT32_MAX / -1: torch ops only."""
    n = codes_t.shape[0]
    pop = torch.from_numpy(POP).to(codes_t.device)
    D = np.full((q_t.shape[0], K), INT32_MAX, np.int32)
    R = np.full((q_t.shape[0], K), -1, np.int64)
    for i in range(q_t.shape[0]):
        d = pop[(codes_t ^ q_t[i]).long()].sum(1, dtype=torch.int64)
        key = torch.sort(d * (1 << 32) + torch.arange(n, device=d.device)).values[:K].cpu().numpy()
        D[i, :key.shape[0]] = key >> 32
        R[i, :key.shape[0]] = key & 0xffffffff
    return D, R


def _rescore(which, dev, qf_t, dim, rows, n, codes_t=None, x8_t=None, norms_t=None, deq=None):
    """Stand-alone scores f64[nq, ncand] of local rows (negative -> NaN)."""
    N, lib = _N()
    nq, nc = rows.shape
    cand = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    out = torch.empty((nq, nc), dtype=torch.float64, device=dev)
    s = N.stream_handle(dev)
    if which == "binary":
        rc = lib.vrq_rescore_binary_dim(N.ptr(qf_t), nq, dim, N.ptr(codes_t), n, N.ptr(cand), nc, N.ptr(out), s)
    elif which == "cosine":
        rc = lib.vrq_rescore_int8_cosine_dim(N.ptr(qf_t), nq, dim, N.ptr(x8_t), N.ptr(norms_t), n, N.ptr(cand), nc,
                                             N.ptr(out), s)
    else:
        mode, q_t, mm_t, limit = deq
        rc = lib.vrq_rescore_dequant(mode, N.ptr(qf_t), nq, dim, N.ptr(q_t), N.ptr(mm_t), float(limit), n,
                                     N.ptr(cand), nc, N.ptr(out), s)
    N.check(rc, which)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _remap(rows, rr):
    return rows if rr is None else np.where(rows >= 0, rr[np.maximum(rows, 0)], rows)


def _desc_stable(s):
    return np.argsort(-(s + 0.0), kind="stable")  # stable, -0.0 ties +0.0, -inf last


def ref_search3(dev, c, D1, R1, k, K3, row_offset=0):
    """The three-phase result from Phase-I (D1, R1): stable sorts over stand-alone scores."""
    nq, K = R1.shape
    n, dim = c["n"], c["dim"]
    s2 = _rescore("binary", dev, c["qf"], dim, _remap(R1, c["rr"]), n, codes_t=c["codes"])
    cnt = np.zeros(nq, np.int32)
    rows = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), INT32_MAX, np.int32)
    b = np.full((nq, k), np.nan)
    cs = np.full((nq, k), np.nan)
    ord2 = np.zeros((nq, K), np.int64)
    K3p = np.zeros(nq, np.int64)
    cand3 = np.full((nq, max(K3, 1)), -1, np.int64)
    for i in range(nq):
        Kp = int((R1[i] >= 0).sum())
        ord2[i, :Kp] = _desc_stable(s2[i, :Kp])
        K3p[i] = min(K3, Kp)
        cand3[i, :K3p[i]] = R1[i, ord2[i, :K3p[i]]]
    s3 = _rescore("cosine", dev, c["qf"], dim, _remap(cand3, c["rr"]), n, x8_t=c["x8"], norms_t=c["norms"])
    for i in range(nq):
        o3 = _desc_stable(s3[i, :K3p[i]])[:k]
        m = o3.shape[0]
        r = ord2[i, o3]
        cnt[i] = m
        rows[i, :m] = R1[i, r] + row_offset
        dist[i, :m] = D1[i, r]
        b[i, :m] = s2[i, r]
        cs[i, :m] = s3[i, o3]
    return cnt, rows, dist, b, cs


def ref_search2(dev, c, deq, D1, R1, k):
    nq, K = R1.shape
    s = _rescore("dequant", dev, c["qf"], c["dim"], _remap(R1, c["rr"]), c["n"], deq=deq)
    cnt = np.zeros(nq, np.int32)
    rows = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), INT32_MAX, np.int32)
    sc = np.full((nq, k), np.nan)
    for i in range(nq):
        Kp = int((R1[i] >= 0).sum())
        o = _desc_stable(s[i, :Kp])[:k]
        cnt[i] = o.shape[0]
        rows[i, :cnt[i]] = R1[i, o]
        dist[i, :cnt[i]] = D1[i, o]
        sc[i, :cnt[i]] = s[i, o]
    return cnt, rows, dist, sc


# ----------------------------------------------------------------------------- calls under test
def _ws(lib, name, n, dim_or_cb, nq, K, dev, fill=None):
    need = getattr(lib, name + "_workspace_size")(n, dim_or_cb, nq, K)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    return ws


def hamming(name, dev, codes_t, q_t, k, row_offset=0, ws=None):
    N, lib = _N()
    n, cb = codes_t.shape
    nq = q_t.shape[0]
    D = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    R = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    ws = _ws(lib, name, n, cb, nq, k, dev) if ws is None else ws
    N.check(getattr(lib, name)(N.ptr(codes_t), n, cb, row_offset, N.ptr(q_t), nq, k, N.ptr(D), N.ptr(R), N.ptr(ws),
                               ws.numel(), N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return D.cpu().numpy(), R.cpu().numpy()


def search3(name, dev, c, k, K, K3, flags=0, row_offset=0, ws=None):
    N, lib = _N()
    nq = c["qf"].shape[0]
    kout = K if flags & N.VRQ_SEARCH_PHASE1_ONLY else k
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, kout), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, kout), -7, dtype=torch.int32, device=dev)
    s2 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    s3 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    ws = _ws(lib, name, c["n"], c["dim"], nq, K, dev) if ws is None else ws
    rr = None if c["rr"] is None else torch.from_numpy(c["rr"]).to(dev)
    N.check(getattr(lib, name)(N.ptr(c["codes"]), N.ptr(c["x8"]), N.ptr(c["norms"]), N.ptr(rr), c["n"], c["dim"],
                               row_offset, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, K3, flags, N.ptr(cnt),
                               N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), N.ptr(ws), ws.numel(),
                               N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (cnt, rows, dist, s2, s3))


def search2(name, dev, c, deq, k, K, ws=None):
    N, lib = _N()
    nq = c["qf"].shape[0]
    mode, q_t, mm_t, limit = deq
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    sc = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    ws = _ws(lib, name, c["n"], c["dim"], nq, K, dev) if ws is None else ws
    rr = None if c["rr"] is None else torch.from_numpy(c["rr"]).to(dev)
    N.check(getattr(lib, name)(mode, N.ptr(c["codes"]), N.ptr(q_t), N.ptr(mm_t), float(limit), N.ptr(rr), c["n"],
                               c["dim"], 0, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, 0, N.ptr(cnt), N.ptr(rows),
                               N.ptr(dist), N.ptr(sc), N.ptr(ws), ws.numel(), N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (cnt, rows, dist, sc))


def same(a, b):
    """Bit-for-bit equality of two tuples of arrays (NaN == NaN, -0.0 != +0.0)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        if x.dtype == np.float64:
            assert np.array_equal(x.view(np.int64), y.view(np.int64))
        else:
            assert np.array_equal(x, y)


def same_values(got, want):
    """Exact equality against a NumPy-built reference (NaN padding equal; values compared as numbers)."""
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x.shape == y.shape
        assert np.array_equal(x, y, equal_nan=x.dtype == np.float64)


# ----------------------------------------------------------------------------- corpora
N_ROWS = 20_000  # at every dim: at least 3 chunks, the last one partial (asserted from the plan)
_corpus_cache = {}
corpus_of = {}   # id of a corpus's codes tensor -> the corpus with all its queries (sub() keeps the tensor)


def corpus(dev, dim, n=N_ROWS, nq=70, seed=0, dup=True):
    """Random codes / int8 rows / float queries; rows 3k+1 copy rows 3k of the first 3000 (equal scores), every
    7th int8 row is zero (-inf in Phase III), rescore_row sends some rows to another row (duplicated ids)."""
    key = (dim, n, nq, seed, dup)
    if key in _corpus_cache:
        return _corpus_cache[key]
    N, lib = _N()
    rng = np.random.default_rng(1000 * dim + n + seed)
    codes = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
    x8 = rng.integers(-127, 128, (n, dim), dtype=np.int8)
    qf = rng.standard_normal((nq, dim)).astype(np.float32)
    qb = np.packbits(qf > 0, axis=1)
    rr = None
    if dup and n >= 3000:
        codes[1:3000:3] = codes[0:3000:3]
        x8[1:3000:3] = x8[0:3000:3]
        x8[::7] = 0
        rr = np.arange(n, dtype=np.int64)
        rr[5:n:11] = rr[5:n:11] // 2      # an id added twice: scores come from the other row
        qb[1] = codes[n // 2]             # a query equal to a code (distance 0)
        qb[2] = 0                         # an all-zero query
    t = lambda a: torch.from_numpy(a).to(dev)
    x8_t = t(x8)
    norms = torch.empty((n,), dtype=torch.float64, device=dev)
    N.check(lib.vrq_int8_row_norms(N.ptr(x8_t), n, dim, N.ptr(norms), N.stream_handle(dev)), "norms")
    c = dict(dim=dim, n=n, codes=t(codes), x8=x8_t, norms=norms, qf=t(qf), qb=t(qb), rr=rr)
    _corpus_cache[key] = c
    corpus_of[id(c["codes"])] = c
    return c


def sub(c, nq):
    d = dict(c)
    d["qf"], d["qb"] = c["qf"][:nq].contiguous(), c["qb"][:nq].contiguous()
    return d


_p1_cache = {}


def phase1_ref(c, K):
    """Reference Phase I of the corpus's 70 queries at K = 8192, computed once per corpus; prefixes serve every
    smaller K and query count."""
    key = id(c["codes"])
    if key not in _p1_cache:
        assert c["n"] >= 8192
        full = corpus_of[key]
        _p1_cache[key] = ref_phase1(full["codes"], full["qb"], 8192)
    D, R = _p1_cache[key]
    return D[:, :K], R[:, :K]


# ----------------------------------------------------------------------------- Phase I
@pytest.mark.parametrize("nq", (1, 5, 70))
@pytest.mark.parametrize("K", (1025, 3000, 8192))
@pytest.mark.parametrize("dim", (256, 384, 1024, 2048))
def test_phase1_against_reference(dev, dim, K, nq):
    c = corpus(dev, dim)
    chunk_rows, chunks, qpw, prefix = _plan(c["n"], dim, nq, K)[:4]
    assert chunks >= 3 and c["n"] % chunk_rows != 0      # several chunks, the last one partial
    if nq == 70:
        assert qpw < nq                                   # the batch crosses a query-group boundary
    D0, R0 = phase1_ref(c, K)
    D1, R1 = hamming("vrq_hamming_topk_large", dev, c["codes"], c["qb"][:nq].contiguous(), K)
    assert np.array_equal(D1, D0[:nq]) and np.array_equal(R1, R0[:nq])


@pytest.mark.parametrize("dim,K", [(384, 1025), (1024, 1100), (1536, 1025)])
def test_phase1_more_rows_and_a_late_cluster(dev, dim, K):
    """A larger corpus with an odd row count, and one whose best candidates all sit in its last rows."""
    n = 40_003
    c = corpus(dev, dim, n=n, nq=5, seed=1)
    D0, R0 = ref_phase1(c["codes"], c["qb"], K)
    same_values(hamming("vrq_hamming_topk_large", dev, c["codes"], c["qb"], K, row_offset=0), (D0, R0))
    # the K-list is filled from the last chunk alone
    codes = c["codes"].clone()
    codes[n - 2000:] = c["qb"][0]
    codes[n - 2000:, 0] ^= torch.arange(2000, device=dev).to(torch.uint8) & 3
    D0, R0 = ref_phase1(codes, c["qb"], K)
    same_values(hamming("vrq_hamming_topk_large", dev, codes, c["qb"], K), (D0, R0))


@pytest.mark.parametrize("K", (3000, 5000))   # the class at T starts the list (c_lt = 0) / follows a full class
def test_tie_cases(dev, K):
    dim, n = 384, N_ROWS
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (6, dim // 8), dtype=np.uint8)
    pick = rng.integers(0, 6, n)
    codes = torch.from_numpy(base[pick]).to(dev)                 # 6 distinct codes: the class at T exceeds K
    q = torch.from_numpy(np.concatenate([base[:2], rng.integers(0, 256, (2, dim // 8), dtype=np.uint8),
                                         np.zeros((1, dim // 8), np.uint8)])).to(dev)
    chunk_rows, chunks = _plan(n, dim, q.shape[0], K)[:2]
    assert chunks >= 3 and min((pick == j).sum() for j in range(6)) > 3000
    assert all((pick[i * chunk_rows:(i + 1) * chunk_rows] == j).any() for i in range(chunks) for j in range(6))
    D0, R0 = ref_phase1(codes, q, K)                             # ... and spans every chunk boundary
    assert (D0[:, 0] == D0[:, -1]).any() == (K == 3000)          # one class fills a whole K-list
    assert (D0[:2, 0] == 0).all() and (D0[:, -1] == ref_phase1(codes, q, K + 1)[0][:, -1]).all()   # cut inside a class
    same_values(hamming("vrq_hamming_topk_large", dev, codes, q, K), (D0, R0))
    # an all-identical corpus: c_lt = 0, the first K rows
    codes = torch.from_numpy(np.repeat(base[:1], n, axis=0)).to(dev)
    D1, R1 = hamming("vrq_hamming_topk_large", dev, codes, q, K)
    assert np.array_equal(R1, np.tile(np.arange(K), (q.shape[0], 1)))
    assert np.array_equal(D1, ref_phase1(codes, q, K)[0]) and (D1[0] == 0).all()


@pytest.mark.parametrize("dim", (384, 1024))
def test_small_corpora(dev, dim):
    rng = np.random.default_rng(dim)
    q = torch.from_numpy(rng.integers(0, 256, (3, dim // 8), dtype=np.uint8)).to(dev)
    for n, K in ((5000, 5000), (1500, 1500), (1200, 3000), (1, 1025), (1, 1), (70, 8192)):   # K = n, n < K, n = 1
        codes = torch.from_numpy(rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)).to(dev)
        D0, R0 = ref_phase1(codes, q, K)
        D1, R1 = hamming("vrq_hamming_topk_large", dev, codes, q, K, row_offset=7)
        assert np.array_equal(D1, D0) and np.array_equal(R1, np.where(R0 >= 0, R0 + 7, -1))
        assert (R1[:, min(n, K):] == -1).all() and (D1[:, min(n, K):] == INT32_MAX).all()


@pytest.mark.parametrize("dim", (384, 1024))
def test_fewer_rows_than_candidates(dev, dim):
    """n < K through the search calls: counts = n (or min(k, K3, n)), padding in the tail."""
    from vectorragquantization_amd import _native as N
    n, K = 1200, 3000
    c = corpus(dev, dim, n=n, nq=3, seed=2, dup=False)
    D1, R1 = ref_phase1(c["codes"], c["qb"], K)
    cnt, rows, dist, s2, s3 = search3("vrq_search3_large", dev, c, 10, K, 30, N.VRQ_SEARCH_PHASE1_ONLY)
    assert (cnt == n).all() and np.array_equal(rows, R1) and np.array_equal(dist, D1)
    assert (rows[:, n:] == -1).all() and (dist[:, n:] == INT32_MAX).all()
    for k, K3 in ((2000, 2500), (100, 300)):
        got = search3("vrq_search3_large", dev, c, k, K, K3)
        same_values(got, ref_search3(dev, c, D1, R1, k, K3))
        assert (got[0] == min(k, K3, n)).all() and np.isnan(got[3][:, min(k, n):]).all()
    deq = _deq(dev, c, "sbin")
    got = search2("vrq_search2_large", dev, c, deq, 2000, K)
    same_values(got, ref_search2(dev, c, deq, D1, R1, 2000))
    assert (got[0] == n).all() and (got[1][:, n:] == -1).all()


# ----------------------------------------------------------------------------- the existing path
def _deq(dev, c, mode):
    """(ABI mode, stored rows, minmax, limit) of a vrq_search2 mode for the corpus."""
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd import quant
    if mode == "sbin":
        return N.VRQ_RESCORE_SIGNED_BINARY, c["codes"], None, 0.0
    rng = np.random.default_rng(c["dim"] + len(mode))
    xf = torch.from_numpy((rng.standard_normal((c["n"], c["dim"])) * 0.1).astype(np.float32)).to(dev)
    if mode == "f32":
        return N.VRQ_RESCORE_F32, xf, None, 0.0
    e = quant.encode(mode, xf, 0.3, dev)
    return quant._DEQ_MODES[mode], e["q"], e["minmax"], 0.3


@pytest.mark.parametrize("K", (100, 1000, 1024))
@pytest.mark.parametrize("dim", (384, 1024))
def test_equals_the_existing_path(dev, dim, K):
    from vectorragquantization_amd import _native as N
    c = sub(corpus(dev, dim), 5)
    same(hamming("vrq_hamming_topk_large", dev, c["codes"], c["qb"], K, row_offset=3),
         hamming("vrq_hamming_topk", dev, c["codes"], c["qb"], K, row_offset=3))
    for k, K3, flags in ((K // 10, 3 * (K // 10), 0), (K, 2 * K, 0), (K, K, N.VRQ_SEARCH_PHASE1_ONLY)):
        same(search3("vrq_search3_large", dev, c, k, K, K3, flags, row_offset=11),
             search3("vrq_search3_dim", dev, c, k, K, K3, flags, row_offset=11))
    for mode in ("sbin", "int8g", "int4", "f32"):
        deq = _deq(dev, c, mode)
        same(search2("vrq_search2_large", dev, c, deq, K // 10, K), search2("vrq_search2", dev, c, deq, K // 10, K))


# ----------------------------------------------------------------------------- K = 3000
@pytest.mark.parametrize("k,K3", [(300, 900), (300, 5000), (2000, 900)])   # also K3 > K and k > K3
@pytest.mark.parametrize("dim", (384, 1024))
def test_three_phase_at_3000(dev, dim, k, K3):
    K = 3000
    c = sub(corpus(dev, dim), 5)     # duplicated ids through rescore_row, zero int8 rows, duplicated rows
    D1, R1 = phase1_ref(c, K)
    D1, R1 = D1[:5], R1[:5]
    want = ref_search3(dev, c, D1, R1, k, K3, row_offset=1000)
    got = search3("vrq_search3_large", dev, c, k, K, K3, row_offset=1000)
    same_values(got, want)
    if k >= K3:
        assert np.isneginf(got[4]).any()             # zero int8 rows reached Phase III and sort last


def test_three_phase_ties_keep_phase1_order(dev):
    """Equal scores (duplicated rows) come out in Phase-I order: checked on the reference itself too."""
    dim, K, k, K3 = 384, 3000, 3000, 3000
    c = sub(corpus(dev, dim), 3)
    D1, R1 = phase1_ref(c, K)
    want = ref_search3(dev, c, D1[:3], R1[:3], k, K3)
    got = search3("vrq_search3_large", dev, c, k, K, K3)
    same_values(got, want)
    cnt, rows, dist, s2, s3 = got
    tied = 0
    for i in range(3):
        rank = {int(r): j for j, r in enumerate(R1[i])}
        for j in range(cnt[i] - 1):
            if s3[i, j] == s3[i, j + 1] and s2[i, j] == s2[i, j + 1]:
                tied += 1
                assert rank[int(rows[i, j])] < rank[int(rows[i, j + 1])]
    assert tied > 10


def test_phase1_only_and_row_offset(dev):
    from vectorragquantization_amd import _native as N
    dim, K = 1024, 3000
    c = sub(corpus(dev, dim), 5)
    D1, R1 = phase1_ref(c, K)
    cnt, rows, dist, s2, s3 = search3("vrq_search3_large", dev, c, 10, K, 30, N.VRQ_SEARCH_PHASE1_ONLY,
                                      row_offset=1 << 33)
    assert (cnt == K).all() and np.array_equal(dist, D1[:5]) and np.array_equal(rows, R1[:5] + (1 << 33))
    assert (s2 == -7.0).all() and (s3 == -7.0).all()     # Phase-I-only calls write no scores


@pytest.mark.parametrize("mode", ("sbin", "int8g", "int4", "f32"))
@pytest.mark.parametrize("dim", (384, 1024))
def test_two_phase_at_3000(dev, dim, mode):
    K = 3000
    c = sub(corpus(dev, dim), 5)
    deq = _deq(dev, c, mode)
    D1, R1 = phase1_ref(c, K)
    for k in (300, 3000):
        same_values(search2("vrq_search2_large", dev, c, deq, k, K), ref_search2(dev, c, deq, D1[:5], R1[:5], k))


# ----------------------------------------------------------------------------- the classes
def test_enhanced_class_k150(dev, tmp_path):
    from vectorragquantization_amd.embed import SyntheticCohereProvider
    from vectorragquantization_amd.enhanced import CohereEnhancedVectorDB
    c = corpus(dev, 1024, dup=False, seed=3, nq=4)
    db = CohereEnhancedVectorDB(str(tmp_path / "db"), provider=SyntheticCohereProvider(device=dev), device=dev)
    db.add_vectors(np.arange(c["n"]) + 500, c["x8"], c["codes"])
    res = db.search_vectors(c["qf"], c["qb"], k=150)                      # K = 1500 with the default oversample
    D1, R1 = ref_phase1(c["codes"], c["qb"], 1500)
    cnt, rows, dist, b, cs = ref_search3(dev, c, D1, R1, 150, 450)
    same_values((res.count.cpu().numpy(), res.row.cpu().numpy(), res.hamming.cpu().numpy(), res.binary.cpu().numpy(),
                 res.cosine.cpu().numpy()), (cnt, rows, dist, b, cs))
    assert np.array_equal(res.doc_id.cpu().numpy(), rows + 500)
    from vectorragquantization_amd import _native as N
    with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
        db.search_vectors(c["qf"], c["qb"], k=900)                        # k * binary_oversample = 9000


def test_binary_index_search_2000(dev):
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    c = corpus(dev, 384, dup=False, seed=4, nq=4)
    idx = BinaryIndexIDMap2(384, device=dev)
    idx.add_with_ids(c["codes"], np.arange(c["n"]) * 2)
    D, L = idx.search(c["qb"], 2000)
    D1, R1 = ref_phase1(c["codes"], c["qb"], 2000)
    assert np.array_equal(D, D1) and np.array_equal(L, R1 * 2)


def test_quant_wrappers_k1500(dev):
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd import quant
    c = sub(corpus(dev, 384), 5)
    mode, q_t, mm_t, limit = deq = _deq(dev, c, "int8g")
    rr = torch.from_numpy(c["rr"]).to(dev)
    D1, R1 = phase1_ref(c, 1500)
    cnt, rows, dist, sc = ref_search2(dev, c, deq, D1[:5], R1[:5], 150)
    for fn in (quant.search2, quant.vectordb_search):
        r, d, s = fn("int8g", c["codes"], q_t, c["qf"], c["qb"], k=150, binary_oversample=10, limit=limit,
                     rescore_row=rr)
        torch.cuda.synchronize()
        same_values((r.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy()), (rows, dist, sc))
        with pytest.raises(N.VrqNativeError, match=r"9000.*8192"):
            fn("int8g", c["codes"], q_t, c["qf"], c["qb"], k=900, binary_oversample=10, limit=limit, rescore_row=rr)


# ----------------------------------------------------------------------------- workspace hygiene
def test_workspace_prefilled_with_ff(dev):
    """The same call twice on one workspace pre-filled with 0xFF (and once zero-filled): every count and prefix
    is written before it is read."""
    N, lib = _N()
    for n, K in ((N_ROWS, 3000), (40_003, 1025)):
        c = corpus(dev, 384, n=n, nq=5, seed=1) if n != N_ROWS else sub(corpus(dev, 384), 5)
        ws = _ws(lib, "vrq_search3_large", n, 384, 5, K, dev, fill=0xFF)
        a = search3("vrq_search3_large", dev, c, K // 10, K, 3 * (K // 10), ws=ws)
        b = search3("vrq_search3_large", dev, c, K // 10, K, 3 * (K // 10), ws=ws)
        ws.fill_(0)
        z = search3("vrq_search3_large", dev, c, K // 10, K, 3 * (K // 10), ws=ws)
        same(a, b)
        same(a, z)
        D1, R1 = ref_phase1(c["codes"], c["qb"], K)
        same_values(a, ref_search3(dev, c, D1, R1, K // 10, 3 * (K // 10)))
