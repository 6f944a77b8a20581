"""GPU checks of the filtered search (vrq_*_filtered: a row allow-bitmap through the counting scan K1h).
Every comparison is exact.  Reference distances are plain torch ops on the device (xor + a byte-popcount
table) with the disallowed rows pushed out of the (dist, row) sort; reference scores are the stand-alone
vrq_rescore_*_dim / vrq_rescore_dequant calls on the Phase-I rows, ordered by NumPy stable sorts -- no kernel
under test appears in a reference.  The defining property is checked once per entry point: the filtered call
equals the *_large call on the gathered allowed rows, rows mapped back.  The stand-alone rescoring kernels of
the reference are pinned against exact rational arithmetic by tests/test_gpu_exact_scores.py.

n = 12 325 = 3 x 4096 + 37 rows: the plan gives 4 chunks and a ragged last tile (asserted), the smallest
shape at which chunk prefixes, the ragged tile and the last bitmap word can go wrong.  Dims 256, 384 (the
unrotated C = 3 ring), 1024 and 2048 (the two-wave workgroup): a template instance each."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
POP = np.array([bin(i).count("1") for i in range(256)], np.int16)
N_ROWS = 12_325
NQ = 17
DIMS = (256, 384, 1024, 2048)
NONE_KEY = np.iinfo(np.int64).max


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


# ----------------------------------------------------------------------------- bitmaps
def pack(mask, tail=False):
    """bool[n] -> the ABI's words as an int64 array (NumPy only: not the helper under test in filters.py);
    tail: every bit past n in the last word set."""
    n = mask.shape[0]
    by = np.zeros(((n + 63) // 64) * 8, np.uint8)
    p = np.packbits(mask, bitorder="little")
    by[:p.shape[0]] = p
    w = by.view("<u8").copy()
    if tail and n % 64:
        w[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    return w.view(np.int64)


def masks(n, chunk_rows):
    rng = np.random.default_rng(77)
    m = {}
    m["ones"] = np.ones(n, bool)
    m["zeros"] = np.zeros(n, bool)
    m["last"] = np.arange(n) == n - 1
    m["first"] = np.arange(n) == 0
    m["r50"] = rng.random(n) < 0.5
    m["r01"] = rng.random(n) < 0.01
    lo, hi = chunk_rows + 37, 2 * chunk_rows + 1000 + 5      # mid-tile in chunk 1 ... mid-tile in chunk 2
    m["range"] = (np.arange(n) >= lo) & (np.arange(n) < hi)
    m["altwords"] = (np.arange(n) >> 6) % 2 == 0              # all-ones and zero words alternate
    return m


MASKS = ("ones", "zeros", "last", "first", "r50", "r01", "range", "altwords")


# ----------------------------------------------------------------------------- corpus and references
_corpus_cache = {}


def corpus(dev, dim):
    """Random codes / int8 rows / float queries; rows 3k+1 copy rows 3k of the first 3000 (equal scores), every
    7th int8 row is zero, rescore_row sends some rows to another row (duplicated ids).  With the full distance
    matrix of its 17 queries (torch ops), computed once."""
    if dim in _corpus_cache:
        return _corpus_cache[dim]
    N, lib = _N()
    n, nq = N_ROWS, NQ
    rng = np.random.default_rng(1000 * dim + n)
    codes = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
    x8 = rng.integers(-127, 128, (n, dim), dtype=np.int8)
    qf = rng.standard_normal((nq, dim)).astype(np.float32)
    qb = np.packbits(qf > 0, axis=1)
    codes[1:3000:3] = codes[0:3000:3]
    x8[1:3000:3] = x8[0:3000:3]
    x8[::7] = 0
    rr = np.arange(n, dtype=np.int64)
    rr[5:n:11] = rr[5:n:11] // 2          # an id added twice: scores come from the other row
    qb[1] = codes[n // 2]                 # a query equal to a code (distance 0)
    qb[2] = 0                             # an all-zero query
    t = lambda a: torch.from_numpy(a).to(dev)
    x8_t = t(x8)
    norms = torch.empty((n,), dtype=torch.float64, device=dev)
    N.check(lib.vrq_int8_row_norms(N.ptr(x8_t), n, dim, N.ptr(norms), N.stream_handle(dev)), "norms")
    c = dict(dim=dim, n=n, codes=t(codes), x8=x8_t, norms=norms, qf=t(qf), qb=t(qb), rr=rr)
    c["dmat"] = dist_matrix(c["codes"], c["qb"])
    chunk_rows, chunks = _plan(n, dim, nq, 1500)[:2]
    assert chunks >= 3 and n % chunk_rows != 0 and n % 64 != 0   # chunk prefixes, a ragged tile, a partial word
    c["chunk_rows"] = chunk_rows
    c["masks"] = masks(n, chunk_rows)
    lo = np.flatnonzero(c["masks"]["range"])
    assert lo[0] // chunk_rows == 1 and lo[-1] // chunk_rows == 2 and lo[0] % 64 and (lo[-1] + 1) % 64
    _corpus_cache[dim] = c
    return c


def sub(c, nq):
    d = dict(c)
    d["qf"], d["qb"], d["dmat"] = c["qf"][:nq].contiguous(), c["qb"][:nq].contiguous(), c["dmat"][:nq]
    return d


def dist_matrix(codes_t, q_t):
    pop = torch.from_numpy(POP).to(codes_t.device)
    return torch.stack([pop[(codes_t ^ q_t[i]).long()].sum(1, dtype=torch.int64) for i in range(q_t.shape[0])])


def ref_phase1(dmat, mask, K):
    """(dist i32[nq, K], rows i64[nq, K]): the min(K, allowed) smallest allowed rows in (dist, row) order,
    padded INT32_MAX / -1.  The disallowed rows are pushed out of the sort."""
    nq, n = dmat.shape
    key = dmat * (1 << 32) + torch.arange(n, device=dmat.device)
    key = torch.where(torch.from_numpy(mask).to(dmat.device), key, torch.full_like(key, NONE_KEY))
    key = torch.sort(key, dim=1).values[:, :K].cpu().numpy()
    D = np.full((nq, K), INT32_MAX, np.int32)
    R = np.full((nq, K), -1, np.int64)
    ok = key != NONE_KEY
    D[:, :key.shape[1]][ok] = (key >> 32)[ok]
    R[:, :key.shape[1]][ok] = (key & 0xffffffff)[ok]
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


# ----------------------------------------------------------------------------- calls under test
def _ws(lib, name, n, dim_or_cb, nq, K, dev, fill=None):
    need = getattr(lib, name + "_workspace_size")(n, dim_or_cb, nq, K)
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    return ws


def _allow(dev, words):
    return None if words is None else torch.from_numpy(np.ascontiguousarray(words)).to(dev)


def hamming(dev, codes_t, q_t, k, words=None, row_offset=0, ws=None):
    """vrq_hamming_topk_filtered, or vrq_hamming_topk_large when words is None."""
    N, lib = _N()
    name = "vrq_hamming_topk_large" if words is None else "vrq_hamming_topk_filtered"
    n, cb = codes_t.shape
    nq = q_t.shape[0]
    D = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    R = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    ws = _ws(lib, name, n, cb, nq, k, dev) if ws is None else ws
    a = _allow(dev, words)
    extra = () if words is None else (N.ptr(a),)
    N.check(getattr(lib, name)(N.ptr(codes_t), n, cb, row_offset, N.ptr(q_t), nq, k, *extra, N.ptr(D), N.ptr(R),
                               N.ptr(ws), ws.numel(), N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return D.cpu().numpy(), R.cpu().numpy()


def search3(dev, c, k, K, K3, words=None, flags=0, row_offset=0, ws=None):
    N, lib = _N()
    name = "vrq_search3_large" if words is None else "vrq_search3_filtered"
    nq = c["qf"].shape[0]
    kout = K if flags & N.VRQ_SEARCH_PHASE1_ONLY else k
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, kout), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, kout), -7, dtype=torch.int32, device=dev)
    s2 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    s3 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    ws = _ws(lib, name, c["n"], c["dim"], nq, K, dev) if ws is None else ws
    rr = None if c["rr"] is None else torch.from_numpy(c["rr"]).to(dev)
    a = _allow(dev, words)
    extra = () if words is None else (N.ptr(a),)
    N.check(getattr(lib, name)(N.ptr(c["codes"]), N.ptr(c["x8"]), N.ptr(c["norms"]), N.ptr(rr), c["n"], c["dim"],
                               row_offset, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, K3, flags, *extra, N.ptr(cnt),
                               N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), N.ptr(ws), ws.numel(),
                               N.stream_handle(dev)), name)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (cnt, rows, dist, s2, s3))


def search2(dev, c, deq, k, K, words=None, ws=None):
    N, lib = _N()
    name = "vrq_search2_large" if words is None else "vrq_search2_filtered"
    nq = c["qf"].shape[0]
    mode, q_t, mm_t, limit = deq
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    sc = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    ws = _ws(lib, name, c["n"], c["dim"], nq, K, dev) if ws is None else ws
    rr = None if c["rr"] is None else torch.from_numpy(c["rr"]).to(dev)
    a = _allow(dev, words)
    extra = () if words is None else (N.ptr(a),)
    N.check(getattr(lib, name)(mode, N.ptr(c["codes"]), N.ptr(q_t), N.ptr(mm_t), float(limit), N.ptr(rr), c["n"],
                               c["dim"], 0, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, 0, *extra, N.ptr(cnt),
                               N.ptr(rows), N.ptr(dist), N.ptr(sc), N.ptr(ws), ws.numel(), N.stream_handle(dev)), name)
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


def gathered(dev, c, mask, deq=None):
    """The corpus with the disallowed rows removed in row order (what remove_ids would leave), the map from its
    rows back to the original ones, and the stored rows of `deq` gathered the same way.  rescore_row is given
    up: the gathered corpus scores every row from itself, so callers compare with rr = None on both sides."""
    keep = np.flatnonzero(mask)
    kt = torch.from_numpy(keep).to(dev)
    g = dict(c)
    g["n"] = int(keep.shape[0])
    g["codes"], g["x8"], g["norms"] = c["codes"][kt].contiguous(), c["x8"][kt].contiguous(), c["norms"][kt].contiguous()
    g["rr"] = None
    gd = None
    if deq is not None:
        mode, q_t, mm_t, limit = deq
        gd = (mode, q_t[kt].contiguous(), None if mm_t is None else mm_t[kt].contiguous(), limit)
    return g, keep, gd


def map_back(rows, keep):
    return np.where(rows >= 0, keep[np.maximum(rows, 0)], rows)


# ----------------------------------------------------------------------------- Phase I
@pytest.mark.parametrize("tail", (False, True))
@pytest.mark.parametrize("mname", MASKS)
@pytest.mark.parametrize("dim", DIMS)
def test_phase1_against_reference(dev, dim, mname, tail):
    """Every bitmap x nq in (1, 5, 17) x K in (10, 1500, 8192), once more with the bits past n set."""
    c = corpus(dev, dim)
    mask = c["masks"][mname]
    words = pack(mask, tail)
    allowed = int(mask.sum())
    D0, R0 = ref_phase1(c["dmat"], mask, 8192)
    qpw = _plan(c["n"], dim, NQ, 8192)[2]
    assert qpw < NQ                                      # 17 queries: more than one count group
    for K in (10, 1500, 8192):
        for nq in (1, 5, NQ):
            D1, R1 = hamming(dev, c["codes"], c["qb"][:nq].contiguous(), K, words)
            assert np.array_equal(D1, D0[:nq, :K]) and np.array_equal(R1, R0[:nq, :K]), (K, nq)
            m = min(K, allowed)
            assert (R1[:, :m] >= 0).all() and (R1[:, m:] == -1).all() and (D1[:, m:] == INT32_MAX).all()
            assert mask[R1[:, :m]].all()


@pytest.mark.parametrize("dim", DIMS)
def test_exact_list_sizes(dev, dim):
    """Bitmaps with exactly K - 1, K and K + 1 allowed rows."""
    c = corpus(dev, dim)
    rng = np.random.default_rng(dim)
    for K in (10, 1500):
        for allowed in (K - 1, K, K + 1):
            mask = np.zeros(c["n"], bool)
            mask[rng.choice(c["n"], allowed, replace=False)] = True
            D0, R0 = ref_phase1(c["dmat"][:5], mask, K)
            D1, R1 = hamming(dev, c["codes"], c["qb"][:5].contiguous(), K, pack(mask, True))
            assert np.array_equal(D1, D0) and np.array_equal(R1, R0), (K, allowed)
            assert ((R1 >= 0).sum(1) == min(K, allowed)).all()


@pytest.mark.parametrize("dim", (384, 1024))
def test_ties_keep_the_first_allowed_rows(dev, dim):
    """8 distinct codes: hundreds of rows sit at T, the filter removes every third of them; the rows kept at T
    are the first allowed ones in row order."""
    n, K = N_ROWS, 1500
    rng = np.random.default_rng(5 + dim)
    base = rng.integers(0, 256, (8, dim // 8), dtype=np.uint8)
    pick = rng.integers(0, 8, n)
    codes = torch.from_numpy(base[pick]).to(dev)
    q = torch.from_numpy(np.concatenate([base[:2], rng.integers(0, 256, (2, dim // 8), dtype=np.uint8)])).to(dev)
    mask = np.ones(n, bool)
    for j in range(8):
        r = np.flatnonzero(pick == j)
        mask[r[::3]] = False                                     # every third row of each class
    dmat = dist_matrix(codes, q)
    D0, R0 = ref_phase1(dmat, mask, K)
    assert min(((pick == j) & mask).sum() for j in range(8)) > 900
    D1, R1 = hamming(dev, codes, q, K, pack(mask))
    assert np.array_equal(D1, D0) and np.array_equal(R1, R0)
    for i in range(q.shape[0]):
        T = D1[i, -1]
        at_T = np.flatnonzero((dmat[i].cpu().numpy() == T) & mask)
        kept = R1[i][D1[i] == T]
        assert at_T.shape[0] > kept.shape[0] >= 100              # the list is cut inside the class at T
        assert np.array_equal(kept, at_T[:kept.shape[0]])        # ... after its first allowed rows


@pytest.mark.parametrize("dim", (384, 2048))
def test_row_offset_and_all_ones_equals_large(dev, dim):
    c = corpus(dev, dim)
    q = c["qb"][:5].contiguous()
    for K in (10, 1500, 8192):
        for tail in (False, True):
            same(hamming(dev, c["codes"], q, K, pack(c["masks"]["ones"], tail), row_offset=3),
                 hamming(dev, c["codes"], q, K, None, row_offset=3))
    mask = c["masks"]["r50"]
    D0, R0 = ref_phase1(c["dmat"][:5], mask, 1500)
    D1, R1 = hamming(dev, c["codes"], q, 1500, pack(mask), row_offset=1 << 33)
    assert np.array_equal(D1, D0) and np.array_equal(R1, R0 + (1 << 33))


@pytest.mark.parametrize("dim", DIMS)
def test_hamming_equals_large_on_the_gathered_rows(dev, dim):
    c = sub(corpus(dev, dim), 5)
    for mname in ("r50", "range", "r01"):
        mask = c["masks"][mname]
        g, keep, _ = gathered(dev, c, mask)
        for K in (10, 1500):
            D1, R1 = hamming(dev, c["codes"], c["qb"], K, pack(mask, True))
            Dg, Rg = hamming(dev, g["codes"], c["qb"], K)
            same((D1, R1), (Dg, map_back(Rg, keep)))


# ----------------------------------------------------------------------------- the three-phase call
@pytest.mark.parametrize("mname", ("r50", "r01", "range", "ones", "zeros", "last"))
@pytest.mark.parametrize("dim", DIMS)
def test_search3_against_reference(dev, dim, mname):
    N, _ = _N()
    c = sub(corpus(dev, dim), 5)
    mask = c["masks"][mname]
    words = pack(mask, True)
    allowed = int(mask.sum())
    for K, k, K3 in ((1500, 150, 450), (10, 10, 30), (8192, 300, 8192)):
        D1, R1 = ref_phase1(c["dmat"], mask, K)
        got = search3(dev, c, k, K, K3, words, row_offset=1000)
        same_values(got, ref_search3(dev, c, D1, R1, k, K3, row_offset=1000))
        assert (got[0] == min(k, K3, K, allowed)).all()
        cnt, rows, dist, s2, s3 = search3(dev, c, k, K, K3, words, N.VRQ_SEARCH_PHASE1_ONLY, row_offset=1000)
        assert (cnt == min(K, allowed)).all() and np.array_equal(dist, D1)
        assert np.array_equal(rows, np.where(R1 >= 0, R1 + 1000, -1))
        assert (s2 == -7.0).all() and (s3 == -7.0).all()     # Phase-I-only calls write no scores
    if mname == "ones":
        same(search3(dev, c, 150, 1500, 450, words), search3(dev, c, 150, 1500, 450, None))
    if mname == "r50":
        # scores come from rescore_row[r] whether or not that row is itself allowed
        D1, R1 = ref_phase1(c["dmat"], mask, 1500)
        tgt = c["rr"][R1[R1 >= 0]]
        assert (~mask[tgt]).sum() > 20 and (tgt != R1[R1 >= 0]).sum() > 20


@pytest.mark.parametrize("dim", (384, 1024))
def test_search3_equals_large_on_the_gathered_rows(dev, dim):
    """The defining property.  rescore_row = None on both sides: the gathered corpus has no row to send a
    disallowed target to."""
    c = sub(corpus(dev, dim), 5)
    c["rr"] = None
    for mname in ("r50", "range"):
        mask = c["masks"][mname]
        g, keep, _ = gathered(dev, c, mask)
        for k, K, K3 in ((150, 1500, 450), (10, 10, 30)):
            cnt, rows, dist, s2, s3 = search3(dev, c, k, K, K3, pack(mask))
            gc, grows, gd, g2, g3 = search3(dev, g, k, K, K3, None)
            same((cnt, rows, dist, s2, s3), (gc, map_back(grows, keep), gd, g2, g3))


# ----------------------------------------------------------------------------- the two-phase call
@pytest.mark.parametrize("mode", ("sbin", "int8g", "int4", "f32"))   # signed binary, a global, a local mode, float
@pytest.mark.parametrize("dim", (384, 1024))
def test_search2_against_reference_and_gathered(dev, dim, mode):
    c = sub(corpus(dev, dim), 5)
    deq = _deq(dev, c, mode)
    for mname in ("r50", "range", "zeros"):
        mask = c["masks"][mname]
        words = pack(mask, True)
        for K, k in ((1500, 150), (10, 10), (8192, 8192)):
            D1, R1 = ref_phase1(c["dmat"], mask, K)
            got = search2(dev, c, deq, k, K, words)
            same_values(got, ref_search2(dev, c, deq, D1, R1, k))
            assert (got[0] == min(k, K, int(mask.sum()))).all()
    # the defining property
    c0 = dict(c)
    c0["rr"] = None
    mask = c["masks"]["r50"]
    g, keep, gdeq = gathered(dev, c0, mask, deq)
    cnt, rows, dist, sc = search2(dev, c0, deq, 150, 1500, pack(mask))
    gc, grows, gd, gs = search2(dev, g, gdeq, 150, 1500, None)
    same((cnt, rows, dist, sc), (gc, map_back(grows, keep), gd, gs))
    same(search2(dev, c, deq, 150, 1500, pack(c["masks"]["ones"], True)), search2(dev, c, deq, 150, 1500, None))


# ----------------------------------------------------------------------------- the staged scan
def _scan(dev, c, K, words, stages, ws):
    N, lib = _N()
    a = _allow(dev, words)
    N.check(lib.vrq_scan_filtered(N.ptr(c["codes"]), c["n"], c["dim"], N.ptr(c["qb"]), c["qb"].shape[0], K, stages,
                                  N.ptr(a), N.ptr(ws), ws.numel(), N.stream_handle(dev)), "vrq_scan_filtered")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dim", DIMS)
def test_scan_stages_equal_the_single_call(dev, dim):
    """COUNT, THRESHOLD, EMIT issued one by one leave the K-lists of the single call, and those are the
    reference's rows (as a set per list part: the scan leaves them unsorted); the defining property of
    vrq_scan_filtered against vrq_scan_large on the gathered rows."""
    N, lib = _N()
    c = sub(corpus(dev, dim), 5)
    K = 1500
    info = _plan(c["n"], dim, 5, K)
    off_lists = info[6]
    for mname in ("r50", "range", "r01"):
        mask = c["masks"][mname]
        words = pack(mask, True)
        ws1 = _ws(lib, "vrq_scan_filtered", c["n"], dim, 5, K, dev, fill=0xFF)
        ws2 = _ws(lib, "vrq_scan_filtered", c["n"], dim, 5, K, dev, fill=0x00)
        _scan(dev, c, K, words, 0, ws1)
        for bit in (N.VRQ_LARGE_STAGE_COUNT, N.VRQ_LARGE_STAGE_THRESHOLD, N.VRQ_LARGE_STAGE_EMIT):
            _scan(dev, c, K, words, bit, ws2)
        l1 = ws1[off_lists:off_lists + 5 * K * 8].cpu().numpy().view(np.int64).reshape(5, K)
        l2 = ws2[off_lists:off_lists + 5 * K * 8].cpu().numpy().view(np.int64).reshape(5, K)
        assert np.array_equal(l1, l2)
        D0, R0 = ref_phase1(c["dmat"], mask, K)
        want = np.where(R0 >= 0, (D0.astype(np.int64) << 40) | R0, -1)     # dist << 40 | row, all-ones padded
        assert np.array_equal(np.sort(l1.view(np.uint64), axis=1), np.sort(want.view(np.uint64), axis=1))
        # vrq_scan_large on the gathered rows: the same lists with rows mapped back
        g, keep, _ = gathered(dev, c, mask)
        wsg = _ws(lib, "vrq_search3_large", g["n"], dim, 5, K, dev)
        N.check(lib.vrq_scan_large(N.ptr(g["codes"]), g["n"], dim, N.ptr(c["qb"]), 5, K, 0, N.ptr(wsg), wsg.numel(),
                                   N.stream_handle(dev)), "vrq_scan_large")
        torch.cuda.synchronize()
        og = _plan(g["n"], dim, 5, K)[6]
        lg = wsg[og:og + 5 * K * 8].cpu().numpy().view(np.int64).reshape(5, K)
        back = np.where(lg != -1, (lg >> 40 << 40) | keep[np.minimum(lg & ((1 << 40) - 1), g["n"] - 1)], -1)
        assert np.array_equal(np.sort(l1.view(np.uint64), axis=1), np.sort(back.view(np.uint64), axis=1))


# ----------------------------------------------------------------------------- workspace hygiene, empty shapes
@pytest.mark.parametrize("dim", (384, 1024))
def test_workspace_prefilled(dev, dim):
    """The same call on a workspace pre-filled with 0xFF, again, and with 0x00: every count, prefix and list
    slot is written before it is read -- with an all-zero bitmap and a sparse one too."""
    N, lib = _N()
    c = sub(corpus(dev, dim), 5)
    for mname in ("r50", "r01", "zeros", "last"):
        words = pack(c["masks"][mname])
        for K in (1500, 10):
            ws = _ws(lib, "vrq_search3_filtered", c["n"], dim, 5, K, dev, fill=0xFF)
            a = search3(dev, c, K // 10, K, 3 * (K // 10), words, ws=ws)
            b = search3(dev, c, K // 10, K, 3 * (K // 10), words, ws=ws)
            ws.fill_(0)
            z = search3(dev, c, K // 10, K, 3 * (K // 10), words, ws=ws)
            same(a, b)
            same(a, z)
            D1, R1 = ref_phase1(c["dmat"], c["masks"][mname], K)
            same_values(a, ref_search3(dev, c, D1, R1, K // 10, 3 * (K // 10)))


def test_all_zero_bitmap_is_all_padding(dev):
    c = sub(corpus(dev, 1024), 5)
    words = pack(c["masks"]["zeros"], True)                      # (the bits past n are set: they are ignored)
    assert words[-1] != 0 and (words[:-1] == 0).all()
    D, R = hamming(dev, c["codes"], c["qb"], 1500, words)
    assert (D == INT32_MAX).all() and (R == -1).all()
    cnt, rows, dist, s2, s3 = search3(dev, c, 150, 1500, 450, words)
    assert (cnt == 0).all() and (rows == -1).all() and (dist == INT32_MAX).all()
    assert np.isnan(s2).all() and np.isnan(s3).all()
    cnt, rows, dist, sc = search2(dev, c, _deq(dev, c, "sbin"), 150, 1500, words)
    assert (cnt == 0).all() and (rows == -1).all() and (dist == INT32_MAX).all() and np.isnan(sc).all()


def test_empty_shapes_behave_as_the_large_calls(dev):
    """n, K or k = 0: counts 0, padding written, no bitmap read (a null one is accepted)."""
    N, lib = _N()
    c = sub(corpus(dev, 384), 3)
    s = N.stream_handle(dev)
    for n, k, K in ((0, 10, 100), (c["n"], 10, 0), (c["n"], 0, 100)):
        outs = {}
        for name in ("vrq_search3_large", "vrq_search3_filtered"):
            cnt = torch.full((3,), -7, dtype=torch.int32, device=dev)
            rows = torch.full((3, max(k, 1)), -7, dtype=torch.int64, device=dev)
            dist = torch.full((3, max(k, 1)), -7, dtype=torch.int32, device=dev)
            s2 = torch.full((3, max(k, 1)), -7.0, dtype=torch.float64, device=dev)
            s3 = torch.full((3, max(k, 1)), -7.0, dtype=torch.float64, device=dev)
            extra = (0,) if name.endswith("filtered") else ()
            N.check(getattr(lib, name)(N.ptr(c["codes"]), N.ptr(c["x8"]), N.ptr(c["norms"]), 0, n, 384, 0,
                                       N.ptr(c["qf"]), N.ptr(c["qb"]), 3, k, K, 30, 0, *extra, N.ptr(cnt), N.ptr(rows),
                                       N.ptr(dist), N.ptr(s2), N.ptr(s3), 0, 0, s), name)
            torch.cuda.synchronize()
            outs[name] = tuple(t.cpu().numpy() for t in (cnt, rows, dist, s2, s3))
        same(outs["vrq_search3_large"], outs["vrq_search3_filtered"])
        assert (outs["vrq_search3_filtered"][0] == 0).all()


# ----------------------------------------------------------------------------- the Python wrappers
def test_index_and_quant_wrappers(dev):
    from vectorragquantization_amd import filters, quant
    from vectorragquantization_amd.enhanced import search3 as py_search3
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    c = sub(corpus(dev, 384), 5)
    mask = c["masks"]["r50"]
    allow = filters.row_bitmap(torch.from_numpy(mask).to(dev))
    assert np.array_equal(allow.cpu().numpy(), pack(mask))       # the helper on the device
    idx = BinaryIndexIDMap2(384, device=dev)
    idx.add_with_ids(c["codes"], np.arange(c["n"]) * 2)
    for K in (10, 2000):
        D0, R0 = ref_phase1(c["dmat"], mask, K)
        D, L = idx.search(c["qb"], K, allow=allow)
        assert np.array_equal(D, D0) and np.array_equal(L, np.where(R0 >= 0, R0 * 2, -1))
    assert torch.equal(filters.ids_bitmap(idx.id_map, (np.flatnonzero(mask) * 2).tolist() + [1, 3]), allow)
    rr = torch.from_numpy(c["rr"]).to(dev)
    D1, R1 = ref_phase1(c["dmat"], mask, 1500)
    got = py_search3(c["codes"], c["x8"], c["norms"], c["qf"], c["qb"], 150, 1500, 450, rescore_row=rr, allow=allow)
    torch.cuda.synchronize()
    same_values(tuple(t.cpu().numpy() for t in got), ref_search3(dev, c, D1, R1, 150, 450))
    mode, q_t, mm_t, limit = deq = _deq(dev, c, "int8g")
    for k, bo in ((150, 10), (5, 2)):                            # K = 1500 and K = 10: one route for both
        D1, R1 = ref_phase1(c["dmat"], mask, k * bo)
        cnt, rows, dist, sc = ref_search2(dev, c, deq, D1, R1, k)
        for fn in (quant.search2, quant.vectordb_search):
            r, d, s = fn("int8g", c["codes"], q_t, c["qf"], c["qb"], k=k, binary_oversample=bo, limit=limit,
                         rescore_row=rr, allow=allow)
            torch.cuda.synchronize()
            same_values((r.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy()), (rows, dist, sc))
