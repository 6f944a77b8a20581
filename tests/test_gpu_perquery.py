"""GPU checks of the per-query filters (vrq_*_perquery: a set of bitmaps and one set id per query, on both
engines of the counting scan).  Every comparison is exact.  The corpus, the masks and the references are
tests/test_gpu_filtered.py's (12 325 rows: at least 3 chunks, a ragged tile, a partial last word); extra random
queries are made here.  Reference distances are that module's dist_matrix (torch xor + popcount table), and
ref_phase1 is applied per query with the query's own mask -- no kernel under test appears in a reference.  The
defining rule is checked against one *_batch call per distinct set over that set's queries.

Sets: r50, range, r01, zeros, altwords, packed with set_words = words + 3; the three spare words of every set
are all-ones (a wrong stride shows) and the bits past n are set.  query_set patterns: all one set; q % 5
(neighbouring accumulator slots differ, and so do the lane halves, slots s and s + 4); sorted runs; one odd
query in a uniform block; and one with -1 (unfiltered), nsets and -2 (no row)."""
import numpy as np
import pytest
import torch

import test_gpu_batch_search as B
import test_gpu_filtered as F

pytestmark = pytest.mark.gpu

DIMS = (256, 384, 1024, 2048)
SETS = ("r50", "range", "r01", "zeros", "altwords")
NSETS = len(SETS)
SPARE = 3
PATTERNS = ("one", "mod5", "runs", "odd", "special")
ENGINES = ("valu", "mfma")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def engine_of(name):
    N, _ = F._N()
    return {"auto": N.VRQ_LARGE_ENGINE_AUTO, "valu": N.VRQ_LARGE_ENGINE_VALU, "mfma": N.VRQ_LARGE_ENGINE_MFMA}[name]


def set_words(c):
    """int64 [NSETS, words + SPARE]: every set's words with the tail bits set, then all-ones spare words."""
    w = (c["n"] + 63) // 64
    a = np.full((NSETS, w + SPARE), -1, np.int64)
    for s, name in enumerate(SETS):
        a[s, :w] = F.pack(c["masks"][name], True)
    return a


def pattern(name, nq):
    q = np.arange(nq)
    if name == "one":
        ids = np.zeros(nq, np.int64)
    elif name == "mod5":
        ids = q % 5
    elif name == "runs":
        ids = (q * NSETS) // nq
    elif name == "odd":
        ids = np.full(nq, 2)
        ids[nq // 2] = 0
    else:
        ids = np.array([-1, 0, NSETS, 3, -2, 1, -1, 4, 2, 1 << 20, -(1 << 31)])[q % 11]
    return ids.astype(np.int32)


def mask_of(c, sid):
    if sid == -1:
        return np.ones(c["n"], bool)
    if sid < 0 or sid >= NSETS:
        return np.zeros(c["n"], bool)
    return c["masks"][SETS[sid]]


_full = {}
NQ_MAX = 520


def batch(dev, dim, nq):
    """The corpus with nq <= 520 queries: its own 17 first, then random ones; the distance matrix computed once."""
    if dim not in _full:
        c = F.corpus(dev, dim)
        rng = np.random.default_rng(dim + 7)
        qf = rng.standard_normal((NQ_MAX, dim)).astype(np.float32)
        qf[:F.NQ] = c["qf"].cpu().numpy()
        qb = np.packbits(qf > 0, axis=1)
        qb[:F.NQ] = c["qb"].cpu().numpy()
        d = dict(c)
        d["qf"], d["qb"] = torch.from_numpy(qf).to(dev), torch.from_numpy(qb).to(dev)
        d["dmat"] = F.dist_matrix(c["codes"], d["qb"])
        assert torch.equal(d["dmat"][:F.NQ], c["dmat"])
        _full[dim] = d
    return F.sub(_full[dim], nq)


def pick(c, idx):
    """The corpus with the queries idx."""
    d = dict(c)
    t = torch.from_numpy(np.asarray(idx)).to(c["qb"].device)
    d["qf"], d["qb"], d["dmat"] = c["qf"][t].contiguous(), c["qb"][t].contiguous(), c["dmat"][t]
    return d


def ref_phase1(c, qs, K):
    """F.ref_phase1 per query with the query's own mask (one call per distinct set id)."""
    nq = qs.shape[0]
    D = np.empty((nq, K), np.int32)
    R = np.empty((nq, K), np.int64)
    for sid in np.unique(qs):
        idx = np.flatnonzero(qs == sid)
        D[idx], R[idx] = F.ref_phase1(c["dmat"][torch.from_numpy(idx).to(c["dmat"].device)], mask_of(c, int(sid)), K)
    return D, R


def tail(dev, c, qs):
    a = torch.from_numpy(set_words(c)).to(dev)
    q = torch.from_numpy(np.ascontiguousarray(qs)).to(dev)
    return a, q


def hamming_pq(dev, c, k, qs, engine, row_offset=0):
    N, lib = F._N()
    n, cb = c["codes"].shape
    nq = c["qb"].shape[0]
    D = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    R = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    ws = F._ws(lib, "vrq_hamming_topk_batch", n, cb, nq, k, dev, fill=0xC3)
    a, q = tail(dev, c, qs)
    N.check(lib.vrq_hamming_topk_perquery(N.ptr(c["codes"]), n, cb, row_offset, N.ptr(c["qb"]), nq, k, N.ptr(a),
                                          N.ptr(D), N.ptr(R), N.ptr(ws), ws.numel(), N.stream_handle(dev),
                                          engine_of(engine), NSETS, a.shape[1], N.ptr(q)), "hamming_perquery")
    torch.cuda.synchronize()
    return D.cpu().numpy(), R.cpu().numpy()


def search3_pq(dev, c, k, K, K3, qs, engine, flags=0, row_offset=0):
    N, lib = F._N()
    nq = c["qf"].shape[0]
    kout = K if flags & N.VRQ_SEARCH_PHASE1_ONLY else k
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, kout), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, kout), -7, dtype=torch.int32, device=dev)
    s2 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    s3 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    ws = F._ws(lib, "vrq_search3_batch", c["n"], c["dim"], nq, K, dev, fill=0xC3)
    rr = torch.from_numpy(c["rr"]).to(dev)
    a, q = tail(dev, c, qs)
    N.check(lib.vrq_search3_perquery(N.ptr(c["codes"]), N.ptr(c["x8"]), N.ptr(c["norms"]), N.ptr(rr), c["n"], c["dim"],
                                     row_offset, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, K3, flags, N.ptr(a),
                                     N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), N.ptr(ws),
                                     ws.numel(), N.stream_handle(dev), engine_of(engine), NSETS, a.shape[1],
                                     N.ptr(q)), "search3_perquery")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (cnt, rows, dist, s2, s3))


def search2_pq(dev, c, deq, k, K, qs, engine, row_offset=0):
    N, lib = F._N()
    nq = c["qf"].shape[0]
    mode, q_t, mm_t, limit = deq
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    sc = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    ws = F._ws(lib, "vrq_search2_batch", c["n"], c["dim"], nq, K, dev, fill=0xC3)
    rr = torch.from_numpy(c["rr"]).to(dev)
    a, q = tail(dev, c, qs)
    N.check(lib.vrq_search2_perquery(mode, N.ptr(c["codes"]), N.ptr(q_t), N.ptr(mm_t), float(limit), N.ptr(rr),
                                     c["n"], c["dim"], row_offset, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, 0,
                                     N.ptr(a), N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(sc), N.ptr(ws),
                                     ws.numel(), N.stream_handle(dev), engine_of(engine), NSETS, a.shape[1],
                                     N.ptr(q)), "search2_perquery")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (cnt, rows, dist, sc))


def words_for(c, sid):
    """The bitmap a *_batch call takes for set id sid: None for -1 (unfiltered), an all-zero one for an id that
    names no set."""
    w = (c["n"] + 63) // 64
    return None if sid == -1 else set_words(c)[sid, :w] if 0 <= sid < NSETS else np.zeros(w, np.int64)


def per_set(qs, got, call):
    """`got` (a tuple of [nq, ...] arrays) equals, set by set, call(idx, set id) -- the *_batch call over that
    set's queries with words_for(set id) -- and the rows of an id that names no set have count 0 and are all
    padding (rows -1, dist INT32_MAX; the score arrays are what the all-zero bitmap leaves)."""
    for sid in np.unique(qs):
        idx = np.flatnonzero(qs == sid)
        mine = tuple(g[idx] for g in got)
        F.same(mine, call(idx, int(sid)))
        if sid != -1 and not 0 <= sid < NSETS:
            for g in mine:
                if g.dtype == np.int64:
                    assert (g == -1).all()
                elif g.dtype == np.int32:
                    assert (g == (0 if g.ndim == 1 else F.INT32_MAX)).all()


# ----------------------------------------------------------------------------- Phase I
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nq,K", ((1, 8192), (17, 1500), (17, 8192), (37, 1500), (70, 10), (520, 10)))
@pytest.mark.parametrize("dim", DIMS)
def test_phase1_against_reference_and_the_batch_calls(dev, dim, nq, K, engine):
    c = batch(dev, dim, nq)
    e = engine_of(engine)
    for pname in PATTERNS:
        qs = pattern(pname, nq)
        got = hamming_pq(dev, c, K, qs, engine, row_offset=3)
        D0, R0 = ref_phase1(c, qs, K)
        assert np.array_equal(got[0], D0), pname
        assert np.array_equal(got[1], np.where(R0 >= 0, R0 + 3, -1)), pname
        if pname == "one":       # one set for all: the *_batch call with that bitmap, on every array
            F.same(got, B.hamming_batch(dev, c["codes"], c["qb"], K, words_for(c, 0), e, row_offset=3))
        if pname in ("mod5", "special", "odd") and nq <= 70:
            per_set(qs, got, lambda idx, sid: B.hamming_batch(dev, c["codes"], pick(c, idx)["qb"], K,
                                                              words_for(c, sid), e, row_offset=3))
        if pname == "special":   # the unfiltered rows equal the *_large call
            idx = np.flatnonzero(qs == -1)
            F.same(tuple(g[idx] for g in got), F.hamming(dev, c["codes"], pick(c, idx)["qb"], K, row_offset=3))


def test_the_second_pass_reads_its_own_set_ids(dev):
    """520 queries: queries 512 .. 519 belong to the second pass, whose set ids start at query_set + 512."""
    c = batch(dev, 384, 520)
    qs = np.zeros(520, np.int32)
    qs[512:] = [1, 2, -1, 3, NSETS, 4, 0, 1]
    for engine in ENGINES:
        D, R = hamming_pq(dev, c, 10, qs, engine)
        D0, R0 = ref_phase1(c, qs, 10)
        assert np.array_equal(D, D0) and np.array_equal(R, R0)


# ----------------------------------------------------------------------------- the fused searches
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("dim", DIMS)
def test_search3(dev, dim, engine):
    N, _ = F._N()
    c = batch(dev, dim, F.NQ)
    e = engine_of(engine)
    for (K, k, K3), pname, off in (((1500, 150, 450), "mod5", 1000), ((10, 10, 30), "special", 0),
                                    ((8192, 300, 8192), "special", 7), ((1500, 150, 450), "odd", 0)):
        qs = pattern(pname, F.NQ)
        for flags in (0, N.VRQ_SEARCH_PHASE1_ONLY):
            got = search3_pq(dev, c, k, K, K3, qs, engine, flags, off)
            per_set(qs, got, lambda idx, sid: B.search3_batch(dev, pick(c, idx), k, K, K3, words_for(c, sid), e,
                                                              flags, off))
        if K == 1500 and pname == "mod5":   # ... and the NumPy reference over stand-alone scores
            D1, R1 = ref_phase1(c, qs, K)
            F.same_values(got[:3], (np.minimum((R1 >= 0).sum(1), K).astype(np.int32), np.where(R1 >= 0, R1 + off, -1), D1))
            full = search3_pq(dev, c, k, K, K3, qs, engine, 0, off)
            F.same_values(full, F.ref_search3(dev, c, D1, R1, k, K3, off))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("mode", ("int8g", "f32", "sbin"))
@pytest.mark.parametrize("dim", DIMS)
def test_search2(dev, dim, mode, engine):
    c = batch(dev, dim, F.NQ)
    e = engine_of(engine)
    deq = F._deq(dev, c, mode)
    for (K, k), pname, off in (((1500, 150), "mod5", 0), ((10, 10), "special", 0), ((1500, 150), "special", 1000)):
        qs = pattern(pname, F.NQ)
        got = search2_pq(dev, c, deq, k, K, qs, engine, off)
        if off == 0:
            per_set(qs, got, lambda idx, sid: B.search2_batch(dev, pick(c, idx), deq, k, K, words_for(c, sid), e))
        D1, R1 = ref_phase1(c, qs, K)
        cnt, rows, dist, sc = F.ref_search2(dev, c, deq, D1, R1, k)
        F.same_values(got, (cnt, np.where(rows >= 0, rows + off, -1), dist, sc))


# ----------------------------------------------------------------------------- the scan and its workspace
def scan_pq(dev, c, K, qs, engine, stages, ws):
    N, lib = F._N()
    a, q = tail(dev, c, qs)
    N.check(lib.vrq_scan_perquery(N.ptr(c["codes"]), c["n"], c["dim"], N.ptr(c["qb"]), c["qb"].shape[0], K, stages,
                                  N.ptr(a), N.ptr(ws), ws.numel(), N.stream_handle(dev), engine_of(engine), NSETS,
                                  a.shape[1], N.ptr(q)), "vrq_scan_perquery")
    torch.cuda.synchronize()


def plan(c, nq, K, engine):
    N, lib = F._N()
    info = np.zeros(10, np.int64)
    assert lib.vrq_scan_batch_plan(c["n"], c["dim"], nq, K, engine_of(engine), info.ctypes.data) == N.VRQ_OK
    return [int(x) for x in info]


@pytest.mark.parametrize("nq", (37, 520))
@pytest.mark.parametrize("dim", DIMS)
def test_scan_stages_engines_and_histogram_totals(dev, dim, nq):
    N, lib = F._N()
    c = batch(dev, dim, nq)
    K = 1500 if nq == 37 else 10
    qs = pattern("special", nq) if nq == 37 else np.concatenate([pattern("mod5", 512), pattern("special", 8)])
    allowed = np.array([mask_of(c, int(s)).sum() for s in qs])
    D0, R0 = ref_phase1(c, qs, K)
    want = np.sort(np.where(R0 >= 0, (D0.astype(np.int64) << 40) | R0, -1).view(np.uint64), axis=1)
    out = {}
    for engine in ENGINES:
        eng, rows, chunks, qpw, nqb, flush, off_hist, off_tc, off_lists, nbytes = plan(c, nq, K, engine)
        ws1 = F._ws(lib, "vrq_scan_batch", c["n"], dim, nq, K, dev, fill=0xFF)
        ws2 = F._ws(lib, "vrq_scan_batch", c["n"], dim, nq, K, dev, fill=0x00)
        scan_pq(dev, c, K, qs, engine, 0, ws1)
        if nq <= 512:   # stage by stage (the histograms hold one pass, so only a single pass can be replayed)
            for bit in (N.VRQ_LARGE_STAGE_COUNT, N.VRQ_LARGE_STAGE_THRESHOLD, N.VRQ_LARGE_STAGE_EMIT):
                scan_pq(dev, c, K, qs, engine, bit, ws2)
        else:
            scan_pq(dev, c, K, qs, engine, 0, ws2)
        get = lambda ws, off, cnt, dt: ws[off:off + cnt * np.dtype(dt).itemsize].cpu().numpy().view(dt)
        tc1, tc2 = (get(w, off_tc, nq * 2, np.int32).reshape(nq, 2) for w in (ws1, ws2))
        l1, l2 = (get(w, off_lists, nq * K, np.int64).reshape(nq, K) for w in (ws1, ws2))
        assert np.array_equal(tc1, tc2) and np.array_equal(l1, l2)
        assert np.array_equal(np.sort(l1.view(np.uint64), axis=1), want)
        # the histograms of the last pass: a query's total is its number of allowed rows
        b0 = (nq - 1) // 512 * 512
        h = get(ws1, off_hist, (nq - b0) * chunks * (dim + 1), np.uint32).reshape(nq - b0, chunks * (dim + 1))
        assert np.array_equal(h.sum(1, dtype=np.int64), allowed[b0:])
        out[engine] = (tc1, l1)
    assert np.array_equal(out["valu"][0], out["mfma"][0]) and np.array_equal(out["valu"][1], out["mfma"][1])


# ----------------------------------------------------------------------------- Python
def _np(ts):
    return tuple(t.cpu().numpy() for t in ts)


def test_python_wrappers_equal_the_per_set_calls(dev):
    from vectorragquantization_amd import filters, quant
    from vectorragquantization_amd.enhanced import search3 as py_search3
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    N, lib = F._N()
    dim = 384
    c = batch(dev, dim, F.NQ)
    qs = pattern("special", F.NQ)
    qs[qs > NSETS] = NSETS
    qs[qs < -2] = -2
    masks = torch.from_numpy(np.stack([c["masks"][s] for s in SETS])).to(dev)
    allow = filters.row_bitmaps(masks)
    assert np.array_equal(allow.cpu().numpy(), np.stack([F.pack(c["masks"][s]) for s in SETS]))
    q_t = torch.from_numpy(qs).to(dev)
    rr = torch.from_numpy(c["rr"]).to(dev)
    idx_ = BinaryIndexIDMap2(dim, device=dev)
    idx_.add_with_ids(c["codes"], np.arange(c["n"]) * 2)
    deq_mode, dq, mm, limit = F._deq(dev, c, "int8g")

    def one(sid):
        return None if sid == -1 else allow[sid] if 0 <= sid < NSETS else torch.zeros_like(allow[0])

    for engine in ("valu", "mfma", None):
        for K in (10, 2000):
            got = _np(idx_.search_device(c["qb"], K, allow=allow, engine=engine, query_set=q_t))
            per = lambda i, sid: _np(idx_.search_device(pick(c, i)["qb"], K, allow=one(sid), engine=engine or "auto"))
            for sid in np.unique(qs):
                i = np.flatnonzero(qs == sid)
                F.same(tuple(g[i] for g in got), per(i, int(sid)))
        got = _np(py_search3(c["codes"], c["x8"], c["norms"], c["qf"], c["qb"], 150, 1500, 450, rescore_row=rr,
                             allow=allow, engine=engine, query_set=q_t))
        for sid in np.unique(qs):
            i = np.flatnonzero(qs == sid)
            p = pick(c, i)
            F.same(tuple(g[i] for g in got), _np(py_search3(c["codes"], c["x8"], c["norms"], p["qf"], p["qb"], 150, 1500,
                                                            450, rescore_row=rr, allow=one(int(sid)),
                                                            engine=engine or "auto")))
        for fn in (quant.search2, quant.vectordb_search):
            got = _np(fn("int8g", c["codes"], dq, c["qf"], c["qb"], k=150, binary_oversample=10, limit=limit,
                         rescore_row=rr, allow=allow, engine=engine, query_set=q_t))
            for sid in np.unique(qs):
                i = np.flatnonzero(qs == sid)
                p = pick(c, i)
                F.same(tuple(g[i] for g in got), _np(fn("int8g", c["codes"], dq, p["qf"], p["qb"], k=150,
                                                        binary_oversample=10, limit=limit, rescore_row=rr,
                                                        allow=one(int(sid)), engine=engine or "auto")))


@pytest.mark.parametrize("dim", [384, 1024])   # AUTO names K1h at 384 dims and K1hm at 1024 for 64 queries
def test_python_auto_runs_the_engine_vrq_large_engine_names(dev, dim):
    """enhanced.search3 with engine=None and engine="auto", on a workspace the test owns.  At 2.1M rows and 64
    queries the two engines chunk differently (asserted), so the histograms the call leaves show which engine
    ran: the per-(query, chunk) totals are the query's allowed rows in the chunks of the plan of the engine
    vrq_large_engine names (another chunking leaves other totals, or unwritten words of the prefilled workspace)."""
    from vectorragquantization_amd import filters
    from vectorragquantization_amd.enhanced import search3 as py_search3
    N, lib = F._N()
    n, nq, K = 2_100_003, 64, 100
    c = dict(n=n, dim=dim)
    pv, pm = plan(c, nq, K, "valu"), plan(c, nq, K, "mfma")
    assert pv[1] != pm[1] and pv[2] != pm[2]
    named = lib.vrq_large_engine(n, dim, nq, K, 1)
    assert named == (N.VRQ_LARGE_ENGINE_MFMA if dim == 1024 else N.VRQ_LARGE_ENGINE_VALU)
    p = pm if named == N.VRQ_LARGE_ENGINE_MFMA else pv
    chunk_rows, chunks, off_hist = p[1], p[2], p[6]
    codes = torch.zeros((n, dim // 8), dtype=torch.uint8, device=dev)
    qb = torch.from_numpy(np.random.default_rng(dim).integers(0, 256, (nq, dim // 8), dtype=np.uint8)).to(dev)
    qf = torch.zeros((nq, dim), device=dev)
    none = torch.zeros((0,), device=dev)
    mask = np.arange(n) % 5 != 0
    allow = filters.row_bitmaps(torch.from_numpy(np.stack([mask, ~mask])).to(dev))
    qs = (np.arange(nq) % 3 - 1).astype(np.int32)               # -1, 0, 1, -1, ...
    want = np.stack([np.bincount(np.flatnonzero(m) // chunk_rows, minlength=chunks)
                     for m in (np.ones(n, bool), mask, ~mask)])[qs + 1]
    for engine in (None, "auto"):
        ws = F._ws(lib, "vrq_search3_batch", n, dim, nq, K, dev, fill=0x3C)
        py_search3(codes, none, none, qf, qb, 10, K, 30, flags=N.VRQ_SEARCH_PHASE1_ONLY, workspace=ws, allow=allow,
                   engine=engine, query_set=torch.from_numpy(qs).to(dev))
        torch.cuda.synchronize()
        hist = ws[off_hist:off_hist + nq * chunks * (dim + 1) * 4].cpu().numpy().view(np.uint32)
        assert np.array_equal(hist.reshape(nq, chunks, dim + 1).sum(2, dtype=np.int64), want), engine


N_DOCS, NQ_DOCS = 600, 7


def _docs(d, seed):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((16, d)) / np.sqrt(d)
    X = (C[rng.integers(0, 16, N_DOCS)] + (0.5 / np.sqrt(d)) * rng.standard_normal((N_DOCS, d))).astype(np.float32)
    Q = (X[rng.integers(0, N_DOCS, NQ_DOCS)] + (0.1 / np.sqrt(d)) * rng.standard_normal((NQ_DOCS, d))).astype(np.float32)
    ids = (rng.permutation(5000)[:N_DOCS] + 10).astype(np.int64)
    A = np.sort(rng.choice(ids, 220, replace=False)).tolist()
    Bs = np.sort(rng.choice(ids, 40, replace=False)).tolist()
    # None, two real sets (one of them twice, reordered), an empty one, unknown ids only
    entries = [A, None, Bs, list(reversed(A)), [], [7, 9_999_999], None]
    return X, Q, ids, entries


def _bits(x):
    x = x.cpu().numpy()
    return x.view(np.int64) if x.dtype == np.float64 else x


def _per_query(search, entries, fields):
    """search(sel, **kw) over the queries sel: allowed_ids_per_query for the batch equals one allowed_ids call per
    query, bit for bit, and an empty / unknown collection finds nothing."""
    with pytest.raises(Exception, match="exclusive"):
        search(slice(None), allowed_ids=[1], allowed_ids_per_query=entries)
    with pytest.raises(Exception, match="entries"):
        search(slice(None), allowed_ids_per_query=entries[:-1])
    for engine in (None, "valu", "mfma"):
        kw = {} if engine is None else {"engine": engine}
        got = fields(search(slice(None), allowed_ids_per_query=entries, **kw))
        for q, e in enumerate(entries):
            want = fields(search(slice(q, q + 1), allowed_ids=e, engine=engine or "auto"))
            for g, w in zip(got, want):
                assert np.array_equal(_bits(g[q:q + 1]), _bits(w)), (engine, q)
        ids = got[0].cpu().numpy()
        assert (ids[4] == -1).all() and (ids[5] == -1).all() and (ids[0] != -1).any() and (ids[1] != -1).any()
        assert np.isin(ids[2][ids[2] != -1], entries[2]).all()


def test_enhanced_class(tmp_path, dev):
    from vectorragquantization_amd.embed import SyntheticCohereProvider
    from vectorragquantization_amd.enhanced import CohereEnhancedVectorDB
    from vectorragquantization_amd.quant import encode
    d = 384
    X, Q, ids, entries = _docs(d, 11)
    e, eq = encode("cohere", X, 0.1, dev), encode("cohere", Q, 0.1, dev)
    db = CohereEnhancedVectorDB(str(tmp_path / "db"), embedding_dim=d, provider=SyntheticCohereProvider(dim=d, device=dev),
                                device=dev)
    db.add_vectors(ids, e["q"], e["codes"], [f"doc {i}" for i in ids])
    qf, qb = torch.from_numpy(Q).to(dev), eq["codes"]
    _per_query(lambda sel, **kw: db.search_vectors(qf[sel], qb[sel], 30, 10, 3, **kw), entries,
               lambda r: (r.doc_id, r.count, r.row, r.hamming, r.binary, r.cosine))


@pytest.mark.parametrize("cls", ("VectorDBInt8Global", "CohereVectorDBInt8"))
def test_vectordb_classes(tmp_path, dev, cls):
    from vectorragquantization_amd import vectordb
    from vectorragquantization_amd.embed import TableProvider
    d = 1024 if cls == "CohereVectorDBInt8" else 384
    X, Q, ids, entries = _docs(d, 12)
    if cls == "CohereVectorDBInt8":
        X, Q = np.clip(X * 2000, -127, 127).astype(np.int8), np.clip(Q * 2000, -127, 127).astype(np.int8)
    db = getattr(vectordb, cls)(str(tmp_path / "db"), embedding_dim=d, provider=TableProvider({}), device=dev)
    db.add_vectors(ids, X, [f"doc {i}" for i in ids])
    _per_query(lambda sel, **kw: db.search_vectors(Q[sel], 30, 10, **kw), entries, lambda r: r)


def test_binary_class(tmp_path, dev):
    from vectorragquantization_amd.binary import CohereVectorDBBinary
    from vectorragquantization_amd.embed import TableProvider
    d = 384
    X, Q, ids, entries = _docs(d, 13)
    db = CohereVectorDBBinary(str(tmp_path / "db"), embedding_dim=d, provider=TableProvider({}), device=dev)
    db.add_vectors(ids, X, [f"doc {i}" for i in ids])
    _per_query(lambda sel, **kw: db.search_vectors(Q[sel], 30, 10, **kw), entries, lambda r: r)
