"""GPU checks of K1hm, the counting scan on the matrix cores, stage by stage through vrq_scan_batch with engine
MFMA forced: after COUNT every bin of every (query, chunk) histogram equals the NumPy model
(tests/batch_scan_model.py), after THRESHOLD the (T, c_lt) pairs do, after EMIT the K-lists equal the model and
engine VALU's lists word for word.  Every comparison is exact; no kernel appears in the model.

The base shape is n = 3 chunks + 37 rows of the plan (at least 3 chunks, a ragged last tile and a ragged last
n-block: asserted); the small shapes are those at which the kernels take another path."""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_scan_model as M

pytestmark = pytest.mark.gpu

DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
STAGES = (1, 2, 4)   # VRQ_LARGE_STAGE_COUNT, _THRESHOLD, _EMIT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _N():
    from vectorragquantization_amd import _native as N
    return N, N.load()


def plan(n, dim, nq, K, engine):
    N, lib = _N()
    info = (C.c_int64 * 10)()
    assert lib.vrq_scan_batch_plan(n, dim, nq, K, engine, info) == N.VRQ_OK
    return [int(v) for v in info]


def base_rows(dim, nq, K):
    N, _ = _N()
    rows = plan(3 * 4096 + 37, dim, nq, K, N.VRQ_LARGE_ENGINE_MFMA)[1]
    n = 3 * rows + 37
    p = plan(n, dim, nq, K, N.VRQ_LARGE_ENGINE_MFMA)
    assert p[1] == rows and p[2] >= 3 and n % 64 != 0 and n % 32 != 0
    return n, rows


def run(dev, codes, queries, K, words, engine, fill):
    """The three stages one at a time on a workspace prefilled with `fill`; returns the plan and, as NumPy arrays,
    the histograms of the last pass after COUNT, the (T, c_lt) pairs after THRESHOLD and the K-lists after EMIT."""
    N, lib = _N()
    n, cb = codes.shape
    nq, dim = queries.shape[0], cb * 8
    p = plan(n, dim, nq, K, engine)
    assert p[0] == (engine or _N()[1].vrq_large_engine(n, dim, nq, K, int(words is not None)))
    chunks, off_hist, off_tc, off_lists, need = p[2], p[6], p[7], p[8], p[9]
    ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
    c_t, q_t = torch.from_numpy(codes).to(dev), torch.from_numpy(queries).to(dev)
    a_t = None if words is None else torch.from_numpy(np.ascontiguousarray(words)).to(dev)
    out = [None, None, None]
    # more than one pass of 512 queries shares the histograms, so its stages cannot be issued apart: one call
    for st in (STAGES if nq <= 512 else (0,)):
        N.check(lib.vrq_scan_batch(N.ptr(c_t), n, dim, N.ptr(q_t), nq, K, st, N.ptr(a_t), N.ptr(ws), ws.numel(),
                                   N.stream_handle(dev), engine), "vrq_scan_batch")
        torch.cuda.synchronize()
        if st in (0, 1):
            qlast = nq - (nq - 1) // 512 * 512      # queries of the last pass: its histograms are what is left
            out[0] = (ws[off_hist:off_hist + qlast * chunks * (dim + 1) * 4].cpu().numpy().view(np.uint32)
                      .reshape(qlast, chunks, dim + 1).copy())
        if st in (0, 2):
            out[1] = ws[off_tc:off_tc + nq * 8].cpu().numpy().view(np.int32).reshape(nq, 2).copy()
        if st in (0, 4):
            out[2] = ws[off_lists:off_lists + nq * K * 8].cpu().numpy().view(np.uint64).reshape(nq, K).copy()
    return p, out


def check(dev, codes, queries, K, mask=None, tail=False, D=None):
    """Engine MFMA against the model after each stage, and against engine VALU's K-lists."""
    N, _ = _N()
    n, dim, nq = codes.shape[0], codes.shape[1] * 8, queries.shape[0]
    words = None if mask is None else M.pack(mask, tail)
    p, (hist, tc, lists) = run(dev, codes, queries, K, words, N.VRQ_LARGE_ENGINE_MFMA, 0xA5)
    D = M.distances(codes, queries) if D is None else D
    m_hist, m_tc, m_lists = M.model(D, np.ones(n, bool) if mask is None else mask, p[1], K, dim, mask is not None)
    qlast = hist.shape[0]
    assert np.array_equal(hist, m_hist[nq - qlast:])        # every bin of every (query, chunk)
    assert np.array_equal(tc, m_tc)
    assert np.array_equal(lists, m_lists)
    _, (_, v_tc, v_lists) = run(dev, codes, queries, K, words, N.VRQ_LARGE_ENGINE_VALU, 0x5A)
    assert np.array_equal(tc, v_tc) and np.array_equal(lists, v_lists)
    return p


_cases = {}


def base_case(dim, nq=33):
    """Random codes with bins 0 and dim planted, at the base shape of `dim`; distances computed once."""
    if (dim, nq) not in _cases:
        n, rows = base_rows(dim, nq, 100)
        codes, q = M.random_case(n, dim, nq, 100 * dim + nq)
        _cases[(dim, nq)] = (codes, q, M.distances(codes, q), rows)
    return _cases[(dim, nq)]


@pytest.mark.parametrize("dim", DIMS)
def test_every_dim_at_the_base_shape(dev, dim):
    codes, q, D, _ = base_case(dim)
    assert D[0].max() == dim and D[1].min() == 0       # bins dim and 0
    p = check(dev, codes, q, 100, D=D)
    assert p[2] >= 3


@pytest.mark.parametrize("n", [1, 31, 33, 64, 65])
@pytest.mark.parametrize("dim", [256, 384, 1024, 2048])
def test_small_corpora(dev, dim, n):
    codes, q = M.random_case(n, dim, 5, n + dim)
    check(dev, codes, q, 10)              # K > n at the small ones
    check(dev, codes, q, 1, mask=np.arange(n) % 2 == 0, tail=True)


@pytest.mark.parametrize("dim", [256, 768, 1024, 2048])
def test_query_counts(dev, dim):
    N, _ = _N()
    qpw = plan(65, dim, 512, 10, N.VRQ_LARGE_ENGINE_MFMA)[3]
    for nq in (1, 31, 33, qpw + 1, 513):     # a padded block, two blocks, a second pass of 512
        codes, q = M.random_case(65, dim, nq, nq + dim)
        check(dev, codes, q, 10)
    codes, q, D, _ = base_case(dim, qpw + 1)
    check(dev, codes, q, 100, D=D)
    check(dev, codes, q, 100, mask=M.masks(codes.shape[0], 64)["r50"], D=D)


@pytest.mark.parametrize("K", [1, 100, 1025, 8192])
@pytest.mark.parametrize("dim", [384, 1024])
def test_list_lengths(dev, dim, K):
    codes, q, D, _ = base_case(dim)
    check(dev, codes, q, K, D=D)
    check(dev, codes[:5000], q[:3], K, D=D[:3, :5000])     # K = 8192 > n


@pytest.mark.parametrize("dim", [256, 1024, 2048])
def test_ties_cut_inside_an_n_block_of_a_middle_chunk(dev, dim):
    nq, K = 33, 4000
    n, rows = base_rows(dim, nq, K)
    codes, q, _ = M.tie_case(n, dim, nq, rows, K, 3)
    check(dev, codes, q, K)
    check(dev, codes, q, K, mask=M.masks(n, rows)["r50"])


@pytest.mark.parametrize("mname", M.MASKS)
@pytest.mark.parametrize("dim", [256, 384, 1024, 2048])
def test_masks(dev, dim, mname):
    codes, q, D, rows = base_case(dim)
    mask = M.masks(codes.shape[0], rows)[mname]
    check(dev, codes, q, 1025, mask=mask, tail=mname in ("last", "r50", "highhalf"), D=D)   # r01: fewer than K allowed


@pytest.mark.parametrize("dim", [384, 1024])   # (at 2048 dims the histogram cap gives both engines the same chunks)
def test_auto_runs_the_engine_vrq_large_engine_names(dev, dim):
    """At 2.1M rows and 64 queries the two engines chunk differently (asserted), so the histograms that
    vrq_scan_batch(AUTO) leaves show which engine ran: their per-(query, chunk) totals are the allowed rows of the
    chunks of the plan of the engine vrq_large_engine names (another chunking leaves other totals, or unwritten
    words of the prefilled workspace)."""
    N, lib = _N()
    n, nq = 2_100_003, 64
    pv, pm = plan(n, dim, nq, 100, N.VRQ_LARGE_ENGINE_VALU), plan(n, dim, nq, 100, N.VRQ_LARGE_ENGINE_MFMA)
    assert pv[1] != pm[1] and pv[2] != pm[2]
    named = lib.vrq_large_engine(n, dim, nq, 100, 0)
    codes = np.zeros((n, dim // 8), np.uint8)
    q = np.random.default_rng(dim).integers(0, 256, (nq, dim // 8), dtype=np.uint8)
    mask = np.arange(n) % 5 != 0
    for words in (None, M.pack(mask)):
        assert lib.vrq_large_engine(n, dim, nq, 100, int(words is not None)) == named
        p, (hist, tc, lists) = run(dev, codes, q, 100, words, N.VRQ_LARGE_ENGINE_AUTO, 0x3C)
        assert p == plan(n, dim, nq, 100, named)
        rows = np.flatnonzero(mask) if words is not None else np.arange(n)
        want = np.bincount(rows // p[1], minlength=p[2])
        assert hist.shape[1] == p[2] and np.array_equal(hist.sum(2, dtype=np.int64), np.tile(want, (nq, 1)))


def test_more_rows_in_a_chunk_than_between_two_flushes(dev):
    """An all-equal corpus: every count of a query lands in one bin, one row more than the 16-bit bins hold
    between two flushes in a single chunk (dim 256, one query block)."""
    N, lib = _N()
    dim, nq, K = 256, 3, 10
    n = 1025 * 65536          # more rows than 1024 chunks of 65 535 hold: some chunk is flushed
    p = plan(n, dim, nq, K, N.VRQ_LARGE_ENGINE_MFMA)
    flush, rows, chunks = p[5], p[1], p[2]
    assert flush and rows >= flush + 1 and p[4] == 1
    codes = torch.zeros((n, dim // 8), dtype=torch.uint8, device=dev)
    q = torch.zeros((nq, dim // 8), dtype=torch.uint8, device=dev)
    q[1, 0] = 0x0F
    q[2] = 0xFF
    ws = torch.empty((p[9],), dtype=torch.uint8, device=dev)
    N.check(lib.vrq_scan_batch(N.ptr(codes), n, dim, N.ptr(q), nq, K, 0, None, N.ptr(ws), ws.numel(),
                               N.stream_handle(dev), N.VRQ_LARGE_ENGINE_MFMA), "vrq_scan_batch")
    torch.cuda.synchronize()
    hist = ws[p[6]:p[6] + nq * chunks * (dim + 1) * 4].cpu().numpy().view(np.uint32).reshape(nq, chunks, dim + 1)
    per_chunk = np.minimum(rows, n - rows * np.arange(chunks))
    for j, b in enumerate((0, 4, 256)):
        want = np.zeros((chunks, dim + 1), np.uint32)
        want[:, b] = per_chunk
        assert np.array_equal(hist[j], want)
    tc = ws[p[7]:p[7] + nq * 8].cpu().numpy().view(np.int32).reshape(nq, 2)
    assert tc.tolist() == [[0, 0], [4, 0], [256, 0]]
    lists = ws[p[8]:p[8] + nq * K * 8].cpu().numpy().view(np.uint64).reshape(nq, K)
    for j, b in enumerate((0, 4, 256)):
        assert lists[j].tolist() == [(b << 40) + r for r in range(K)]


@pytest.mark.parametrize("engine", ["valu", "mfma"])
def test_stages_issued_apart_over_two_passes_leave_what_one_call_leaves(dev, engine):
    """The pass loop of the counting-scan route, which both engines share: COUNT, THRESHOLD and EMIT as three calls
    leave the (T, c_lt) pairs and the K-lists of all 513 queries that one call with stages = 0 leaves on a second
    workspace.  513 queries are two passes, the second of one query; 70 000 rows at 384 dims are several chunks;
    every third row is allowed.  The histograms region holds one pass (run() above), so after the COUNT call its
    slot 0 holds the counts of query 512, not of query 0: query 512 is a copy of query 0 here, which makes the two
    the same words and the stages separable, while the pairs, chunk prefixes and lists of the two queries still
    live in their own slices (b0 = 0 and b0 = 512) and are all compared."""
    N, lib = _N()
    eng = {"valu": N.VRQ_LARGE_ENGINE_VALU, "mfma": N.VRQ_LARGE_ENGINE_MFMA}[engine]
    dim, n, nq, K = 384, 70_000, 513, 1025
    p = plan(n, dim, nq, K, eng)
    chunks, off_tc, off_lists, need = p[2], p[7], p[8], p[9]
    assert p[0] == eng and chunks > 1
    codes, q = M.random_case(n, dim, nq, 513)
    q[512] = q[0]
    c_t, q_t = torch.from_numpy(codes).to(dev), torch.from_numpy(q).to(dev)
    a_t = torch.from_numpy(M.pack(np.arange(n) % 3 == 0)).to(dev)
    left = []
    for fill, stages in ((0xA5, STAGES), (0x5A, (0,))):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        for st in stages:
            N.check(lib.vrq_scan_batch(N.ptr(c_t), n, dim, N.ptr(q_t), nq, K, st, N.ptr(a_t), N.ptr(ws), ws.numel(),
                                       N.stream_handle(dev), eng), "vrq_scan_batch")
        torch.cuda.synchronize()
        left.append((ws[off_tc:off_tc + nq * 8].cpu().numpy().view(np.int32).reshape(nq, 2),
                     ws[off_lists:off_lists + nq * K * 8].cpu().numpy().view(np.uint64).reshape(nq, K)))
    (tc3, lists3), (tc1, lists1) = left
    assert np.array_equal(tc3, tc1) and np.array_equal(lists3, lists1)
    # not vacuous: every list is full of allowed rows (nothing of the prefill is left), cut among ties at T
    rows = lists1 & np.uint64((1 << 40) - 1)
    assert (rows < n).all() and (rows % 3 == 0).all() and ((lists1 >> np.uint64(40)) <= tc1[:, :1].astype(np.uint64)).all()
    assert (tc1[:, 1] < K).all() and np.array_equal(lists1[512], lists1[0]) and not np.array_equal(lists1[1], lists1[0])
