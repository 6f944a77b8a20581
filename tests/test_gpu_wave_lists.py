"""GPU checks of the intermediate the wavefront Phase-I scans write: K1 (hamming_scan.hip, 128 code bytes) and
K1d (search_dim.hip, the other code sizes) leave u64[nq][nchunks][K] keys at workspace offset 0, and the merge
(select_topk) takes every list to be the exact top-min(K, rows) of its chunk, ascending in (dist, row),
KEY_NONE padded.  A list that breaks that contract without changing the merged top-K is invisible to the
parity tests; here every key of every list is compared with the reference, on inputs that drive the list
through every path of ``accept`` (tests/wave_scan_model.py restates it and counts, tests/test_wave_scan_model.py
asserts that each schedule reaches its path):

A  every kernel instance on random codes: 7 code sizes x both sides of every CAP step x the query counts that
   give 1 or 2 queries per wave, 1 to 8 waves per group, idle trailing waves and an odd last query;
B  every exit of the software pipeline (1, 2, 3, 4, 5+ tiles, odd and even, ragged) as the last chunk and as
   the only one, K below and above the chunk's rows (padded lists);
C  adversarial row order: every tile re-sorts; exact fill then overflow; overflow by one key; a tile partly
   accepted at the second ballot; a ramp at the chunk's end; rows that fall between the (K - 1)-th and the K-th
   key after the last cut; distance 2048 (the key's top bit); query pairs (q0, ~q0) so that one wave holds a
   list that re-sorts every tile and one that rejects every tile;
D  64 / 65 lists and K = 128 / 129 (the merge's LDS instances) with the top-K planted in one list, a threshold
   row in every list, and the single row of a 1-row chunk as the best;
E  the widest chunk (2^20 rows: local row 0xFFFFF) at 32 bytes and 1024 queries, final lists only.

The reference of a list: the chunk's rows sorted by (exact distance, row), cut, as dist << 40 | row.  Exact
distances come from an fp32 GEMM of 0/1 bit matrices (integers <= 2048); the whole call is compared with the C
restatement of FAISS hammings_knn_hc (oracle_knn), case E with one popcount per row.
"""
import numpy as np
import pytest
import torch

from tests import wave_scan_model as M
from tests.conftest import oracle_knn

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
PATTERN_KEY = int(np.array([PATTERN] * 8, np.uint8).view(np.int64)[0])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    return torch.device("cuda", 0)


def _bits(c):
    """u8[m, cb] -> f32[m, 8 cb] 0/1."""
    sh = torch.arange(7, -1, -1, device=c.device, dtype=torch.uint8)
    return ((c[:, :, None] >> sh) & 1).reshape(c.shape[0], -1).float()


def _dist(codes, qb, block=1 << 16):
    """Exact Hamming distances i64[nq, n]: pc(q) + pc(r) - 2 <q, r>, all integers in fp32."""
    qbits = _bits(qb)
    pcq = qbits.sum(1)
    out = torch.empty((qb.shape[0], codes.shape[0]), dtype=torch.int64, device=codes.device)
    for r0 in range(0, codes.shape[0], block):
        cb = _bits(codes[r0:r0 + block])
        out[:, r0:r0 + block] = (pcq[:, None] + cb.sum(1)[None, :] - 2.0 * (qbits @ cb.T)).long()
    return out


def chunk_lists(codes, qb, K):
    """Runs the wavefront scan alone on a workspace pre-filled with a pattern and checks what it left: all of
    u64[nq][nchunks][K] written (nchunks from the model) and nothing after it, every list equal to the reference.
    -> (lists i64[nq, nchunks, K], the model's plan)."""
    from vectorragquantization_amd import _native as N
    lib = N.load()
    dev = codes.device
    (n, cb), nq = codes.shape, qb.shape[0]
    p = M.plan(n, cb, nq, K)
    flags = N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_VALU
    assert lib.vrq_scan_kind(n, 8 * cb, nq, K, flags, None) == N.VRQ_SCAN_KIND_VALU
    nkeys = nq * p.nchunks * K
    need = lib.vrq_search3_dim_workspace_size(n, 8 * cb, nq, K)
    assert need >= 8 * nkeys
    ws = torch.full((max(need, 8 * nkeys) + 256,), PATTERN, dtype=torch.uint8, device=dev)
    N.check(lib.vrq_search3_dim_scan(N.ptr(codes), n, 8 * cb, N.ptr(qb), nq, K, flags, N.ptr(ws), ws.numel(),
                                     N.stream_handle(dev)), "vrq_search3_dim_scan")
    torch.cuda.synchronize()
    keys = ws[:8 * nkeys + 8].view(torch.int64)
    lists = keys[:nkeys].view(nq, p.nchunks, K)
    assert not (lists == PATTERN_KEY).any(), "a list entry was never written (more chunks planned than scanned?)"
    assert int(keys[nkeys]) == PATTERN_KEY, "the scan wrote past nq * nchunks * K keys"
    D = _dist(codes, qb)
    for c in range(p.nchunks):
        r0, r1 = c * p.chunk_rows, min(n, (c + 1) * p.chunk_rows)
        want = torch.full((nq, K), -1, dtype=torch.int64, device=dev)                    # KEY_NONE
        ref = torch.sort((D[:, r0:r1] << M.KEY_ROW_BITS) | torch.arange(r0, r1, device=dev)[None, :], dim=1).values
        m = min(K, r1 - r0)
        want[:, :m] = ref[:, :m]
        bad = torch.nonzero(lists[:, c] != want)
        assert bad.numel() == 0, (
            f"chunk {c} (rows {r0}..{r1}), K {K}, cb {cb}, nq {nq}: {bad.shape[0]} wrong keys; first: query "
            f"{int(bad[0, 0])} pos {int(bad[0, 1])} gpu {int(lists[bad[0, 0], c, bad[0, 1]]):#x} "
            f"want {int(want[bad[0, 0], bad[0, 1]]):#x}")
    return lists, p


def topk_call(codes, qb, K):
    """The whole Phase-I call through the wavefront scan -> (dist i32[nq, K], rows i64[nq, K]), NumPy:
    vrq_hamming_topk where the shape takes that scan by itself, else vrq_search3_dim with the scan forced."""
    from vectorragquantization_amd import _native as N
    lib = N.load()
    dev = codes.device
    (n, cb), nq = codes.shape, qb.shape[0]
    dist = torch.empty((nq, K), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, K), dtype=torch.int64, device=dev)
    st = N.stream_handle(dev)
    if lib.vrq_scan_kind(n, 8 * cb, nq, K, 0, None) == N.VRQ_SCAN_KIND_VALU:
        ws = torch.empty((lib.vrq_hamming_topk_workspace_size(n, cb, nq, K),), dtype=torch.uint8, device=dev)
        N.check(lib.vrq_hamming_topk(N.ptr(codes), n, cb, 0, N.ptr(qb), nq, K, N.ptr(dist), N.ptr(rows), N.ptr(ws),
                                     ws.numel(), st), "vrq_hamming_topk")
    else:
        flags = N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_VALU
        ws = torch.empty((lib.vrq_search3_dim_workspace_size(n, 8 * cb, nq, K),), dtype=torch.uint8, device=dev)
        cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
        N.check(lib.vrq_search3_dim(N.ptr(codes), 0, 0, 0, n, 8 * cb, 0, 0, N.ptr(qb), nq, K, K, K, flags, N.ptr(cnt),
                                    N.ptr(rows), N.ptr(dist), 0, 0, N.ptr(ws), ws.numel(), st), "vrq_search3_dim")
        torch.cuda.synchronize()
        assert K <= n and cnt.cpu().tolist() == [K] * nq
    torch.cuda.synchronize()
    return dist.cpu().numpy(), rows.cpu().numpy()


def check(codes_np, qb_np, K, oracle_lib, dev):
    """Every chunk list against the reference, then the merged call against the FAISS restatement."""
    codes, qb = torch.from_numpy(codes_np).to(dev), torch.from_numpy(qb_np).to(dev)
    lists, p = chunk_lists(codes, qb, K)
    D0, I0 = oracle_knn(oracle_lib, codes_np, qb_np, K)
    D1, I1 = topk_call(codes, qb, K)
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1), f"merged top-{K} differs ({p})"
    return lists, p


# ----------------------------------------------------------------------------- A: instance matrix
A_KS = (1, 192, 193, 448, 449, 960, 961, 1024)
A_NQS = (1, 2, 3, 5, 9, 17)


@pytest.mark.parametrize("cb", (32, 48, 64, 96, 128, 192, 256))
def test_instance_matrix_random_codes(dev, oracle_lib, cb):
    """Two full chunks and a ragged tail, the whole (K, nq) product (a few milliseconds a run): at 128 bytes every
    (CAP, QG, WPG) instance, at the other sizes (one wave per group) every CAP with full and half-empty waves."""
    rng = np.random.default_rng(100 + cb)
    cr = M.plan(1, cb, 1, 1).chunk_rows
    n = 2 * cr + 777
    codes = rng.integers(0, 256, (n, cb), dtype=np.uint8)
    q = rng.integers(0, 256, (17, cb), dtype=np.uint8)
    q[0] = codes[n - 1]                                   # exact hits: the ragged tile, a chunk's last row
    q[1] = codes[cr - 1]
    codes[cr + 5] = codes[5]                              # equal rows in two chunks
    seen = set()
    for K in A_KS:
        for nq in A_NQS:
            _, p = check(codes, q[:nq], K, oracle_lib, dev)
            assert (p.chunk_rows, p.nchunks) == (cr, 3)
            seen.add((p.cap, p.qg, p.wpg))
    caps = {256, 512, 1024, 2048}
    if cb == 128:
        assert seen == {(c, g, w) for c in caps for g, w in ((1, 1), (2, 1), (2, 2), (2, 4), (2, 8))}
    else:
        assert seen == {(c, 2 if cb <= 96 else 1, 1) for c in caps}


# ----------------------------------------------------------------------------- B: pipeline exits
B_TAILS = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 321)


@pytest.mark.parametrize("cb", (48, 128, 256))
def test_pipeline_exits(dev, oracle_lib, cb):
    """The last chunk's tile count picks the pipeline's exit: tails of 1..6 tiles, full and ragged, behind one
    full chunk and alone; at K = 1024 every tail list is padded."""
    rng = np.random.default_rng(200 + cb)
    cr = M.plan(1, cb, 3, 100).chunk_rows
    codes = rng.integers(0, 256, (cr + max(B_TAILS), cb), dtype=np.uint8)
    q = rng.integers(0, 256, (3, cb), dtype=np.uint8)
    for tail in B_TAILS:
        q[1] = codes[cr + tail - 1]                       # an exact hit on the tail's last row
        for K in (100, 1024):
            for sub in (codes[:cr + tail], codes[cr:cr + tail]):
                lists, p = check(sub, q, K, oracle_lib, dev)
                assert p.nchunks == (2 if sub.shape[0] > tail else 1)
                npad = (lists[:, -1] == -1).sum(dim=1)
                assert npad.tolist() == [max(K - tail, 0)] * 3


# ----------------------------------------------------------------------------- C: adversarial order
@pytest.mark.parametrize("cb", (32, 128, 256))
def test_adversarial_row_order(dev, oracle_lib, cb):
    """Each schedule of wave_scan_model.adversarial_cases as chunk 0, a second schedule as chunk 1 (its list
    starts from scratch: the state is per chunk), a short random tail; queries (q0, ~q0, ~q0, q0, q0), as a
    pair in one wave (two queries) and over several waves with an odd last one (five)."""
    dim = 8 * cb
    rng = np.random.default_rng(300 + cb)
    q0 = rng.integers(0, 256, cb, dtype=np.uint8)
    T = M.plan(1, cb, 2, 192).chunk_rows // 64
    cases = M.adversarial_cases(dim)
    by_k = {}
    for name, (K, sched) in cases.items():
        by_k.setdefault(K, []).append((name, sched))
    q = np.stack([q0, ~q0, ~q0, q0, q0])
    tail = rng.integers(0, 256, (100, cb), dtype=np.uint8)
    for K, group in by_k.items():
        chunks = [M.build_chunk(q0, sched(T), rng)[0] for _, sched in group]
        if len(chunks) == 1:
            chunks.append(chunks[0][::-1].copy())         # the same rows, ascending for q0
        codes = np.concatenate(chunks + [tail])
        for nq in (2, 5):
            _, p = check(codes, q[:nq], K, oracle_lib, dev)
            assert (p.chunk_rows, p.nchunks) == (64 * T, len(chunks) + 1)


# ----------------------------------------------------------------------------- D: merge boundaries
def _plant(codes, rows, q, dists, rng):
    codes[rows] = M.rows_at(q, np.asarray(dists), rng)


@pytest.mark.parametrize("cb,cr", ((128, 4096), (48, 10_944)))
def test_merge_boundaries_with_the_scan_forced(dev, oracle_lib, cb, cr):
    """64 and 65 lists (the last of one row) x K = 128 and 129: both sides of the merge's list-count and K
    instances.  One query per planting: (0) the whole top-K in the last full chunk; (1) K - 30 near rows
    scattered, then one row at the threshold distance T in every list: the cut takes 30 of them, in row
    order; (2) the last row of the corpus -- the single row of the 1-row chunk at 65 lists -- is the best."""
    rng = np.random.default_rng(400 + cb)
    dim = 8 * cb
    base = rng.integers(0, 256, (64 * cr + 1, cb), dtype=np.uint8)
    q = rng.integers(0, 256, (3, cb), dtype=np.uint8)
    for n, K in ((64 * cr, 128), (64 * cr + 1, 129)) + (((64 * cr, 129), (64 * cr + 1, 128)) if cb == 128 else ()):
        codes = base[:n].copy()
        nl = (n + cr - 1) // cr
        rows = 63 * cr + rng.choice(cr - 1, K + 10, replace=False)
        _plant(codes, rows, q[0], rng.integers(1, dim // 8, K + 10), rng)
        near = rng.permutation(np.setdiff1d(rng.choice(n - 1, 2 * K, replace=False), rows))[:K - 30]
        _plant(codes, near, q[1], rng.integers(2, 20, K - 30), rng)
        at_t = np.minimum(np.arange(nl) * cr + rng.integers(0, cr, nl), n - 1)
        at_t = np.setdiff1d(at_t, np.concatenate([rows, near, [n - 1]]))   # (the 1-row chunk serves planting 2)
        _plant(codes, at_t, q[1], np.full(at_t.shape[0], 30), rng)
        codes[n - 1] = q[2]
        lists, p = check(codes, q, K, oracle_lib, dev)
        assert (p.chunk_rows, p.nchunks) == (cr, nl)
        d = (lists >> M.KEY_ROW_BITS).cpu().numpy()
        assert (d[0, 63, :K] < dim // 8).all() and d[0, :63, 0].min() > dim // 8       # planting 0
        d1 = d[1][d[1] >= 0]                               # (KEY_NONE >> 40 is -1)
        assert at_t.shape[0] >= nl - 2 and (d1 <= 30).sum() == K - 30 + at_t.shape[0]
        assert d[2, nl - 1, 0] == 0
        if n % cr == 1:
            assert (lists[:, nl - 1, 1:] == -1).all()


# ----------------------------------------------------------------------------- E: widest chunk
def _popcount_rows(codes):
    """Popcount per row of u8[n, 32] device codes -> i64[n]."""
    x = codes.view(torch.int32)
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    x = ((x * 0x01010101) >> 24) & 0xFF
    return x.sum(1).long()


_WIDE = {}


def _wide_corpus(dev):
    """2^23 + 1 rows of 32 bytes generated on the device, extreme popcounts planted at the first and last local
    rows of the first and the last full chunk and in the lone row of chunk 8; popcounts; the queries."""
    if not _WIDE:
        n, cr = (1 << 23) + 1, 1 << 20
        g = torch.Generator(device=dev)
        g.manual_seed(77)
        codes = torch.randint(0, 256, (n, 32), generator=g, device=dev, dtype=torch.uint8)
        edge = torch.cat([torch.tensor([0]), torch.arange(cr - 64, cr)])
        for c in (0, 7):
            for i, r in enumerate((c * cr + edge).tolist()):
                codes[r] = 0
                nbytes = i % 5                             # popcount 0, 8, .., 32, or 256 - that
                codes[r, :nbytes] = 0xFF
                if (i + c) & 1:
                    codes[r] = ~codes[r]
        codes[n - 1] = 0
        codes[n - 1, 0] = 1                                # popcount 1: second best for the zero query
        qb = torch.zeros((1024, 32), dtype=torch.uint8, device=dev)
        qb[1::2] = 0xFF
        _WIDE.update(codes=codes, pc=_popcount_rows(codes), qb=qb)
    return _WIDE["codes"], _WIDE["pc"], _WIDE["qb"]


@pytest.mark.parametrize("n,K", (((1 << 23), 100), ((1 << 23) + 1, 100), ((1 << 23), 1024), ((1 << 23) + 1, 1024)))
def test_widest_chunk_local_row_bits(dev, n, K):
    """chunk_rows = 2^20, the width of the key's row field: 8 full chunks, and 9 with a 1-row chunk.  Queries
    alternate all-zeros and all-ones, so a row's distance is its popcount or 256 minus it."""
    from vectorragquantization_amd import _native as N
    lib = N.load()
    codes, pc, qb = _wide_corpus(dev)
    codes, pc, nq = codes[:n], pc[:n], qb.shape[0]
    p = M.plan(n, 32, nq, K)
    assert p.chunk_rows == 1 << 20 and p.nchunks == (n + (1 << 20) - 1) >> 20
    flags = N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_VALU
    ws = torch.empty((lib.vrq_search3_dim_workspace_size(n, 256, nq, K),), dtype=torch.uint8, device=dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, K), dtype=torch.int64, device=dev)
    dist = torch.empty((nq, K), dtype=torch.int32, device=dev)
    N.check(lib.vrq_search3_dim(N.ptr(codes), 0, 0, 0, n, 256, 0, 0, N.ptr(qb), nq, K, K, K, flags, N.ptr(cnt),
                                N.ptr(rows), N.ptr(dist), 0, 0, N.ptr(ws), ws.numel(), N.stream_handle(dev)),
            "vrq_search3_dim")
    torch.cuda.synchronize()
    assert (cnt == K).all()
    ar = torch.arange(n, device=dev)
    edge_rows = 0
    for parity, d in ((0, pc), (1, 256 - pc)):
        want = torch.topk((d << M.KEY_ROW_BITS) | ar, K, largest=False, sorted=True).values
        assert torch.equal(dist[parity::2].long(), (want >> M.KEY_ROW_BITS)[None, :].expand(nq // 2, K))
        assert torch.equal(rows[parity::2], (want & ((1 << M.KEY_ROW_BITS) - 1))[None, :].expand(nq // 2, K))
        local = (want & M.LOCAL_MASK)
        edge_rows += int(((local == 0) | (local >= (1 << 20) - 64)).sum())
    assert edge_rows >= 130                                 # all 2 x 65 planted edge rows are in the lists
