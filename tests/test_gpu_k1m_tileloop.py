"""K1m's tile loop around its steady/general switch, against the exact lists and the FAISS restatement.

The loop carries its ring slots and its LDS-DMA source as scalar state stepped once per tile, and splits
its tiles into steady ones (tile t + 4 exists and is whole: uniform DMA form, constant end-of-tile wait)
and the rest (the chunk's last four tiles, the refill of a partial last tile: clamped rows, counted
waits).  A wrong slot, source or wait shows as a stale or missing 64-row tile, i.e. as wrong or missing
list entries for rows of particular tiles of a chunk -- so rows at distance 3 from chosen queries are
planted in exactly those tiles, in both 32-row n-blocks, and every case requires

* every (query, chunk) list to be exactly {dist < tau(q)} with exact distances (check_scan_lists), and
* the final top-K of the planted queries plus a spread sample to equal ``hammings_knn_hc``'s.

Short chunks run the MB = 2 instance (nq = 256; the dense sample pass too, T = 4 tiles per sample chunk):
chunks of 4 tiles (never steady), 5 (one steady tile), 6 and 8 tiles, with last chunks of one 1-row tile,
one whole tile plus a 16-row tile, and four whole tiles plus 7 rows.  The MB = 4 instance runs chunks of
several hundred tiles (the rings wrap many times) with plants at the head, around the first ring wraps and
in the last six tiles of the first, a middle and the ragged last chunk.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_k1m_edges import N_BIG, _assert_k1m4, _check, _flip, _phase1, _sel
from tests.test_gpu_lists import check_scan_lists

pytestmark = pytest.mark.gpu

NPK = 4                     # packed ring depth of K1m: tile t + NPK is issued in iteration t
K = 100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    return torch.device("cuda", 0)


def _plan_mfma(n, nq):
    """The plan check_scan_lists runs with (the matrix-core scan forced, as there)."""
    from vectorragquantization_amd import _native as N
    info = np.zeros(12, np.int64)
    N.check(N.load().vrq_scan_plan(n, 1024, nq, K, N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_MFMA,
                                   info.ctypes.data), "plan")
    return info


def _phase1_mfma(codes_t, qb, dev):
    """_phase1 with the matrix-core scan forced (the library's own choice at 64K rows is another scan)."""
    from vectorragquantization_amd import _native as N
    from vectorragquantization_amd.enhanced import search3
    nq = qb.shape[0]
    x8 = torch.empty((1, 1024), dtype=torch.int8, device=dev)
    norms = torch.empty((1,), dtype=torch.float64, device=dev)
    qf = torch.zeros((nq, 1024), dtype=torch.float32, device=dev)
    q_t = torch.from_numpy(np.ascontiguousarray(qb)).to(dev)
    cnt, rows, dist, _, _ = search3(codes_t, x8, norms, qf, q_t, K, K, K,
                                    N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_MFMA)
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), dist.cpu().numpy(), rows.cpu().numpy()


def _plant(rng, codes, qb, n, tiles, queries):
    """One row at distance 3 from each of `queries` in both n-blocks of every (chunk_row0, tile) of `tiles`
    (rows past the corpus end are skipped: partial tiles).  -> planted row count per query."""
    count = {q: 0 for q in queries}
    for row0, t in tiles:
        for nblk in (0, 1):
            for i, q in enumerate(queries):
                r = row0 + t * 64 + nblk * 32 + 9 * i        # rows 0, 9, 18, 27 of the n-block: one per query
                if r < n:
                    codes[r] = _flip(rng, qb[q:q + 1], 3)[0]
                    count[q] += 1
    return count


def _verify(dev, oracle_lib, codes, qb, planted_q, counts, phase1, want_plan):
    codes_t = torch.from_numpy(codes).to(dev)
    q_t = torch.from_numpy(np.ascontiguousarray(qb)).to(dev)
    info = check_scan_lists(codes_t, q_t, K, allow_overflow=False)
    assert tuple(int(info[i]) for i in (0, 1, 2, 3)) == want_plan
    c, D1, I1 = phase1(codes_t, qb)
    assert np.array_equal(c, np.full(qb.shape[0], K))
    _check(oracle_lib, codes, qb, K, D1, I1, _sel(planted_q, qb.shape[0]))
    for q in planted_q:                                   # every planted row reached its query's top-K
        assert (D1[q] == 3).sum() == min(counts[q], K)


# n -> (chunk_rows, nchunks) of the MB = 2 plan at nq = 256: 4-tile chunks (never steady); 5-tile chunks (one
# steady tile) with a last chunk of 4 whole tiles + 7 rows / of one 1-row tile / of a whole tile + 16 rows;
# 6-tile chunks; 8-tile chunks with a 1-row last chunk
SHORT = {65_536: (256, 256), 65_543: (320, 205), 65_921: (320, 207), 66_000: (320, 207), 98_304: (384, 256),
         114_689: (512, 225)}


@pytest.mark.parametrize("n", sorted(SHORT))
def test_k1m2_short_chunks(dev, oracle_lib, n):
    nq = 256
    cr, nch = SHORT[n]
    info = _plan_mfma(n, nq)
    assert tuple(int(info[i]) for i in (0, 1, 2, 3)) == (0, 2, cr, nch), "K1m MB = 2 with the chunking this case is for"
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    qb = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    nt = cr // 64
    last0 = (nch - 1) * cr
    nt_last = (n - last0 + 63) // 64
    tiles = [(0, 0), (0, nt - 1)] + [(last0, t) for t in range(nt_last)]
    queries = [3, 70, 200, 255]                           # one per wave of the 256-query block
    counts = _plant(rng, codes, qb, n, tiles, queries)
    assert counts[queries[0]] >= 4 + nt_last              # (row 0 of every tile exists, also in a 1-row tile)
    _verify(dev, oracle_lib, codes, qb, queries, counts, lambda c, q: _phase1_mfma(c, q, dev), (0, 2, cr, nch))


@pytest.fixture(scope="module")
def big():
    """The uniform corpus and queries of the MB = 4 cases, generated once; the tests plant into copies."""
    rng = np.random.default_rng(77)
    return (rng.integers(0, 256, (N_BIG, 128), dtype=np.uint8), rng.integers(0, 256, (1024, 128), dtype=np.uint8))


def _big_plan():
    info = _assert_k1m4(N_BIG, 1024, K)
    cr, nch = int(info[2]), int(info[3])
    assert cr % 64 == 0 and cr // 64 >= 200 and nch >= 3, "chunks of several hundred whole tiles"
    assert (N_BIG - (nch - 1) * cr) % 64 != 0, "ragged last chunk"
    assert tuple(int(x) for x in _plan_mfma(N_BIG, 1024)[:4]) == (0, 4, cr, nch)
    return cr, nch


def test_k1m4_steady_drain_seam(dev, oracle_lib, big):
    """Plants in tiles 0, 1, 3, 4, 5, 11, 12, 13 and in the last six tiles of chunk 0, a middle chunk and the
    ragged last chunk, for a query of the first and of the last wave of each 512-query block."""
    cr, nch = _big_plan()
    rng = np.random.default_rng(78)
    codes, qb = big[0].copy(), big[1].copy()
    tiles = []
    for ch in (0, nch // 2, nch - 1):
        row0 = ch * cr
        nt = (min(N_BIG, row0 + cr) - row0 + 63) // 64
        assert nt > 32
        tiles += [(row0, t) for t in (0, 1, 3, 4, 5, 11, 12, 13)] + [(row0, t) for t in range(nt - 6, nt)]
    queries = [5, 500, 517, 1020]
    counts = _plant(rng, codes, qb, N_BIG, tiles, queries)
    assert min(counts.values()) >= 3 * 14 * 2 - 2         # (the ragged chunk's partial last tile holds fewer rows)
    _verify(dev, oracle_lib, codes, qb, queries, counts, lambda c, q: _phase1(c, q, K, dev), (0, 4, cr, nch))


def test_k1m4_sync_flush_on_last_steady_tile(dev, oracle_lib, big):
    """More than 64 hits staged by one wave in its last steady iteration t = nt - NPK - 1 of a middle chunk:
    the synchronous flush (entries past the 64 of the asynchronous one) right before the loop switches to
    its general forms.  A tile has 64 rows, so one query cannot give more than 64 hits per iteration: two
    queries of one wave, 2 bits apart, each get all 64 rows that iteration tests (n-block 1 of tile t - 1
    and n-block 0 of tile t) at distance 3 / <= 5 -- 128 hits; a query of another query block gets the same
    rows of the next iteration (the first general one)."""
    cr, nch = _big_plan()
    info = _plan_mfma(N_BIG, 1024)
    assert int(info[4]) >= 96, "list capacity holds the 64 planted rows of a (query, chunk) list"
    rng = np.random.default_rng(79)
    codes, qb = big[0].copy(), big[1].copy()
    qb[201] = _flip(rng, qb[200:201], 2)[0]               # queries 200, 201: the same wave (128..255)
    row0 = (nch // 2) * cr
    t = cr // 64 - NPK - 1
    w0 = row0 + (t - 1) * 64 + 32
    codes[w0:w0 + 64] = _flip(rng, np.broadcast_to(qb[200:201], (64, 128)), 3)
    codes[w0 + 64:w0 + 128] = _flip(rng, np.broadcast_to(qb[900:901], (64, 128)), 3)
    planted = [200, 201, 900]
    codes_t = torch.from_numpy(codes).to(dev)
    q_t = torch.from_numpy(np.ascontiguousarray(qb)).to(dev)
    info = check_scan_lists(codes_t, q_t, K, allow_overflow=False)
    assert tuple(int(info[i]) for i in (0, 1, 2, 3)) == (0, 4, cr, nch)
    c, D1, I1 = _phase1(codes_t, qb, K, dev)
    assert np.array_equal(c, np.full(1024, K))
    _check(oracle_lib, codes, qb, K, D1, I1, _sel(planted, 1024))
    assert (D1[200] == 3).sum() == 64 and (D1[201] <= 5).sum() == 64 and (D1[900] == 3).sum() == 64
