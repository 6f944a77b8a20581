"""K1m's tile loop is two loops -- a steady one (tiles whose refill exists and is whole) and a tail -- and its
first n-block has no `t == 0` case: exact-distance plants at the places where the two loops, the first n-block
and the partial last tile meet, every list entry read back (check_scan_lists of test_gpu_lists.py) and the
top-K compared with the FAISS restatement (oracle_knn).

Geometry comes from vrq_scan_plan: a chunk of `cr` rows is ntiles = ceil(rows / 64) tiles, nwhole = rows // 64
of them whole, and the steady loop runs nsteady = max(nwhole - 4, 0) iterations; the last chunk of the corpus
holds what is left.  MB = 2 (nq = 200) cases, (chunk tiles / last chunk rows -> its tiles):
  n =  65 601: 5 / 1   -> 1 tile of 1 row (tail loop alone)      n =  65 664: 5 / 64  -> 1 whole tile
  n =  82 303: 6 / 127 -> 2 tiles, the last of 63 rows           n =  82 175: 6 / 383 -> 6 tiles, 63-row last
  n = 131 584: 9 / 256 -> 4 tiles (tail, empty steady loop)      n = 131 393: 9 / 65  -> 2 tiles, 1-row last
so chunks of 1, 2, 4, 5, 6 and 9 tiles occur, with 0, 1, 2 and 5 steady iterations.  MB = 4: n = 4 200 007,
nq = 1024 (513-tile chunks, a last chunk of 474 tiles + 7 rows).

The background is uniform random (distances 512 +- 16 sigma-wise; the builder verifies on the CPU, with the
reference alone, that every background row of a planted query lies at least one above its farthest plant), so
no list overflows and a planted query's top-K begins with exactly its plants."""
import numpy as np
import pytest
import torch

from tests.conftest import oracle_knn
from tests.test_gpu_k1m_edges import _flip, _phase1, _plan
from tests.test_gpu_lists import check_scan_lists, scan_paths

pytestmark = pytest.mark.gpu

RT, NPK, K = 64, 4, 100
# n -> (chunk tiles, last chunk rows) the plan must give at nq = 200
MB2_CASES = {65_601: (5, 1), 65_664: (5, 64), 82_303: (6, 127), 82_175: (6, 383), 131_584: (9, 256), 131_393: (9, 65)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    return torch.device("cuda", 0)


def _geometry(n, nq):
    info = _plan(n, nq, K)
    cr, nch = int(info[2]), int(info[3])
    assert cr % RT == 0 and (nch - 1) * cr < n <= nch * cr
    return (int(info[0]), int(info[1])), cr, nch


def _chunk_sites(row0, rows):
    """Rows of the chunk [row0, row0 + rows) at the places the loop split touches."""
    ntiles, nwhole = (rows + RT - 1) // RT, rows // RT
    nsteady = max(nwhole - NPK, 0)
    s = [row0 + min(5, rows - 1)]                      # rows 0-31 of the first tile: the former t == 0 n-block
    if rows > 40:
        s.append(row0 + 40)                            # rows 32-63 of the first tile
    if nsteady >= 1:
        s.append(row0 + (nsteady - 1) * RT + 37)       # last tile of the steady loop
    if ntiles > nsteady and nsteady * RT + 9 < rows:
        s.append(row0 + nsteady * RT + 9)              # first tile of the tail loop
    if rows % RT and ntiles - 1 - NPK >= 0:
        s.append(row0 + (ntiles - 1 - NPK) * RT + 50)  # the tile whose refill is the partial tile
    s.append(row0 + rows - 1)                          # last row of the chunk
    return sorted(set(s))


def _build(n, nq, cr, nch, seed):
    """Uniform corpus and queries; query i < len(sites) has one plant, at site i and distance 3 + i % 8; query
    len(sites) has a plant at EVERY site.  -> codes, qb, {query: [(row, dist)]}"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    qb = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    mid = nch // 2
    sites = _chunk_sites(mid * cr, cr) + _chunk_sites((nch - 1) * cr, n - (nch - 1) * cr)
    assert sites[-1] == n - 1                          # the last row of the corpus
    # the all-sites query's plants take other rows of the same tiles (one row holds one plant)
    alt = [r + 1 if (r + 1) % RT and r + 1 < n else r - 1 for r in sites[:-1]]
    assert not set(alt) & set(sites) and len(set(alt)) == len(alt)
    plants, qall = {}, len(sites)
    for i, r in enumerate(sites):
        d = 3 + i % 8
        codes[r] = _flip(rng, qb[i:i + 1], d)[0]
        plants[i] = [(r, d)]
    plants[qall] = []
    for i, r in enumerate(alt):
        d = 3 + (i + 3) % 8
        codes[r] = _flip(rng, qb[qall:qall + 1], d)[0]
        plants[qall].append((r, d))
    return codes, qb, plants


def _run_case(dev, oracle_lib, n, nq, inst, seed):
    kind, cr, nch = _geometry(n, nq)
    assert kind == inst, "shape does not run the K1m instance under test"
    codes, qb, plants = _build(n, nq, cr, nch, seed)
    qsel = np.unique(np.concatenate([np.fromiter(plants, np.int64), np.linspace(0, nq - 1, 24).round().astype(np.int64)]))
    D0, I0 = oracle_knn(oracle_lib, codes, qb[qsel], K, threads=16)
    pos = {int(q): i for i, q in enumerate(qsel)}
    for q, pl in plants.items():                       # the reference alone: plants first, background >= +1
        pl = sorted(pl, key=lambda x: (x[1], x[0]))
        got = list(zip(I0[pos[q]][:len(pl)].tolist(), D0[pos[q]][:len(pl)].tolist()))
        assert got == pl, (q, got, pl)
        assert D0[pos[q]][len(pl)] >= max(d for _, d in pl) + 1
    codes_t, qb_t = torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev)
    info = check_scan_lists(codes_t, qb_t, K)          # every entry exact, every list complete, none overflowed
    assert (int(info[0]), int(info[1])) == inst
    ovf, _, _, _ = scan_paths(codes_t, qb_t, K)
    assert not ovf.any()
    cnt, D1, I1 = _phase1(codes_t, qb, K, dev)
    assert np.array_equal(cnt, np.full(nq, K))
    assert np.array_equal(D0, D1[qsel]) and np.array_equal(I0, I1[qsel])


@pytest.mark.parametrize("n", sorted(MB2_CASES))
def test_k1m2_loop_split_plants(dev, oracle_lib, n):
    kind, cr, nch = _geometry(n, 200)
    assert (cr // RT, n - (nch - 1) * cr) == MB2_CASES[n], "the plan's chunk geometry moved: choose n again"
    _run_case(dev, oracle_lib, n, 200, (0, 2), 4000 + n % 997)


def test_k1m2_cases_cover_the_chunk_shapes():
    tiles = set()
    for n, (ct, last) in MB2_CASES.items():
        tiles |= {ct, (last + RT - 1) // RT}
    assert {1, 2, 4, 5, 6, 9} <= tiles
    assert {last % RT for _, last in MB2_CASES.values()} >= {1, 63}


def test_k1m4_loop_split_plants(dev, oracle_lib):
    _run_case(dev, oracle_lib, 4_200_007, 1024, (0, 4), 4242)


def test_k1m2_all_ties_at_the_ceiling(dev, oracle_lib):
    """All-zero corpus, all-ones queries: every distance is 1024 and every threshold at its ceiling.  The last
    chunk is one tile + one row (the planner takes no corpus that small as a whole: n = 131 393 ends in a
    65-row chunk).  Nothing listed twice or lost: the K-list is rows 0 .. K-1 at distance 1024."""
    n, nq = 131_393, 200
    kind, cr, nch = _geometry(n, nq)
    assert kind == (0, 2) and n - (nch - 1) * cr == RT + 1
    codes = np.zeros((n, 128), np.uint8)
    qb = np.full((nq, 128), 255, np.uint8)
    codes_t, qb_t = torch.from_numpy(codes).to(dev), torch.from_numpy(qb).to(dev)
    check_scan_lists(codes_t, qb_t, K, allow_overflow=True)
    cnt, D1, I1 = _phase1(codes_t, qb, K, dev)
    D0, I0 = oracle_knn(oracle_lib, codes, qb[:8], K, threads=16)
    assert np.array_equal(cnt, np.full(nq, K))
    assert (D1 == 1024).all() and (I1 == np.arange(K)[None, :]).all()
    assert np.array_equal(D0, D1[:8]) and np.array_equal(I0, I1[:8])
