"""CPU checks of tests/batch_scan_model.py: the model against a brute-force restatement, and each planted input
of tests/test_gpu_batch_scan.py against the property it is named for."""
import ctypes as C

import numpy as np
import pytest

import batch_scan_model as M
from vectorragquantization_amd import _native as N

MFMA = N.VRQ_LARGE_ENGINE_MFMA


def plan(n, dim, nq, K):
    info = (C.c_int64 * 10)()
    assert N.load().vrq_scan_batch_plan(n, dim, nq, K, MFMA, info) == N.VRQ_OK
    return [int(v) for v in info]


def base_rows(dim, nq, K):
    """n = 3 chunks + 37 rows of the plan that n itself gets."""
    rows = plan(3 * 4096 + 37, dim, nq, K)[1]
    n = 3 * rows + 37
    assert plan(n, dim, nq, K)[1] == rows
    return n, rows


@pytest.mark.parametrize("filtered", [False, True])
def test_model_against_brute_force(filtered):
    rng = np.random.default_rng(5)
    n, nq, dim, chunk_rows = 300, 4, 16, 64
    D = rng.integers(0, dim + 1, (nq, n))
    mask = rng.random(n) < 0.6 if filtered else np.ones(n, bool)
    for K in (1, 7, 150, 400):
        hist, tc, lists = M.model(D, mask, chunk_rows, K, dim, filtered)
        assert hist.shape == (nq, 5, dim + 1) and hist.sum() == nq * mask.sum()
        for q in range(nq):
            for c in range(5):
                for b in range(dim + 1):
                    rows = [r for r in range(c * 64, min(n, c * 64 + 64)) if mask[r] and D[q, r] == b]
                    assert hist[q, c, b] == len(rows)
            order = sorted((int(D[q, r]), r) for r in range(n) if mask[r])[:K]
            T, c_lt = tc[q]
            assert order and T == order[-1][0] and c_lt == sum(1 for d, _ in order if d < T)
            got = lists[q][lists[q] != M.KEY_NONE]
            assert sorted((int(k) >> 40, int(k) & ((1 << 40) - 1)) for k in got) == order
            lt = [int(k) & ((1 << 40) - 1) for k in got[:c_lt]]
            eq = [int(k) & ((1 << 40) - 1) for k in got[c_lt:]]
            assert lt == sorted(lt) and eq == sorted(eq)      # each part in row order
            assert np.all(lists[q][len(order):] == M.KEY_NONE)


def test_model_of_an_empty_filter():
    D = np.zeros((2, 70), np.int64)
    hist, tc, lists = M.model(D, np.zeros(70, bool), 64, 5, 32, True)
    assert hist.sum() == 0 and np.all(tc == (32, 0)) and np.all(lists == M.KEY_NONE)


def test_distances_and_pack():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 256, (9, 4), dtype=np.uint8)
    q = rng.integers(0, 256, (2, 4), dtype=np.uint8)
    want = [[int(np.unpackbits(c[r] ^ q[i]).sum()) for r in range(9)] for i in range(2)]
    assert M.distances(c, q).tolist() == want
    w = M.pack(np.arange(70) % 2 == 0, tail=True).view(np.uint64)
    assert w[0] == 0x5555555555555555 and w[1] == (0x15 | (0xFFFFFFFFFFFFFFFF << 6) & 0xFFFFFFFFFFFFFFFF)


@pytest.mark.parametrize("dim", [256, 384, 512, 768, 1024, 1536, 2048])
def test_base_shape_has_three_chunks_and_ragged_blocks(dim):
    n, rows = base_rows(dim, 33, 100)
    assert plan(n, dim, 33, 100)[2] >= 3 and n % 64 != 0 and n % 32 != 0
    m = M.masks(n, rows)
    assert set(m) == set(M.MASKS)
    lo = np.flatnonzero(m["range"])
    assert lo[0] // rows == 1 and lo[-1] // rows == 2 and lo[0] % 64 and (lo[-1] + 1) % 64
    words = M.pack(m["lowhalf"]).view(np.uint64)
    assert np.all(words[:-1] == 0x00000000FFFFFFFF)
    words = M.pack(m["highhalf"]).view(np.uint64)
    assert np.all(words[:-1] == 0xFFFFFFFF00000000)
    assert 0 < m["r01"].sum() < 1000           # fewer allowed rows than K = 1025
    assert np.all(M.pack(m["altwords"]).view(np.uint64)[1::2] == 0)


def test_random_case_reaches_bin_zero_and_bin_dim():
    codes, q = M.random_case(500, 256, 3, 9)
    D = M.distances(codes, q)
    assert D[0].max() == 256 and D[1].min() == 0


@pytest.mark.parametrize("dim", [256, 1024, 2048])
def test_tie_case_cuts_inside_an_n_block_of_a_middle_chunk(dim):
    nq, K = 33, 4000
    n, rows = base_rows(dim, nq, K)
    codes, q, flip = M.tie_case(n, dim, nq, rows, K, 3)
    assert len(np.unique(codes, axis=0)) == 2
    D = M.distances(codes, q)
    hist, tc, lists = M.model(D, np.ones(n, bool), rows, K, dim, False)
    assert np.array_equal(tc[:, 0], flip) and np.all(tc[:, 1] == 0)     # every listed row sits at T
    at_T = np.flatnonzero(D[0] == tc[0, 0])
    assert np.array_equal(at_T, np.flatnonzero(np.arange(n) % 3 != 0)) and at_T.shape[0] > K
    last, nxt = int(at_T[K - 1]), int(at_T[K])
    chunks = -(-n // rows)
    assert 0 < last // rows < chunks - 1                                 # a middle chunk
    assert last // 32 == nxt // 32 and last % 32 != 31                  # strictly inside an n-block
    assert int(lists[0, K - 1]) & ((1 << 40) - 1) == last
