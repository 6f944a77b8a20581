"""CPU checks of tests/wave_scan_model.py, the restated model behind tests/test_gpu_wave_lists.py: the replay
of the wavefront scans' candidate list gives the exact top-K whatever the row order, every adversarial
schedule reaches the path it is named for (counted by the replay: these are the preconditions of the GPU
cases), the builders' rows sit at exactly the scheduled distances, and the plan reproduces the shapes the GPU
cases rely on -- against the library's own workspace sizes where the wavefront scan is the only route."""
import numpy as np
import pytest

from tests import wave_scan_model as M

# code bytes -> tiles of a full chunk of a small corpus (the plan's minimum chunk)
CASE_BYTES = (32, 128, 256)


def _tiles(cb):
    return M.plan(3 * M.plan(1, cb, 2, 192).chunk_rows, cb, 2, 192).chunk_rows // 64


def test_replay_is_exact_on_random_chunks():
    rng = np.random.default_rng(1)
    seen_resort = 0
    for i in range(200):
        K = int(rng.choice([1, 7, 100, 192, 193, 448, 449, 960, 961, 1024]))
        rows = int(rng.integers(1, 6000))
        dim = int(rng.choice([256, 1024, 2048]))
        spread = int(rng.choice([2, 16, dim // 2]))         # few distinct distances: ties; many: none
        d = np.clip(rng.integers(dim // 2 - spread, dim // 2 + spread + 1, rows), 0, dim)
        if i % 3 == 0:
            d = np.sort(d)[::-1]                            # descending: the worst order for the list
        r = M.replay(d, K, M.cap_for(K))
        assert np.array_equal(r.keys, M.reference_list(d, K)), (i, K, rows)
        assert r.keys.shape[0] == min(K, rows)
        assert np.array_equal(M.replay(d, K, M.cap_for(K), reballot=False).keys, r.keys)
        seen_resort += r.resorts > 0
    assert seen_resort > 50


@pytest.mark.parametrize("cb", CASE_BYTES)
def test_adversarial_schedules_reach_their_paths(cb):
    dim, T = cb * 8, _tiles(cb)
    assert T == (256 if cb == 32 else 64)
    for name, (K, sched) in M.adversarial_cases(dim).items():
        cap = M.cap_for(K)
        d = M.schedule_dists(sched(T), dim, np.random.default_rng(5))
        assert d.shape[0] == 64 * T
        r, ro = M.replay(d, K, cap), M.replay(dim - d, K, cap)      # q0 and ~q0
        assert np.array_equal(r.keys, M.reference_list(d, K)), name
        assert np.array_equal(ro.keys, M.reference_list(dim - d, K)), name
        fill = cap // 64
        kind = name.rsplit("_K", 1)[0]
        if kind in ("every_tile", "exact_fill", "top_bit"):
            assert r.resorts >= T - fill - 1 and r.rejected_tiles == 0, (name, r)
        if kind in ("exact_fill", "top_bit"):
            assert K == cap - 64 and r.exact_fills >= 1 and r.fill_then_sort >= T - fill - 1, (name, r)
        if kind == "by_one":
            assert r.overflow_by_one >= 3 and r.fill_then_sort >= r.overflow_by_one, (name, r)
        if kind == "partial":
            assert r.reballot_partial >= 2 and r.resorts >= T - fill - 1, (name, r)
        if kind == "late_ramp":
            assert r.rejected_tiles >= T - 20 - fill - 1 and r.resorts >= (20 * 64 - cap) // (cap - K), (name, r)
            assert ((r.keys & M.LOCAL_MASK) >= (T - 20) * 64).all(), name   # the list: rows of the ramp only
        if kind == "tau_gap":
            # the only case that tells a tau taken one key too low (cj[K - 2]) from the real one: on tie-heavy
            # rows the (K - 1)-th and K-th keys share a distance and no later row can fall between them
            assert r.resorts >= T - fill - 1
            assert not np.array_equal(M.replay(d, K, cap, tau_pos=K - 2).keys, r.keys), name
            assert int(r.keys[-1]) & M.LOCAL_MASK >= 64 * (T - 1)        # the K-th row: one of the last tile
        # without the second ballot the list takes rows that are not below the new tau; the next cut drops
        # them again: slower, never wrong -- no input can tell
        assert np.array_equal(M.replay(d, K, cap, reballot=False).keys, r.keys), name
        if kind == "top_bit":
            assert d[0] == 2048 and int(M.reference_list(d, 64 * T)[-1]) >= 1 << 31
        # the opposite regime: the list fills, is cut once or a few times, then whole tiles are rejected
        assert ro.resorts <= 4 and ro.reballot_changed >= 1 and ro.rejected_tiles >= T // 2, (name, ro)
        assert r.resorts >= 4 * ro.resorts, name


@pytest.mark.parametrize("cb", CASE_BYTES)
def test_builders_place_rows_at_the_scheduled_distances(cb):
    dim, rng = cb * 8, np.random.default_rng(cb)
    q0 = rng.integers(0, 256, cb, dtype=np.uint8)
    sched = M.sched_partial(12, dim, 192)
    codes, d = M.build_chunk(q0, sched, rng)
    assert codes.shape == (12 * 64, cb) and codes.dtype == np.uint8
    got = np.unpackbits(codes ^ q0[None, :], axis=1).sum(1)
    assert np.array_equal(got, d)
    assert np.array_equal(np.unpackbits(codes ^ ~q0[None, :], axis=1).sum(1), dim - d)
    for t, groups in enumerate(sched):
        want = sorted(sum(([dist] * m for m, dist in groups), []) + [dim] * (64 - sum(m for m, _ in groups)))
        assert sorted(d[64 * t:64 * t + 64].tolist()) == want
    full = codes[:64][d[:64] < dim]
    # tied rows, different codes (only 256 codes exist at distance 255 of a 256-bit query: some repeat)
    assert len({r.tobytes() for r in full}) > full.shape[0] // 2


def test_plan_shapes_of_the_gpu_cases():
    # merge boundaries with the scan forced, 128 bytes: 64 and 65 lists, the last of one row
    for K in (128, 129):
        p = M.plan(262_144, 128, 3, K)
        assert (p.chunk_rows, p.nchunks, p.cap) == (4096, 64, 256)
        p = M.plan(262_145, 128, 3, K)
        assert (p.chunk_rows, p.nchunks) == (4096, 65) and 262_145 - 64 * p.chunk_rows == 1
    # ... and at 48 bytes: the narrow codes' minimum chunk (4096 * 128 / 48 rows, up to a tile)
    p = M.plan(64 * 10_944 + 1, 48, 3, 129)
    assert (p.chunk_rows, p.nchunks, p.qg, p.wpg) == (10_944, 65, 2, 1)
    # the widest chunk: 2^20 rows, local row 0xFFFFF in every full chunk
    p = M.plan(1 << 23, 32, 1024, 100)
    assert (p.chunk_rows, p.nchunks, p.qg, p.wpg, p.nqg) == (1 << 20, 8, 2, 1, 512)
    p = M.plan((1 << 23) + 1, 32, 1024, 1024)
    assert (p.chunk_rows, p.nchunks, p.cap) == (1 << 20, 9, 2048)
    # at most 4096 lists (one wave per chunk at the target of 4096 waves), up to 2^32 rows at the clamp
    p = M.plan(100_000_000, 128, 1, 10)
    assert (p.chunk_rows, p.nchunks) == (24_448, 4091)
    p = M.plan(1 << 32, 128, 1, 10)
    assert (p.chunk_rows, p.nchunks) == (1 << 20, 4096)
    # queries per wave and waves per group of the 128-byte kernel, groups with idle trailing waves
    got = {nq: (M.plan(9000, 128, nq, 10).qg, M.plan(9000, 128, nq, 10).wpg, M.plan(9000, 128, nq, 10).nqg)
           for nq in (1, 2, 3, 5, 9, 17)}
    assert got == {1: (1, 1, 1), 2: (2, 1, 1), 3: (2, 2, 1), 5: (2, 4, 1), 9: (2, 8, 1), 17: (2, 8, 2)}
    assert [M.cap_for(K) for K in (1, 192, 193, 448, 449, 960, 961, 1024)] == [256, 256, 512, 512, 1024, 1024,
                                                                               2048, 2048]
    assert {cb: M.plan(1, cb, 1, 1).chunk_rows for cb in (32, 48, 64, 96, 128, 192, 256)} == \
        {32: 16_384, 48: 10_944, 64: 8192, 96: 5504, 128: 4096, 192: 4096, 256: 4096}


def test_plan_matches_the_library_workspace():
    """Where the wavefront scan is the only route (K > 128, or fewer than 65 536 rows) the call's workspace is
    its lists: nq * nchunks * K keys."""
    from vectorragquantization_amd import _native as N
    lib = N.load()
    rng = np.random.default_rng(3)
    shapes = [(262_145, 3, 129), (1 << 23, 1024, 1024), ((1 << 23) + 1, 1024, 129), (65_535, 1024, 100)]
    shapes += [(int(rng.integers(1, 3_000_000)), int(rng.integers(1, 300)), int(rng.integers(129, 1025)))
               for _ in range(40)]
    shapes += [(int(rng.integers(1, 65_536)), int(rng.integers(1, 2000)), int(rng.integers(1, 129)))
               for _ in range(40)]
    for cb in (32, 48, 64, 96, 128, 192, 256):
        for n, nq, K in shapes:
            p = M.plan(n, cb, nq, K)
            assert lib.vrq_hamming_topk_workspace_size(n, cb, nq, K) == 8 * nq * p.nchunks * K, (cb, n, nq, K)
