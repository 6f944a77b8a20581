"""A NumPy restatement of what the wavefront Phase-I scans K1 (hamming_scan.hip) and K1d (search_dim.hip)
do per (query, chunk), and builders of corpora whose row ORDER drives their candidate list through the
paths that random rows never reach.  Test infrastructure only (tests/test_wave_scan_model.py checks it
without a GPU, tests/test_gpu_wave_lists.py uses it on one).

* ``plan`` restates ``scan_plan``: how a call shape is cut into chunks and query groups.
* ``replay`` restates ``accept``: rows arrive in 64-row tiles; a row is appended to an unsorted list of
  capacity CAP iff its key ``dist << 20 | local row`` is below the running threshold tau; a tile that would
  overflow the list first sorts it, cuts it to K, lowers tau to the K-th key and ballots again.  It counts
  how often each of those things happened, so that a test can state which path its input reaches.
* the builders turn a per-tile schedule of (row count, distance) groups into code rows at exactly those
  distances from a query q0.  A distance that decreases from tile to tile makes every scheduled row pass
  whatever tau is; the other rows of a tile are ``~q0`` (distance dim, the maximum).  Seen from ``~q0`` the
  same rows are an ascending ramp behind rows at distance 0: the list fills once and then rejects every tile.
"""
from dataclasses import dataclass

import numpy as np

WAVE = 64
LOCAL_BITS = 20                      # wave_scan.h
LOCAL_MASK = (1 << LOCAL_BITS) - 1
KEY_ROW_BITS = 40                    # vrq_internal.h
KEY_NONE = (1 << 64) - 1
TARGET_WAVES = 4096                  # vrq_scan.h kTargetWaves
MIN_CHUNK_ROWS = 4096                # vrq_scan.h kMinChunkRows
MAX_LISTS = 4096                     # lists the merge takes per query
DIM_CODE_BYTES = (32, 48, 64, 96, 192, 256)
TAU_NONE = 0xFFFFFFFF


# ----------------------------------------------------------------------------- plan
def cap_for(K):
    c = 256
    while c < K + 64:
        c <<= 1
    return c


@dataclass(frozen=True)
class Plan:
    cap: int
    qg: int
    wpg: int
    nqg: int
    chunk_rows: int
    nchunks: int


def plan(n, cb, nq, K):
    """scan_plan (hamming_scan.hip) for n rows of cb code bytes, nq queries, K candidates."""
    assert n >= 1 and nq >= 1 and 1 <= K <= 1024 and (cb == 128 or cb in DIM_CODE_BYTES)
    qg = (2 if cb <= 96 else 1) if cb != 128 else (2 if nq >= 2 else 1)
    waves_needed = (nq + qg - 1) // qg
    wpg = 1
    while cb == 128 and wpg < 8 and wpg < waves_needed:
        wpg <<= 1
    per_group = qg * wpg
    nqg = (nq + per_group - 1) // per_group
    want = max(TARGET_WAVES // (nqg * wpg), 1)
    cr = (n + want - 1) // want
    min_rows = MIN_CHUNK_ROWS * 128 // cb if cb < 128 else MIN_CHUNK_ROWS
    cr = max(cr, min_rows)
    cr = (cr + 63) & ~63
    if (n + cr - 1) // cr > MAX_LISTS:
        cr = ((n + MAX_LISTS - 1) // MAX_LISTS + 63) & ~63
    cr = min(cr, 1 << LOCAL_BITS)
    assert (n + cr - 1) // cr <= MAX_LISTS, "n > 2^32 rows"
    return Plan(cap_for(K), qg, wpg, nqg, cr, (n + cr - 1) // cr)


# ----------------------------------------------------------------------------- replay
@dataclass
class Replay:
    keys: np.ndarray          # the final list: sorted u32 keys dist << 20 | local, min(K, rows) of them
    tiles: int
    resorts: int              # overflows: sort + cut + new tau + second ballot
    exact_fills: int          # tiles that ended with cnt == CAP exactly
    fill_then_sort: int       # ... whose next accepting tile found the list full and re-sorted
    overflow_by_one: int      # overflows with cnt + nnew == CAP + 1
    reballot_changed: int     # overflows whose second ballot accepted fewer rows than the first
    reballot_partial: int     # ... but not none
    rejected_tiles: int       # tiles of which no row passed the first ballot


def replay(dists_of_chunk, K, cap, tau_pos=None, reballot=True):
    """Replays ``accept`` over the rows of one chunk for one query (dists_of_chunk: their distances in row
    order) and the final sort + cut.  ``tau_pos`` (default K - 1: the K-th key) and ``reballot`` restate two
    ways of getting ``accept`` wrong, for the tests that show which inputs tell them from the real thing."""
    d = np.asarray(dists_of_chunk, dtype=np.int64)
    nrows = d.shape[0]
    assert 1 <= nrows <= 1 << LOCAL_BITS and K + 64 <= cap
    keys = ((d << LOCAL_BITS) | np.arange(nrows, dtype=np.int64))
    buf = np.empty(cap, np.int64)
    cnt, tau = 0, TAU_NONE
    r = Replay(None, (nrows + 63) // 64, 0, 0, 0, 0, 0, 0, 0)
    full = False
    for t in range(r.tiles):
        kt = keys[t * 64:t * 64 + 64]
        acc = kt < tau
        nnew = int(acc.sum())
        if nnew == 0:
            r.rejected_tiles += 1
            continue
        if cnt + nnew > cap:
            r.resorts += 1
            r.fill_then_sort += full
            r.overflow_by_one += cnt + nnew == cap + 1
            buf[:cnt] = np.sort(buf[:cnt])
            cnt = min(cnt, K)
            if cnt >= K:
                tau = int(buf[K - 1 if tau_pos is None else tau_pos])
            if reballot:
                acc = kt < tau
            n2 = int(acc.sum())
            r.reballot_changed += n2 != nnew
            r.reballot_partial += 0 < n2 < nnew
            nnew = n2
        assert cnt + nnew <= cap, "the list overflowed its capacity"
        buf[cnt:cnt + nnew] = kt[acc]
        cnt += nnew
        full = cnt == cap
        r.exact_fills += full
    r.keys = np.sort(buf[:cnt])[:min(cnt, K)]
    return r


def global_keys(keys, row0):
    """The u64 keys the kernels write for a final list of chunk keys: dist << 40 | shard row."""
    k = np.asarray(keys, dtype=np.uint64)
    return ((k >> np.uint64(LOCAL_BITS)) << np.uint64(KEY_ROW_BITS)) | (np.uint64(row0) + (k & np.uint64(LOCAL_MASK)))


# ----------------------------------------------------------------------------- builders
def rows_at(q0, d, rng):
    """u8[len(d), cb]: row i differs from q0 in exactly d[i] bits: the first d[i] of one seeded order of the
    bit positions (spread over every word of the code), started at a seeded offset per row."""
    d = np.asarray(d, dtype=np.int64)
    dim = q0.shape[0] * 8
    assert d.min() >= 0 and d.max() <= dim
    order = rng.permutation(dim)
    out = np.empty((d.shape[0], q0.shape[0]), np.uint8)
    for r0 in range(0, d.shape[0], 4096):
        dd = d[r0:r0 + 4096]
        off = rng.integers(0, dim, dd.shape[0])
        flip = np.empty((dd.shape[0], dim), bool)
        flip[:, order] = (np.arange(dim)[None, :] - off[:, None]) % dim < dd[:, None]
        out[r0:r0 + 4096] = np.packbits(flip, axis=1) ^ q0[None, :]
    return out


def schedule_dists(schedule, dim, rng=None):
    """Distances i64[64 * tiles] of a schedule: entry t lists the (count, distance) groups of tile t, its other
    rows sit at distance dim.  With ``rng`` the groups take seeded lanes of the tile, else its first ones."""
    out = np.full((len(schedule), 64), dim, np.int64)
    for t, groups in enumerate(schedule):
        lanes = np.arange(64) if rng is None else rng.permutation(64)
        at = 0
        for m, dist in groups:
            assert 0 <= dist <= dim and at + m <= 64
            out[t, lanes[at:at + m]] = dist
            at += m
    return out.reshape(-1)


def build_chunk(q0, schedule, rng, spread=True):
    """(codes u8[64 * tiles, cb], distances to q0) of a schedule."""
    d = schedule_dists(schedule, q0.shape[0] * 8, rng if spread else None)
    return rows_at(q0, d, rng), d


def ramp(tiles, dim, d0=None):
    """A distance per tile, strictly decreasing from d0 (default dim - 1) and >= 0."""
    d0 = dim - 1 if d0 is None else d0
    step = max(d0 // max(tiles - 1, 1), 1)
    assert d0 - (tiles - 1) * step >= 0, "more tiles than distances"
    return [d0 - t * step for t in range(tiles)]


def sched_full_tiles(tiles, dim, d0=None):
    """Every row of every tile scheduled.  At CAP - 128 < K <= CAP - 64 every tile after the fill re-sorts; at
    K = CAP - 64 each of them also leaves the list at CAP exactly, so the next one overflows a full list."""
    return [[(64, d)] for d in ramp(tiles, dim, d0)]


def sched_overflow_by_one(tiles, dim, K, cap):
    """After the first cut the list is topped up to CAP exactly, then a tile brings one row."""
    dr = ramp(tiles, dim)
    out, cnt, cut = [], 0, False
    for t in range(tiles):
        if not cut:                      # tau is still open: all 64 rows pass, scheduled or not
            m = 64
            if cnt + 64 > cap:
                cnt, cut = K, True
            cnt += 64
        elif cnt == cap:
            m, cnt = 1, K + 1
        else:
            m = min(64, cap - cnt)
            cnt += m
        out.append([(m, dr[t])])
    return out


def sched_partial(tiles, dim, K):
    """K = CAP - 64 = 64 w.  Full tiles re-sort every tile: at tile t the old tau is the last key of tile
    t - w - 1 and the new one the last key of tile t - w.  Every (w + 2)-th tile puts 24 of its rows at the
    distance of tile t - w: below the old tau, not below the new one (equal distance, larger row); the w + 1 full
    tiles that follow push those rows out of the list again."""
    w = K // 64
    assert K == 64 * w
    dr = ramp(tiles, dim)
    return [[(40, dr[t]), (24, dr[t - w])] if t >= w + 2 and t % (w + 2) == 0 else [(64, dr[t])]
            for t in range(tiles)]


def sched_late_ramp(tiles, dim, last=20):
    """Rows at the maximum distance, then a ramp over the chunk's last tiles."""
    dr = ramp(last, dim)
    return [[] for _ in range(tiles - last)] + [[(64, d)] for d in dr]


def sched_tau_gap(tiles, dim, K):
    """K = 64 w + 1 with K + 128 > CAP: full tiles re-sort every tile, and on entry to the last tile the list's
    K-th key is the first row of tile T - 2 - w, its (K - 1)-th the last row of tile T - 1 - w, at a smaller
    distance.  The last tile's rows sit at that smaller distance: every one of them lies between the two keys,
    and the first of them is the chunk's true K-th row.  A tau taken one position low rejects them all."""
    w = (K - 1) // 64
    assert K == 64 * w + 1 and K + 128 > cap_for(K)
    dr = ramp(tiles, dim)
    return [[(64, d)] for d in dr[:tiles - 1]] + [[(64, dr[tiles - 1 - w])]]


def reference_list(dists, K):
    """Sorted top-min(K, rows) chunk keys of the distances of one chunk, by (distance, row)."""
    d = np.asarray(dists, dtype=np.int64)
    return np.sort((d << LOCAL_BITS) | np.arange(d.shape[0], dtype=np.int64))[:K]


# the adversarial cases of tests/test_gpu_wave_lists.py: name -> (K, schedule(tiles, dim))
def adversarial_cases(dim):
    c = {}
    for K in (150, 400, 900):
        c[f"every_tile_K{K}"] = (K, lambda T, K=K: sched_full_tiles(T, dim))
    for K in (192, 448, 960):
        c[f"exact_fill_K{K}"] = (K, lambda T, K=K: sched_full_tiles(T, dim))
    for K in (100, 192, 449):
        c[f"by_one_K{K}"] = (K, lambda T, K=K: sched_overflow_by_one(T, dim, K, cap_for(K)))
    for K in (192, 448):
        c[f"partial_K{K}"] = (K, lambda T, K=K: sched_partial(T, dim, K))
    for K in (192, 300):
        c[f"late_ramp_K{K}"] = (K, lambda T, K=K: sched_late_ramp(T, dim))
    for K in (129, 385, 897):
        c[f"tau_gap_K{K}"] = (K, lambda T, K=K: sched_tau_gap(T, dim, K))
    if dim == 2048:
        c["top_bit_K192"] = (192, lambda T: sched_full_tiles(T, dim, d0=dim))
    return c
