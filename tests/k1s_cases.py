"""Inputs of the K1s edge tests (tests/test_gpu_k1s_edges.py) and the arithmetic their preconditions rest
on, in NumPy only, so that tests/test_k1s_cases.py checks every precondition without a GPU.

K1s (hamming_mfma_swap_kernel<2, 8>) geometry the builders aim at -- the chunk size and count come from
vrq_scan_plan (chunk rows ``cr``, a multiple of 64), the rest restates the kernel's shape constants:

* a workgroup serves one (chunk, 512-query block): query q is query q % 512 of workgroup q // 512, in
  32-query block (q % 512) // 32 at position q % 32; the blocks run in pairs, so a workgroup of nqv
  valid queries runs ceil(nqv / 32) rounded up to even blocks;
* the chunk's rows are split into 64-row sets; set rs belongs to wave rs % 8 and is that wave's
  (rs // 8)-th set; rows 0..31 / 32..63 of a set are its two row blocks;
* each wave stages at most STG = 512 hits per row set over the workgroup's 512 queries; a set whose
  hits pass that marks the lists of the query block in which it happened and of every later block of the
  workgroup (exact rescan), and keeps the earlier blocks' staged hits.
"""
import math

import numpy as np

SRS = 64        # rows per row set
SNW = 8         # waves per workgroup
SQPB = 512      # queries per workgroup
STG = 512       # staged hits per wave and row set
MIN_SAMPLE = 65536


def sample_order(lam, K):
    """mfma_sample_order (mfma_threshold.hip): the smallest j < K with P(Poisson(lam) >= j) <= 1e-6, else K."""
    term, cdf = math.exp(-lam), 0.0
    for j in range(1, K):
        cdf += term
        if 1.0 - cdf <= 1e-6:
            return j
        term *= lam / j
    return K


def flip(rng, rows, nflip, lo=0, hi=1024):
    """Copies of `rows` with exactly nflip distinct bits of [lo, hi) flipped each (np.unpackbits order)."""
    m = rows.shape[0]
    out = np.empty((m, 128), np.uint8)                   # C-contiguous (rows may be a broadcast view)
    out[...] = rows
    pos = rng.integers(lo, hi, (m, nflip))
    while nflip > 1:                                     # distinct positions per row
        bad = (np.diff(np.sort(pos, axis=1), axis=1) == 0).any(axis=1)
        if not bad.any():
            break
        pos[bad] = rng.integers(lo, hi, (int(bad.sum()), nflip))
    flat = out.reshape(-1)
    base = np.arange(m, dtype=np.int64) * 128
    for c in range(nflip):                               # one position per row per step: unique indices
        flat[base + (pos[:, c] >> 3)] ^= (0x80 >> (pos[:, c] & 7)).astype(np.uint8)
    return out


def distances(qb, codes, block=16384):
    """Exact Hamming distances i16[nq, n]: pc(q) + pc(r) - 2 <q, r>, integers <= 1024 in float32."""
    qbits = np.unpackbits(qb, axis=1).astype(np.float32)
    pcq = qbits.sum(1)
    out = np.empty((qb.shape[0], codes.shape[0]), np.int16)
    for r0 in range(0, codes.shape[0], block):
        cb = np.unpackbits(codes[r0:r0 + block], axis=1).astype(np.float32)
        out[:, r0:r0 + block] = pcq[:, None] + cb.sum(1)[None, :] - 2.0 * (qbits @ cb.T)
    return out


def standin_tau(D, K, slack=3):
    """(K-th smallest distance + slack) per query: a generous stand-in for the threshold a pass runs with
    (tau_p = the K-th smallest lane minimum of the dense sample + 1, which covers nearly every row at
    these sizes)."""
    return np.partition(D, K - 1, axis=1)[:, K - 1].astype(np.int64) + slack


def stage_load(hit, wg):
    """Hits each 64-row set stages for workgroup wg: i64[ceil(n / 64)].  (Chunks are multiples of 64 rows,
    so the row sets of every chunk are the corpus's 64-row groups; the last one may be partial.)"""
    per_row = hit[wg * SQPB:(wg + 1) * SQPB].sum(0, dtype=np.int64)
    return np.add.reduceat(per_row, np.arange(0, hit.shape[1], SRS))


def list_load(hit, cr):
    """Entries of every (query, chunk) list: i64[nq, chunks]."""
    return np.add.reduceat(hit.astype(np.int32), np.arange(0, hit.shape[1], cr), axis=1)


def blocks_run(nq, wg):
    """Query blocks workgroup wg runs (pairs: rounded up to even) and how many of them hold a query."""
    nqv = min(SQPB, nq - wg * SQPB)
    valid = (nqv + 31) // 32
    return (valid + 1) & ~1, valid


# ---------------------------------------------------------------------------------- geometry matrix
def geometry_case(n, nq, cr, seed):
    """Uniform codes, queries 40 flips from random rows; query 0 is an exact copy of the corpus's last row
    and query nq - 1 of the first row of the last chunk."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    qb = flip(rng, codes[rng.integers(0, n, nq)], 40)
    qb[0] = codes[n - 1]
    qb[nq - 1] = codes[(n - 1) // cr * cr]
    return codes, qb


# ------------------------------------------------------------------------------------ dense patches
def patch_specs(n, nq, cr):
    """(chunk, row set, row subset, workgroup, query block, query parity) of every patch.  Row subset
    s = 2 rb + p: rows 32 rb + 2 i + p of the set (16 of row block rb); query parity p: positions 2 i + p.
    One patch per chunk and per query group, so no patch takes another's queries or rows."""
    nch = (n + cr - 1) // cr
    spc = cr // SRS
    assert spc > SNW and nch > 112, "wave 0 needs a second row set, and the patches chunks of their own"
    last_wg = (nq - 1) // SQPB
    last_blk = blocks_run(nq, last_wg)[1] - 1
    specs = []
    qgrp = [(0, 0, 0), (0, 15, 0), (0, 0, 1), (0, 15, 1), (0, 7, 0), (0, 8, 1), (0, 3, 0), (0, 12, 1)]
    for w in range(SNW):                                 # every wave's first row set
        specs.append((3 + 13 * w, w, w % 4) + qgrp[w])
    for i, g in enumerate([(last_wg, 0, 0), (last_wg, 0, 1), (last_wg, 1, 1), (last_wg, last_blk, 0)]):
        specs.append((105 + i, SNW, i) + g)              # wave 0's second set, after the switch
    nlast = n - (nch - 1) * cr                           # the partial last set of the last chunk
    assert nlast % SRS, "the last chunk must end in a partial row set"
    specs.append((nch - 1, (nlast - 1) // SRS, 0, 0, 5, 0))
    specs.append((nch - 1, (nlast - 1) // SRS, 1, 0, 6, 1))
    return specs


def patch_case(n, nq, cr, seed):
    """The geometry matrix's background plus the dense patches: per patch a fresh base, its queries 4 flips
    from it and its rows 6 flips from it, so each (query, row) pair of a patch is at distance <= 10.
    -> codes, qb, [(queries, rows)] per patch (rows past the chunk's end and queries past nq dropped)."""
    codes, qb = geometry_case(n, nq, cr, seed)
    rng = np.random.default_rng(seed + 1)
    patches = []
    for chunk, rs, rsub, wg, blk, par in patch_specs(n, nq, cr):
        base = rng.integers(0, 256, (1, 128), dtype=np.uint8)
        rows = chunk * cr + rs * SRS + 32 * (rsub >> 1) + 2 * np.arange(16) + (rsub & 1)
        rows = rows[rows < min(n, (chunk + 1) * cr)]
        qs = wg * SQPB + 32 * blk + 2 * np.arange(16) + par
        qs = qs[qs < nq]
        if rows.size == 0 or qs.size == 0:
            continue
        codes[rows] = flip(rng, np.repeat(base, rows.size, axis=0), 6)
        qb[qs] = flip(rng, np.repeat(base, qs.size, axis=0), 4)
        patches.append((qs, rows))
    return codes, qb, patches


# ---------------------------------------------------------------------------- late-block stage flood
FLOOD_S = 32_768                                         # the suffix [FLOOD_S, n) holds the flood rows
FLOOD_BLOCKS = ((0, 14), (1, 9))                         # (workgroup, flooded query block)


def flood_queries():
    return np.concatenate([wg * SQPB + 32 * blk + np.arange(32) for wg, blk in FLOOD_BLOCKS])


def flood_may_mark(nq):
    """Queries a flooded row set may mark overflowed: the flooded block and the later ones of its workgroup."""
    return np.concatenate([np.arange(wg * SQPB + 32 * blk, min(nq, (wg + 1) * SQPB)) for wg, blk in FLOOD_BLOCKS])


def flood_case(n, nq, seed):
    """Suffix rows = base with 6 flips among bits 512..1023, flood queries = base with 4 flips among bits
    0..511: every (flood query, suffix row) distance is exactly 10.  The other queries are uniform and
    at least 512 from base (complemented where nearer), so the suffix rows are never their candidates.
    In every 64-row set of the suffix, rows 3 and 40 are witnesses: 8-flip copies of a query of a block
    BEFORE the flooded one of workgroup 0 / 1, rotating through those blocks and their positions.
    -> codes, qb, witnesses [(query, row)]"""
    assert FLOOD_S % SRS == 0 and nq == 2 * SQPB
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (1, 128), dtype=np.uint8)
    codes = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    codes[FLOOD_S:] = flip(rng, np.repeat(base, n - FLOOD_S, axis=0), 6, 512, 1024)
    qb = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    near = np.unpackbits(qb ^ base, axis=1).sum(1) < 512
    qb[near] = ~qb[near]
    fq = flood_queries()
    qb[fq] = flip(rng, np.repeat(base, fq.size, axis=0), 4, 0, 512)
    wit = []
    for k, s0 in enumerate(range(FLOOD_S, n, SRS)):
        for (wg, blk), pos in zip(FLOOD_BLOCKS, (3, 40)):
            row = s0 + pos
            if row < n:
                q = wg * SQPB + 32 * (k % blk) + (k // blk + 5 * wg) % 32
                wit.append((q, row))
    wq, wr = np.array(wit).T
    codes[wr] = flip(rng, qb[wq], 8)
    return codes, qb, wit


# -------------------------------------------------------------------------------- two-valued corpus
def two_valued_case(n, nq, seed):
    """All rows zero except 50 all-ones rows at random places; query 0 all ones, query 1 all zeros, the rest
    uniform.  -> codes, qb, the ones rows (sorted)"""
    rng = np.random.default_rng(seed)
    codes = np.zeros((n, 128), np.uint8)
    ones = np.sort(rng.choice(n, 50, replace=False))
    codes[ones] = 255
    qb = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    qb[0] = 255
    qb[1] = 0
    return codes, qb, ones


# ------------------------------------------------------------------------- sampled-threshold re-run
def sample_lanes(rows, ts, tiles_per_chunk):
    """Lane of the dense sample pass that holds each of `rows` (all sample rows): tile i = row // ts ...
    of sample chunk i // T, lane row (row - i * ts) % 32 -> column chunk * 32 + lane row, as
    test_scan_sample_lane_minima_exact restates it."""
    rows = np.asarray(rows, np.int64)
    tile = rows // ts
    within = rows - tile * ts
    assert (within < 64).all(), "not a sample row"
    return (tile // tiles_per_chunk) * 32 + (within & 31)
