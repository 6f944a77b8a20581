"""A NumPy restatement of what the counting scan leaves in its workspace, stage by stage, from a distance matrix
and a row mask -- and the planted inputs of tests/test_gpu_batch_scan.py.  No kernel appears here.

  count      hist[q, c, b] = allowed rows r of chunk c (rows [c * chunk_rows, (c + 1) * chunk_rows)) with
             dist(q, r) == b
  threshold  want = min(K, n) (filtered: min(K, allowed rows)); T = the smallest t with count(dist <= t) >= want,
             c_lt = count(dist < T); want == 0 leaves T = dim, c_lt = 0
  emit       the K-list of q: its allowed rows below T in row order, then its first want - c_lt allowed rows at T
             in row order, as keys dist << 40 | row, all-ones padded to K
"""
import numpy as np

POP = np.array([bin(i).count("1") for i in range(256)], np.int64)
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def distances(codes, queries):
    """int64 [nq, n] Hamming distances of uint8 code arrays."""
    return np.stack([POP[codes ^ q].sum(1) for q in queries])


def model(D, mask, chunk_rows, K, dim, filtered):
    """(hist u32[nq, chunks, dim + 1], tc i32[nq, 2], lists u64[nq, K]) for distances D i64[nq, n], mask bool[n]."""
    nq, n = D.shape
    chunks = -(-n // chunk_rows)
    rows = np.flatnonzero(mask)
    cid = rows // chunk_rows
    hist = np.zeros((nq, chunks, dim + 1), np.uint32)
    tc = np.zeros((nq, 2), np.int32)
    lists = np.full((nq, K), KEY_NONE, np.uint64)
    want = min(K, n)
    if filtered:
        want = min(want, rows.shape[0])
    for q in range(nq):
        d = D[q, rows]
        hist[q] = np.bincount(cid * (dim + 1) + d, minlength=chunks * (dim + 1)).reshape(chunks, dim + 1)
        cum = np.cumsum(hist[q].sum(0, dtype=np.int64))
        if want == 0:
            T, c_lt = dim, 0
        else:
            T = int(np.searchsorted(cum, want, side="left"))
            c_lt = int(cum[T - 1]) if T else 0
        tc[q] = (T, c_lt)
        lt = rows[d < T]
        eq = rows[d == T][:want - c_lt]
        assert lt.shape[0] == c_lt and c_lt + eq.shape[0] == want
        keys = np.concatenate([(np.uint64(1) << np.uint64(40)) * D[q, lt].astype(np.uint64) + lt.astype(np.uint64),
                               (np.uint64(1) << np.uint64(40)) * D[q, eq].astype(np.uint64) + eq.astype(np.uint64)])
        lists[q, :want] = keys
    return hist, tc, lists


def pack(mask, tail=False):
    """bool[n] -> the ABI's bitmap words as an int64 array; tail: every bit past n in the last word set."""
    n = mask.shape[0]
    by = np.zeros(((n + 63) // 64) * 8, np.uint8)
    p = np.packbits(mask, bitorder="little")
    by[:p.shape[0]] = p
    w = by.view("<u8").copy()
    if tail and n % 64:
        w[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    return w.view(np.int64)


MASKS = ("ones", "zeros", "first", "last", "r50", "r01", "range", "altwords", "lowhalf", "highhalf")


def masks(n, chunk_rows):
    """The masks of tests/test_gpu_filtered.py, and the two that allow one n-block of every 64-row tile only."""
    rng = np.random.default_rng(77)
    r = np.arange(n)
    m = {}
    m["ones"] = np.ones(n, bool)
    m["zeros"] = np.zeros(n, bool)
    m["first"] = r == 0
    m["last"] = r == n - 1
    m["r50"] = rng.random(n) < 0.5
    m["r01"] = rng.random(n) < 0.01
    lo, hi = chunk_rows + 37, 2 * chunk_rows + 1000 + 5      # mid-tile in chunk 1 ... mid-tile in chunk 2
    m["range"] = (r >= lo) & (r < hi)
    m["altwords"] = (r >> 6) % 2 == 0                        # all-ones and zero words alternate
    m["lowhalf"] = (r >> 5) % 2 == 0                         # the low half of every tile's word
    m["highhalf"] = (r >> 5) % 2 == 1                        # the high half
    return m


# ---- planted inputs ----
def random_case(n, dim, nq, seed):
    """Random codes and queries; query 1 equals a code (bin 0), and one row is query 0's complement (bin dim)."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
    queries = rng.integers(0, 256, (nq, dim // 8), dtype=np.uint8)
    codes[n // 3] = ~queries[0]
    if nq > 1:
        queries[1] = codes[n // 2]
    return codes, queries


def tie_case(n, dim, nq, chunk_rows, K, seed):
    """A two-valued corpus: rows r with r % 3 != 0 hold A, the others B, and every query is nearer to A than to
    B.  So T = dist(q, A) for every query, c_lt = 0, every A row sits at T, and the cut after the K-th A row falls
    where the caller's K puts it: test_batch_scan_model.py checks that this is strictly inside an n-block of a
    chunk that is neither the first nor the last."""
    rng = np.random.default_rng(seed)
    cb = dim // 8
    A = rng.integers(0, 256, cb, dtype=np.uint8)
    B = ~A
    codes = np.where((np.arange(n) % 3 != 0)[:, None], A[None, :], B[None, :]).astype(np.uint8)
    queries = np.repeat(A[None, :], nq, 0)
    flip = rng.integers(0, dim // 4, nq)   # query j differs from A in flip[j] < dim / 2 bits: nearer to A
    for j in range(nq):
        bits = rng.choice(dim, flip[j], replace=False)
        for b in bits:
            queries[j, b >> 3] ^= np.uint8(1 << (b & 7))
    return codes, queries, flip
