"""Host-only model of the scores the library defines as exact quantities, in integer / Fraction arithmetic
(no float summation), the fixtures that take the kernels off the grid on which every summation order agrees,
and NumPy float64 restatements of the summation orders the kernels use (for tests/test_exact_score_model.py).

  Phase II   float(q . (2 * unpackbits(code) - 1)) in float64
  Phase III  the exact dot q . int8 row, rounded once to float32, divided by the float64 norm (-inf if 0)
  flat IP    the exact dot q . float32 row, rounded once to float32

A kernel sums n exact products in float64 in some order.  Two facts bound what it may return:
  * ``order_free``: all non-zero |q_i| are multiples of 2^g and wmax * sum|q_i| < 2^(g + 53).  Then every
    partial sum of every order is a multiple of 2^g below 2^(g + 53), hence exact: the float64 sum IS
    ``exact_dot`` and all paths are bit-identical.
  * otherwise ``sum_bound`` = gamma_(n-1) * sum|q_i w_i|, gamma_m = m u / (1 - m u), u = 2^-53: the a-priori
    bound of a float64 sum of n exact terms in ANY order (Higham, Accuracy and Stability, section 4.2) -- a
    leaf passes at most n - 1 roundings in the butterfly, in the 4 + 256 nibble sums and in a lane's loop alike.
"""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
# 128: the model only (one lane block; the library starts at 256).  256, 384: one short nibble pass; 768: a full pass
# and a short one; 1536: three full passes; 1024: its own kernels; 2048: the longest loop.
DIMS = (128, 256, 384, 768, 1024, 1536, 2048)
A_BIG = 2.0 ** 60


# ----------------------------------------------------------------------------- exact arithmetic
def _decompose(a):
    """float32 array -> (mant int64, exp int64) with a == mant * 2^exp exactly (denormals are ordinary values)."""
    a = np.asarray(a)
    assert a.dtype == np.float32 and np.isfinite(a).all()
    m, e = np.frexp(a.astype(np.float64))
    mant = np.ldexp(m, 24).astype(np.int64)          # |m| in [0.5, 1) with <= 24 bits: an integer
    assert np.array_equal(np.ldexp(mant.astype(np.float64), e - 24), a.astype(np.float64))
    return mant, (e - 24).astype(np.int64)


def weights(w, dim):
    """The integer weights of a row: +-1 of a packed code (uint8[dim / 8], packbits MSB first) or an int8 row."""
    w = np.asarray(w)
    if w.dtype == np.uint8:
        assert w.shape[-1] * 8 == dim
        return 2 * np.unpackbits(w, axis=-1).astype(np.int64) - 1
    assert w.dtype == np.int8 and w.shape[-1] == dim
    return w.astype(np.int64)


def _assemble(sums, exps):
    """sum_j sums[j] * 2^exps[j] as a Fraction (Python integers)."""
    nz = [(int(s), int(e)) for s, e in zip(sums, exps) if s != 0]
    if not nz:
        return Fraction(0)
    emin = min(e for _, e in nz)
    tot = sum(s << (e - emin) for s, e in nz)
    return Fraction(tot) * Fraction(2) ** emin


def _terms(q, w):
    """(int64 term mantissas, exponents) of the products q_i * w_i."""
    q = np.asarray(q)
    mq, eq = _decompose(q)
    w = np.asarray(w)
    if w.dtype == np.float32:
        mw, ew = _decompose(w)
        return mq * mw, eq + ew                       # < 2^48
    return mq * weights(w, q.shape[0]), eq


def _grouped(t, e):
    ue, inv = np.unique(e, return_inverse=True)
    sums = np.zeros(ue.shape[0], np.int64)            # <= 2048 terms below 2^48: no overflow
    np.add.at(sums, inv, t)
    return sums, ue


def exact_dot(q, w):
    """The exact rational sum q_i * w_i; w a packed code (+-1), an int8 row or a float32 row."""
    t, e = _terms(q, w)
    return _assemble(*_grouped(t, e))


def abs_dot(q, w):
    """The exact sum |q_i * w_i|."""
    t, e = _terms(q, w)
    return _assemble(*_grouped(np.abs(t), e))


def exact_dots(q, W, absolute=False):
    """exact_dot (or abs_dot) of one query against every row of W (codes uint8[R, dim / 8] or int8[R, dim]): one
    integer matrix product per exponent class of the query."""
    q = np.asarray(q)
    mq, eq = _decompose(q)
    Wi = weights(W, q.shape[0])
    if absolute:
        mq, Wi = np.abs(mq), np.abs(Wi)
    ue, inv = np.unique(eq, return_inverse=True)
    M = np.zeros((ue.shape[0], q.shape[0]), np.int64)
    M[inv, np.arange(q.shape[0])] = mq
    P = M @ Wi.T                                      # int64, exact: < 2048 * 2^24 * 128
    return [_assemble(P[:, r], ue) for r in range(Wi.shape[0])]


def _rn(x, p, qmin, emax):
    """x (Fraction) rounded once to the binary format with p significand bits, least quantum 2^qmin and largest
    exponent emax, ties to even; returned as a Python float (exact: the format is a subset of float64)."""
    x = Fraction(x)
    if x == 0:
        return 0.0
    sign = -1.0 if x < 0 else 1.0
    n, d = abs(x).numerator, abs(x).denominator
    e = n.bit_length() - d.bit_length()               # 2^(e-1) < x < 2^(e+1)
    if (n >> e if e >= 0 else n << -e) < d:           # x < 2^e
        e -= 1
    qe = max(e - (p - 1), qmin)                       # quantum of the result (subnormal: qmin)
    num, den = (n, d << qe) if qe >= 0 else (n << -qe, d)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and m & 1):
        m += 1
    if m >= 2 ** p:                                   # rounded up into the next binade
        m >>= 1                                       # (m == 2^p exactly)
        qe += 1
    if qe + p - 1 > emax:
        return sign * float("inf")
    return sign * float(np.ldexp(float(m), qe))


def rn64(x):
    """One correct rounding (ties to even) of an exact value to float64."""
    return _rn(x, 53, -1074, 1023)


def rn32(x):
    """One correct rounding (ties to even) of an exact value to float32, as a Python float."""
    return _rn(x, 24, -149, 127)


def order_free(q, wmax):
    """True iff all non-zero |q_i| are multiples of some 2^g and wmax * sum|q_i| < 2^(g + 53): every partial sum
    of q_i * w_i, |w_i| <= wmax integers, is then exact in float64 in every order."""
    mq, eq = _decompose(np.asarray(q))
    nz = mq != 0
    if not nz.any():
        return True
    m, e = np.abs(mq[nz]), eq[nz]
    tz = np.array([(int(v) & -int(v)).bit_length() - 1 for v in m])
    g = int((e + tz).min())
    total = _assemble(*_grouped(m, e)) * int(wmax)
    return total < Fraction(2) ** (g + 53)


def gamma(m):
    return m * U / (1 - m * U)


def sum_bound(q, w, absdot=None):
    """gamma_(n-1) * sum|q_i w_i|: the a-priori error bound of a float64 sum of the n exact products in any
    order.  Derived, not tuned.  (``absdot``: the sum, if the caller has it.)"""
    return gamma(np.asarray(q).shape[0] - 1) * (abs_dot(q, w) if absdot is None else absdot)


def f32_between(lo, hi, limit=4):
    """The float32 values f = rn32(y) for y in [lo, hi] (rounding is monotone: every float32 from rn32(lo) to
    rn32(hi)), ascending; None when there are more than ``limit``."""
    a, b = np.float32(rn32(lo)), np.float32(rn32(hi))
    out = [a]
    while out[-1] < b:
        if len(out) == limit:
            return None
        out.append(np.nextafter(out[-1], np.float32(np.inf)))
    return [float(v) for v in out]


def phase3_values(q, x, norm, exact=None, bound=None, limit=4):
    """The values Phase III (``norm`` a float) or the flat inner product (``norm`` None) may return for the row:
    {float64(f) / norm} over the float32 f = rn32(y), y in [exact - sum_bound, exact + sum_bound]; one element,
    or two adjacent ones, wherever the bound is small against the float32 spacing; [-inf] for a zero norm.
    None when the reference alone admits more than ``limit`` values."""
    if norm is not None and norm == 0.0:
        return [-np.inf]
    exact = exact_dot(q, x) if exact is None else exact
    bound = sum_bound(q, x) if bound is None else bound
    fs = f32_between(exact - bound, exact + bound, limit)
    if fs is None:
        return None
    return fs if norm is None else [float(np.float64(f) / np.float64(norm)) for f in fs]


def int8_norm(x):
    """sqrt of the exact integer sum of squares, correctly rounded (np.linalg.norm of the reference)."""
    return float(np.sqrt(np.float64(int((np.asarray(x, np.int64) ** 2).sum()))))


# ----------------------------------------------------------------------------- summation orders (float64)
def products(q, w):
    """The float64 products q_i * w_i (exact: 24-bit x 24-bit significands at the most); rows on axis -2."""
    q = np.asarray(q, np.float32).astype(np.float64)
    w = np.asarray(w)
    ww = w.astype(np.float64) if w.dtype == np.float32 else weights(w, q.shape[-1]).astype(np.float64)
    return q * ww


def _butterfly(s):
    """The wave's butterfly all-reduce over axis -1 (64 lanes): a balanced tree over adjacent lanes."""
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def order_wave1024(t):
    """phase2_dot / phase3_cos / flat_ip at 1024: lane l sums dims 16l .. 16l+15 in turn, then the butterfly."""
    t = t.reshape(t.shape[:-1] + (64, 16))
    s = np.zeros(t.shape[:-1])
    for i in range(16):
        s = s + t[..., i]
    return _butterfly(s)


def order_wave_dim(t):
    """phase2_dot_dim / phase3_cos_dim: lane l takes dims 2l and 2l+1 of every 128-dim block, then the butterfly."""
    t = t.reshape(t.shape[:-1] + (t.shape[-1] // 128, 64, 2))
    s = np.zeros(t.shape[:-3] + (64,))
    for b in range(t.shape[-3]):
        s = s + t[..., b, :, 0]
        s = s + t[..., b, :, 1]
    return _butterfly(s)


def order_nibble(t, pass_bytes=64, drop_short_last=False):
    """phase2_nibble_tables / _dim: the table entry of a nibble sums its 4 terms in turn from 0, the candidate's
    accumulator adds the entries in nibble order through passes of up to ``pass_bytes`` code bytes (the passes
    only rebuild the tables: the accumulator runs on).  ``drop_short_last``: a wrong variant for the tests."""
    tv = t.reshape(t.shape[:-1] + (t.shape[-1] // 4, 4))
    T = ((tv[..., 0] + tv[..., 1]) + tv[..., 2]) + tv[..., 3]
    cb = t.shape[-1] // 8
    if drop_short_last and cb % pass_bytes:
        T = T[..., :2 * (cb - cb % pass_bytes)]
    T = np.concatenate([np.zeros(T.shape[:-1] + (1,)), T], axis=-1)      # acc = 0.0; acc += T[p] ...
    return np.add.accumulate(T, axis=-1)[..., -1]


def order_sequential(t):
    return np.add.accumulate(t, axis=-1)[..., -1]


ORDERS = {"wave1024": order_wave1024, "wave_dim": order_wave_dim, "nibble": order_nibble,
          "sequential": order_sequential}


def orders_for(dim):
    return {k: f for k, f in ORDERS.items() if k != "wave1024" or dim == 1024}


# ----------------------------------------------------------------------------- fixtures
FAMILIES = ("a", "b", "c", "d", "e", "f")


def big_positions(dim):
    """Where family (d) puts its cancelling pairs (+A, -A), (-A, +A): different lanes of both wave orders and
    different nibbles.  The int8 and float32 corpora are zero there: Phase III of such a query is then as well
    conditioned as of any other (a product with 2^60 would push ``sum_bound`` past the float32 spacing and leave
    the reference itself ambiguous); Phase II takes the pairs in full."""
    return (3, dim // 2 + 38, 17, dim - 5)


def _limit_query(dim, rng, wmax):
    """Family (a): magnitudes from 2^0 down to the smallest power of two ``order_free`` admits for the dim and
    wmax, 24-bit multiples of it, and +-0.0."""
    for E in range(52, 0, -1):
        e = rng.integers(0, E + 1, dim)
        q = np.ldexp(rng.choice([-1.0, 1.0], dim), -e)
        wide = rng.random(dim) < 0.25                  # 24-bit multiples of 2^-E
        q[wide] = rng.choice([-1.0, 1.0], wide.sum()) * np.ldexp(rng.integers(1, 2 ** 24, wide.sum()).astype(float), -E)
        q[np.abs(q) > 1.0] = 1.0
        q[0], q[1], q[dim - 1], q[dim // 2] = 1.0, -2.0 ** -E, 2.0 ** -E, -1.0
        q[5], q[dim - 9] = 0.0, -0.0
        q = q.astype(np.float32)
        if order_free(q, wmax):
            return q, E
    raise AssertionError("no order-free exponent range")


def queries(dim, seed=0):
    """{family: float32[nq_f, dim]} and the per-query facts the tests need (``meta``)."""
    rng = np.random.default_rng(1000 * dim + seed)
    out, meta = {}, {}
    q1, E1 = _limit_query(dim, rng, 1)
    q127, E127 = _limit_query(dim, rng, 127)
    den = np.ldexp(q127.astype(np.float64), E127 - 149).astype(np.float32)   # floor at 2^-149: denormals, exactly
    assert np.array_equal(np.ldexp(den.astype(np.float64), 149 - E127), q127.astype(np.float64))
    assert (np.abs(den[den != 0]) < 2.0 ** -126).any()
    out["a"] = np.stack([q1, q127, den])
    meta["a_wmax"] = (1, 127, 127)
    meta["a_E"] = (E1, E127, E127)
    g = rng.standard_normal((2, dim))
    tiny = rng.random((2, dim)) < 0.5
    out["b"] = np.where(tiny, g * 1e-9, g).astype(np.float32)
    out["c"] = (rng.standard_normal((2, dim)) * np.exp(rng.normal(0.0, 8.0, (2, dim)))).astype(np.float32)
    d = rng.standard_normal((2, dim)).astype(np.float32)
    p = big_positions(dim)
    d[0, p[0]], d[0, p[1]], d[0, p[2]], d[0, p[3]] = A_BIG, -A_BIG, -A_BIG, A_BIG
    d[1, p[0]], d[1, p[1]], d[1, p[2]], d[1, p[3]] = -A_BIG, A_BIG, A_BIG, -A_BIG
    out["d"] = d
    # (e), (f): on the 2^-24 grid; halves that cancel against the rows of ``tie_rows``; (e) adds 1 + m 2^-24
    h = dim // 2
    base = (np.round(rng.standard_normal(h) * 0.05 / 2.0 ** -24) * 2.0 ** -24)
    base[base == 0] = 2.0 ** -24
    ef = np.tile(np.concatenate([base, base]).astype(np.float32), (3, 1))
    ef[0:2, 40], ef[0:2, h + 40] = 1.0, 2.0 ** -24      # row weights there: (1, 1) and (1, 3)
    out["e"] = ef[0:2]
    out["f"] = ef[2:3]
    return out, meta


def tie_rows(dim, seed=0):
    """int8 rows for families (e), (f): x[h + i] = -x[i] (so the halves of the (e) / (f) queries cancel), except
    at dims 40 and h + 40, where row 0 has (1, 1), row 1 has (1, 3) and row 2 the cancelling (7, -7):
      (e) query 0 . row 0 = 1 + 2^-24: a tie, rounds DOWN to even 1;
      (e) query 1 . row 1 = 1 + 3 2^-24: a tie, rounds UP to even 1 + 2^-22;
      (f) query . row 2 = 0 from dim non-zero terms."""
    rng = np.random.default_rng(77 * dim + seed)
    h = dim // 2
    half = rng.integers(1, 128, (3, h)).astype(np.int8) * rng.choice([-1, 1], (3, h)).astype(np.int8)
    x = np.concatenate([half, -half], axis=1).astype(np.int8)
    x[0, 40], x[0, h + 40] = 1, 1
    x[1, 40], x[1, h + 40] = 1, 3
    x[2, 40], x[2, h + 40] = 7, -7
    return x


TIE_EXPECT = ((0, 0, 1.0), (1, 1, 1.0 + 2.0 ** -22))   # ((e) query, tie row, the float32 dot)


def code_rows(dim, nrand, seed=0):
    """Packed codes: all zeros, all ones, 0x0F, 0xF0, 0xA5, a single set bit at dims 0, 7, 8, dim - 1, random."""
    rng = np.random.default_rng(31 * dim + seed)
    cb = dim // 8
    rows = [np.full(cb, v, np.uint8) for v in (0x00, 0xFF, 0x0F, 0xF0, 0xA5)]
    for bit in (0, 7, 8, dim - 1):
        r = np.zeros(cb, np.uint8)
        r[bit // 8] = 0x80 >> (bit % 8)
        rows.append(r)
    return np.concatenate([np.stack(rows), rng.integers(0, 256, (nrand, cb), dtype=np.uint8)])


N_SPECIAL = 9          # special codes / int8 rows at the head of a corpus
ZERO_ROW = 5           # the zero int8 row (-inf cosine)


def int8_rows(dim, nrand, seed=0):
    """int8 rows, zero at ``big_positions``: the three ``tie_rows``, two rows of -128 and +127 only (one of them with
    every other entry zero), the zero row, three random rows with -128 at every seventh dim, random."""
    rng = np.random.default_rng(53 * dim + seed)
    ext = rng.choice(np.array([-128, 127], np.int8), (2, dim))
    ext[1, 1::2] = 0
    ext[:, 0], ext[:, 1] = -128, 127
    more = rng.integers(-128, 128, (3, dim)).astype(np.int8)
    more[:, ::7] = -128
    x = np.concatenate([tie_rows(dim, seed), ext, np.zeros((1, dim), np.int8), more,
                        rng.integers(-128, 128, (nrand, dim)).astype(np.int8)])
    assert not x[ZERO_ROW].any() and x.shape[0] == N_SPECIAL + nrand
    keep = x[:3].copy()
    x[:, list(big_positions(dim))] = 0
    h = dim // 2
    for p in big_positions(dim):                       # keep the tie rows' halves cancelling
        x[:3, (p + h) % dim] = 0
    assert np.array_equal(x[:3, [40, h + 40]], keep[:, [40, h + 40]])
    return x


def float_rows(dim, nrand, seed=0):
    """float32 rows of the flat inner product, zero at ``big_positions``: the int8 rows as floats (integer
    weights: ``order_free(q, 128)`` applies to them), then standard-normal rows."""
    rng = np.random.default_rng(91 * dim + seed)
    x = np.concatenate([int8_rows(dim, 3, seed).astype(np.float32),
                        rng.standard_normal((nrand, dim)).astype(np.float32)])
    x[:, list(big_positions(dim))] = 0.0
    return x


def all_queries(dim, seed=0):
    """(float32[nq, dim], family letter of each query, meta)."""
    fam, meta = queries(dim, seed)
    return np.concatenate([fam[f] for f in FAMILIES]), [f for f in FAMILIES for _ in range(fam[f].shape[0])], meta
