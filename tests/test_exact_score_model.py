"""CPU checks of tests/exact_score_model.py: the roundings against Fraction, the restated summation orders
against the exact dot under ``order_free``, and the fixtures -- that they take the orders apart off the grid,
leave Phase III unambiguous, and tell wrong implementations (restated in NumPy) from right ones."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_score_model as M

NRAND = 12      # random rows next to the special ones, per dim


def _rn_brute(x, fmt):
    """Round to nearest, ties to even, by walking the format's neighbours of x and comparing exact distances."""
    f = np.dtype(fmt).type
    it = np.uint32 if fmt == "float32" else np.uint64
    fin = np.finfo(f)
    big = Fraction(float(fin.max))
    if abs(x) >= big + Fraction(2) ** (fin.maxexp - 1 - fin.nmant - 1):      # max + half an ulp
        return math.inf if x > 0 else -math.inf
    if abs(x) >= big:
        return float(fin.max) if x > 0 else -float(fin.max)
    below = f(float(x))                                  # (any rounding: only the start of the walk)
    while Fraction(float(below)) > x:
        below = np.nextafter(below, f(-np.inf))
    above = below
    while Fraction(float(above)) < x:
        above = np.nextafter(above, f(np.inf))
    dl, dh = x - Fraction(float(below)), Fraction(float(above)) - x
    if dl != dh:
        return float(below if dl < dh else above)
    return float(below if int(below.view(it)) % 2 == 0 else above)


def test_roundings_agree_with_fraction():
    rng = np.random.default_rng(1)
    xs = []
    for _ in range(300):                                # random rationals over many binades
        xs.append(Fraction(int(rng.integers(-2 ** 62, 2 ** 62)), int(rng.integers(1, 2 ** 62)))
                  * Fraction(2) ** int(rng.integers(-1100, 1000)))
    for e in (-1074, -1073, -1050, -1022, -150, -149, -148, -127, -126, -100, -1, 0, 1, 60, 127, 1023):
        for m in (1, 3, 5, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 25 - 1, 2 ** 53 - 1, 2 ** 53 + 1, 2 ** 54 - 1, 2 ** 54 + 3):
            base = Fraction(m) * Fraction(2) ** e
            xs += [base, -base, base / 2, base / 4, base + Fraction(2) ** (e - 70), base - Fraction(2) ** (e - 70)]
    for x in xs:
        if abs(x) < Fraction(2) ** 1023:                  # Python's int / int is correctly rounded too
            assert M.rn64(x) == float(x), x
        assert M.rn64(x) == _rn_brute(x, "float64"), x
        assert M.rn32(x) == _rn_brute(x, "float32"), x
    # exact half-ulp ties, to even, normal and subnormal; overflow at max + half an ulp
    assert M.rn32(1 + Fraction(1, 2 ** 24)) == 1.0
    assert M.rn32(1 + Fraction(3, 2 ** 24)) == 1.0 + 2.0 ** -22
    assert M.rn32(1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 200)) == 1.0 + 2.0 ** -23
    assert M.rn32(Fraction(1, 2 ** 150)) == 0.0 and M.rn32(Fraction(3, 2 ** 150)) == 2.0 ** -148
    assert M.rn32(-Fraction(5, 2 ** 150)) == -2.0 ** -148
    assert M.rn64(Fraction(1, 2 ** 1075)) == 0.0 and M.rn64(Fraction(3, 2 ** 1075)) == 2.0 ** -1073
    assert M.rn32(Fraction(2) ** 128 - Fraction(2) ** 103) == math.inf
    assert M.rn32(Fraction(2) ** 128 - Fraction(2) ** 103 - 1) == float(np.finfo(np.float32).max)
    # the double rounding the model must not make: 1 + 2^-24 + 2^-60 is above the tie, float() puts it on it
    x = 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert float(np.float32(float(x))) == 1.0 and M.rn32(x) == 1.0 + 2.0 ** -23


def _corpus(dim):
    return M.code_rows(dim, NRAND), M.int8_rows(dim, NRAND)


@pytest.mark.parametrize("dim", M.DIMS)
def test_fixtures_have_the_stated_shape(dim):
    Q, fam, meta = M.all_queries(dim)
    codes, x8 = _corpus(dim)
    a = Q[:3]
    for j, (wmax, E) in enumerate(zip(meta["a_wmax"], meta["a_E"])):
        assert M.order_free(a[j], wmax)
        floor = a[j].copy()                            # two binades below the floor the predicate fails: at the limit
        floor[1] = floor[1] * np.float32(0.25) if j < 2 else floor[1]
        if j < 2:
            assert not M.order_free(floor, wmax)
            assert np.abs(a[j]).max() == 1.0 and np.abs(a[j][a[j] != 0]).min() == 2.0 ** -E
    assert not M.order_free(a[0], 127)
    den = a[2]
    assert np.abs(den[den != 0]).min() == 2.0 ** -149 and (np.abs(den[den != 0]) < 2.0 ** -126).sum() > 10
    for j in range(3):
        assert (a[j] == 0).sum() == 2 and np.signbit(a[j][a[j] == 0]).sum() == 1      # +0.0 and -0.0
    for f in "bcd":
        for q in Q[[i for i, g in enumerate(fam) if g == f]]:
            assert not M.order_free(q, 1) and np.isfinite(q).all()
    p = M.big_positions(dim)
    assert len({v // 16 for v in p}) == 4 and len({(v % 128) // 2 for v in p}) == 4 and len({v // 4 for v in p}) == 4
    for q in Q[[i for i, g in enumerate(fam) if g == "d"]]:
        assert sorted(np.abs(q[list(p)])) == [M.A_BIG] * 4 and q[list(p)].sum() == 0
    assert not x8[:, list(p)].any() and (x8 == -128).any() and (x8 == 127).any() and not x8[M.ZERO_ROW].any()
    e0 = fam.index("e")
    for qi, r, want in M.TIE_EXPECT:                     # exact half-ulp ties of float32, to even
        y = M.exact_dot(Q[e0 + qi], x8[r])
        assert M.order_free(Q[e0 + qi], 128)
        lo, hi = np.nextafter(np.float32(want), np.float32(0)), np.nextafter(np.float32(want), np.float32(2))
        assert y in ((Fraction(float(lo)) + Fraction(want)) / 2, (Fraction(float(hi)) + Fraction(want)) / 2)
        assert M.rn32(y) == want
    f0 = fam.index("f")
    assert M.exact_dot(Q[f0], x8[2]) == 0 and M.abs_dot(Q[f0], x8[2]) > 1
    assert M.phase3_values(Q[f0], x8[2], M.int8_norm(x8[2]), bound=0) == [0.0]
    assert M.phase3_values(Q[0], x8[M.ZERO_ROW], 0.0) == [-np.inf]
    for v in (0, 7, 8, dim - 1):
        assert any(np.array_equal(np.flatnonzero(np.unpackbits(c)), [v]) for c in codes)


@pytest.mark.parametrize("dim", M.DIMS)
def test_orders_equal_the_exact_dot_when_order_free(dim):
    Q, fam, meta = M.all_queries(dim)
    codes, x8 = _corpus(dim)
    n2 = n3 = 0
    for qi, q in enumerate(Q):
        ex2, ex3 = M.exact_dots(q, codes), M.exact_dots(q, x8)
        ab3 = M.exact_dots(q, x8, absolute=True)
        for name, fn in M.orders_for(dim).items():
            s2 = fn(M.products(q, codes))
            if M.order_free(q, 1):
                assert [Fraction(float(v)) for v in s2] == ex2, (name, fam[qi])
                n2 += 1
            if name != "nibble":
                s3 = fn(M.products(q, x8))
                if M.order_free(q, 128):
                    assert [Fraction(float(v)) for v in s3] == ex3, (name, fam[qi])
                    n3 += 1
                for r in range(x8.shape[0]):            # and off the grid every order stays inside the bound
                    assert abs(Fraction(float(s3[r])) - ex3[r]) <= M.gamma(dim - 1) * ab3[r]
    assert n2 >= 6 and n3 >= 5                         # (a) x 3 + (e) x 2 + (f); (a)[0] is free for +-1 only
    # exact_dot, one pair at a time and on float32 rows, agrees with the batched form
    xf = M.float_rows(dim, 2)
    assert M.exact_dot(Q[3], x8[7]) == M.exact_dots(Q[3], x8)[7]
    assert M.exact_dot(Q[3], xf[7]) == M.exact_dots(Q[3], x8)[7] or not np.array_equal(xf[7], x8[7].astype(np.float32))
    assert M.exact_dot(Q[0], xf[0]) == M.exact_dot(Q[0], M.int8_rows(dim, 3)[0])
    t = M.products(Q[4], xf[-1])
    assert abs(Fraction(float(M.order_sequential(t))) - M.exact_dot(Q[4], xf[-1])) <= M.sum_bound(Q[4], xf[-1])


# Off the grid the wave order and the nibble order of the library differ in the last bits of s2.  Shares of the
# 42 pairs (2 queries x the 21 codes of _corpus) measured with these fixtures over the seven dims: (b) 0.74 - 0.93,
# (c) 0.71 - 0.98, (d) 0.48 - 0.71; asserted with slack.  150 random pairs at 1024 (the next test): 0 for
# standard-normal queries, 132 for (b), 131 for (c).
MIN_DISAGREE = {"b": 0.6, "c": 0.6, "d": 0.35}


@pytest.mark.parametrize("dim", M.DIMS)
def test_off_grid_families_split_the_orders(dim):
    Q, fam, _ = M.all_queries(dim)
    codes, _ = _corpus(dim)
    wave = M.order_wave1024 if dim == 1024 else M.order_wave_dim
    for f, floor in MIN_DISAGREE.items():
        idx = [i for i, g in enumerate(fam) if g == f]
        differ = total = 0
        for i in idx:
            t = M.products(Q[i], codes)
            differ += int((wave(t) != M.order_nibble(t)).sum())
            total += codes.shape[0]
        print(f"dim {dim} family {f}: wave and nibble order differ on {differ} of {total} pairs")
        assert differ >= floor * total, (f, differ, total)


def test_random_pairs_at_1024_split_like_the_issue_measured():
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 256, (150, 128), dtype=np.uint8)
    g = rng.standard_normal((150, 1024))
    fams = {"normal": g, "b": np.where(rng.random((150, 1024)) < 0.5, g * 1e-9, g),
            "c": g * np.exp(rng.normal(0, 8, (150, 1024)))}
    got = {}
    for name, q in fams.items():
        t = M.products(q.astype(np.float32), codes)     # pair i: query i, code i
        got[name] = int((M.order_wave1024(t) != M.order_nibble(t)).sum())
    print(got)
    assert got["normal"] <= 5 and got["b"] >= 110 and got["c"] >= 110


@pytest.mark.parametrize("dim", M.DIMS)
def test_reference_leaves_phase3_unambiguous(dim):
    """A condition on the fixtures, not a tolerance: [exact - sum_bound, exact + sum_bound] holds a float32
    rounding boundary on at most 1 % of the pairs of every family (int8 rows and float32 rows)."""
    Q, fam, _ = M.all_queries(dim)
    _, x8 = _corpus(dim)
    xf = M.float_rows(dim, 4)[-4:]
    for f in M.FAMILIES:
        two = total = 0
        for i in [i for i, g in enumerate(fam) if g == f]:
            ex, ab = M.exact_dots(Q[i], x8), M.exact_dots(Q[i], x8, absolute=True)
            free = M.order_free(Q[i], 128)
            for r in range(x8.shape[0]):
                b = 0 if free else M.gamma(dim - 1) * ab[r]
                vals = M.phase3_values(Q[i], x8[r], M.int8_norm(x8[r]), exact=ex[r], bound=b)
                assert vals is not None and 1 <= len(vals) <= 2
                two += len(vals) == 2
                total += 1
            for x in xf:
                vals = M.phase3_values(Q[i], x, None)
                assert vals is not None and 1 <= len(vals) <= 2
                two += len(vals) == 2
                total += 1
        assert two <= 0.01 * total, (f, two, total)


# ----------------------------------------------------------------------------- wrong implementations
def _outside(got, exact, bound):
    return [abs(Fraction(float(g)) - e) > b for g, e, b in zip(got, exact, bound)]


def _facts(q, W):
    ex, ab = M.exact_dots(q, W), M.exact_dots(q, W, absolute=True)
    wmax = 1 if W.dtype == np.uint8 else 128
    free = M.order_free(q, wmax)
    return ex, [0 if free else M.gamma(q.shape[0] - 1) * a for a in ab]


def _caught(dim, wrong, rows, queries=None):
    """Pairs (query, row) on which ``wrong(q, rows) -> float64[R]`` leaves sum_bound (0 under order_free)."""
    Q, fam, _ = M.all_queries(dim)
    hits = []
    for i, q in enumerate(Q):
        if queries and fam[i] not in queries:
            continue
        ex, bd = _facts(q, rows)
        hits += [(fam[i], r) for r, out in enumerate(_outside(wrong(q, rows), ex, bd)) if out]
    return hits


@pytest.mark.parametrize("dim", M.DIMS)
def test_fixtures_catch_wrong_variants(dim):
    codes, x8 = _corpus(dim)
    wave = M.order_wave1024 if dim == 1024 else M.order_wave_dim
    # the right orders pass everywhere (the control of this test)
    for fn in M.orders_for(dim).values():
        assert not _caught(dim, lambda q, W: fn(M.products(q, W)), codes)
    assert not _caught(dim, lambda q, W: wave(M.products(q, W)), x8)

    def f32_acc(q, W):
        t = M.products(q, W).astype(np.float32)
        return np.add.accumulate(t, axis=-1, dtype=np.float32)[..., -1].astype(np.float64)
    hits = _caught(dim, f32_acc, x8)
    assert {f for f, _ in hits} >= {"a", "b", "c"}, "float32 accumulation"
    assert _caught(dim, f32_acc, codes)

    def flushed(q, W):
        qq = q.copy()
        qq[np.abs(qq) < np.finfo(np.float32).tiny] = 0.0
        return wave(M.products(qq, W))
    assert {f for f, _ in _caught(dim, flushed, codes)} == {"a"} and _caught(dim, flushed, x8, "a")

    def plus128(q, W):
        t = M.products(q, W)
        qq = np.asarray(q, np.float64)
        return wave(np.where(W == -128, 128.0 * qq, t))
    assert {f for f, _ in _caught(dim, plus128, x8, "aef")} == {"a", "e", "f"}

    def reversed_nibble(q, W):
        bits = np.unpackbits(W, axis=-1).reshape(W.shape[0], -1, 4)[..., ::-1].reshape(W.shape[0], -1)
        return M.order_nibble(M.products(q, np.packbits(bits, axis=-1)))
    hits = _caught(dim, reversed_nibble, codes)
    assert {f for f, _ in hits} == set(M.FAMILIES)
    # 0x00, 0xFF, 0xA5 ... are nibble palindromes or not: the single bits and 0xA5 must be among the catches
    assert {6, 7, 8}.issubset({r for _, r in hits}) or {5, 6, 7}.issubset({r for _, r in hits})

    if (dim // 8) % 64:          # 16, 32, 48, 96 code bytes; 192 = 3 x 64 has no short pass
        def short_pass_dropped(q, W):
            return M.order_nibble(M.products(q, W), drop_short_last=True)
        assert {f for f, _ in _caught(dim, short_pass_dropped, codes)} == set(M.FAMILIES)

    # truncation instead of rounding to float32: the value leaves phase3_values
    Q, fam, _ = M.all_queries(dim)
    missed = 0
    for i, q in enumerate(Q):
        ex, bd = _facts(q, x8)
        s = wave(M.products(q, x8))
        for r in range(x8.shape[0]):
            if r == M.ZERO_ROW:
                continue
            f = np.float32(s[r])
            if abs(np.float64(f)) > abs(s[r]):          # rounded away from zero: truncation steps back
                f = np.nextafter(f, np.float32(0))
            nrm = M.int8_norm(x8[r])
            vals = M.phase3_values(q, x8[r], nrm, exact=ex[r], bound=bd[r])
            assert float(np.float64(np.float32(s[r])) / nrm) in vals      # the right rounding is inside
            missed += float(np.float64(f) / nrm) not in vals
    assert missed >= 0.3 * len(Q) * (x8.shape[0] - 1)
    e0 = fam.index("e")                                 # the tie that rounds up to even: truncation gives the odd one
    s = float(wave(M.products(Q[e0 + 1], x8[1:2]))[0])
    assert s == 1.0 + 3 * 2.0 ** -24 and float(np.float32(s)) == 1.0 + 2.0 ** -22
