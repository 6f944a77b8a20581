"""Pure-NumPy model of K5's pruning rule (gemm_topk.hip: vrq_gemm_topk / vrq_flat_ip_topk) and the
adversarial inputs that make its proof's worst case real.  Test infrastructure only, no product code.

The rule, in float64 (d = 1024):
  1. pieces   q/S = a + rho, S = max|q| / 127, a = clip(rint(q/S), +-127)
  2. Delta    a per-query bound on |u - s'| over all rows (u: the matrix-core value <a, x> [/ ||x||],
              s': the reference score in the same units), the formulas of the kernel's header comment
  3. U        the k-th largest u (here over all rows: at n <= 8192 the sample is the whole corpus)
  4. thr      U - 2 Delta; a row with u < thr is never rescored
Every row of the exact top-k (ties with the k-th included: the "must" rows) has to pass step 4.

Fixtures (``fixture(name)``): the queries have max|q| = 127, so S = 1 and q/S = q exactly.
  binary_sym / binary_asym   Phase II, sum rho+ = sum rho- (500 / 500 dims) and 600 / 400 dims
  int8_cosine                Phase III
  float_ip                   IndexFlatIP rows with their own quantisation residual
Each holds k identical "winner" rows whose u overstates s' by nearly Delta (they set U) and one
"victim" row, the true best, whose u understates s' by nearly Delta.
"""
import numpy as np

D = 1024
SLACK = 2.0 ** -20
MODES = ("binary", "int8_cosine", "float_ip")


# ------------------------------------------------------------------------------------------------
# the prep kernel restated
def prep_reference(mode, qf, bounds=None, scale=1.0, one_sided=max):
    """-> dict(a int8[nq, D] natural order, rho, delta, alpha, beta, inv_s), all float64.  ``scale``
    multiplies Delta and ``one_sided`` (max / min) picks between the Phase-II one-sided sums: the
    mutations the CPU test of the fixtures applies."""
    q = np.asarray(qf, np.float32).astype(np.float64)
    mx = np.abs(q).max(axis=1)
    inv_s = np.where(mx > 0, 127.0 / np.where(mx > 0, mx, 1.0), 1.0)
    x = q * inv_s[:, None]
    a = np.clip(np.rint(x), -127.0, 127.0)
    rho = x - a
    r2 = (rho * rho).sum(1)
    rp = np.where(rho > 0, rho, 0.0).sum(1)
    rn = np.where(rho < 0, -rho, 0.0).sum(1)
    q2 = (q * q).sum(1)
    q1 = np.abs(q).sum(1)
    qs = q.sum(1)
    if mode == "binary":
        side = np.array([one_sided(p, m) for p, m in zip(rp, rn)])
        delta = side * (1.0 + SLACK) + SLACK * q1 * inv_s
        alpha, beta = 0.5 * inv_s, 0.5 * inv_s * qs
    elif mode == "float_ip":
        qn, rnorm, bx, bs = np.sqrt(q2) * inv_s, np.sqrt(r2), float(bounds[0]), float(bounds[1])
        delta = (rnorm * bx + qn * bs) * (1.0 + SLACK) + SLACK * (qn + rnorm) * bx
        alpha, beta = inv_s, np.zeros_like(inv_s)
    else:
        delta = np.sqrt(r2) * (1.0 + SLACK) + SLACK * np.sqrt(q2) * inv_s
        alpha, beta = inv_s, np.zeros_like(inv_s)
    return dict(a=a.astype(np.int8), rho=rho, delta=delta * scale, alpha=alpha, beta=beta, inv_s=inv_s,
                beta_tol=1e-12 * 0.5 * inv_s * q1)


def flat_prepare_reference(F):
    """vrq_flat_ip_prepare restated: (b int8[n, D], s f64[n] the row scales, bounds f64[2])."""
    x = np.asarray(F, np.float32).astype(np.float64)
    mx = np.abs(x).max(axis=1)
    live = mx >= 1e-30
    inv = np.where(live, 127.0 / np.where(live, mx, 1.0), 0.0)
    s = np.where(live, mx / 127.0, 0.0)
    b = np.clip(np.rint(x * inv[:, None]), -127.0, 127.0)
    bx = (s * np.sqrt((b * b).sum(1))).max()
    bs = np.sqrt(((x - s[:, None] * b) ** 2).sum(1)).max()
    return b.astype(np.int8), s, np.array([bx, bs])


def bits_of(codes):
    """u8[n, 128] -> f64[n, 1024] 0/1 in np.unpackbits order (the oracle's)."""
    return np.unpackbits(np.asarray(codes, np.uint8), axis=1).astype(np.float64)


def matrix_values(mode, a, codes=None, x8=None, scales=None):
    """u of every (query, row) in float64: <a, bits>, <a, x> / ||x|| (NaN for a zero norm), or
    s_r <a, b_r>."""
    a = np.asarray(a, np.float64)
    if mode == "binary":
        return a @ bits_of(codes).T
    A = a @ np.asarray(x8, np.float64).T
    if mode == "float_ip":
        return A * np.asarray(scales, np.float64)[None, :]
    nrm = np.sqrt((np.asarray(x8, np.float64) ** 2).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = A / nrm[None, :]
    u[:, nrm == 0] = np.nan
    return u


def scores_u_units(mode, qf, prep, codes=None, x8=None, F=None):
    """s' of every (query, row) in float64: the reference score mapped to u units without the
    reference's own float32 rounding (Phase II (s + sum q) / (2S) = <q/S, bits>; Phase III
    <q/S, x> / ||x||; float-IP <q/S, x>)."""
    x = np.asarray(qf, np.float32).astype(np.float64) * prep["inv_s"][:, None]
    if mode == "binary":
        return x @ bits_of(codes).T
    if mode == "float_ip":
        return x @ np.asarray(F, np.float32).astype(np.float64).T
    X = np.asarray(x8, np.float64)
    nrm = np.sqrt((X * X).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (x @ X.T) / nrm[None, :]
    s[:, nrm == 0] = -np.inf
    return s


def kth_largest(v, k):
    """k-th largest non-NaN value of a vector, -inf when it holds fewer than k."""
    v = np.asarray(v, np.float64)
    v = np.sort(v[~np.isnan(v)])[::-1]
    return v[k - 1] if v.size >= k else -np.inf


def round_down_f32(x):
    """float64 -> the largest float32 <= x."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
    up = f.astype(np.float64) > x
    return np.where(up, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def float_key(v):
    """The select kernel's monotone u32 key of float32 values (NaN -> 0, below -inf)."""
    b = np.asarray(v, np.float32).view(np.uint32)
    key = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    return np.where((b & 0x7FFFFFFF) > 0x7F800000, 0, key).astype(np.uint32)


def model_keeps(fx, scale=1.0, one_sided=max, thr_mult=2.0):
    """The four steps on a fixture -> (kept bool[nq, n], must bool[nq, n], ratio f64[nq]): the rows that
    pass the threshold, the rows of the exact top-k (ties with the k-th included), and the achieved
    max|u - s'| / Delta over the rows with a score."""
    mode, k = fx["mode"], fx["k"]
    prep = prep_reference(mode, fx["qf"], fx.get("bounds"), scale, one_sided)
    u = matrix_values(mode, prep["a"], fx.get("codes"), fx.get("x8"), fx.get("scales"))
    sp = scores_u_units(mode, fx["qf"], prep, fx.get("codes"), fx.get("x8"), fx.get("F"))
    nq = u.shape[0]
    kept, must, ratio = np.zeros(u.shape, bool), np.zeros(u.shape, bool), np.zeros(nq)
    for q in range(nq):
        thr = kth_largest(u[q], k) - thr_mult * prep["delta"][q]
        kept[q] = u[q] >= thr                      # NaN (zero norm): never kept
        must[q] = sp[q] >= kth_largest(sp[q], k)
        fin = ~np.isnan(u[q]) & np.isfinite(sp[q])
        ratio[q] = np.abs(u[q][fin] - sp[q][fin]).max() / prep["delta"][q]
    return kept, must, ratio


# ------------------------------------------------------------------------------------------------
# adversarial fixtures
ANCHOR = 0                       # q = 127: max|q| = 127, so S = 1
TWENTY = np.arange(1, 24)        # 23 dims at 20.0 (rho = 0)
RES = np.arange(24, 1024)        # 1000 dims at +-0.45 (a = 0, rho = +-0.45)
N_FIX, K_FIX = 4096, 10
WINNERS = np.arange(1500, 1500 + K_FIX)   # k identical rows, not at a chunk's edge
VICTIM = 3333


def _pack(bits):
    return np.packbits(bits.astype(np.uint8), axis=1)


def _binary_fixture(npos, seed):
    rng = np.random.default_rng(seed)
    sig = np.ones(1000)
    sig[npos:] = -1.0
    sig = sig[rng.permutation(1000)]             # npos dims at +0.45, the rest at -0.45, interleaved
    q = np.zeros(D)
    q[ANCHOR], q[TWENTY], q[RES] = 127.0, 20.0, 0.45 * sig
    bits = np.zeros((N_FIX, D), np.uint8)
    for r in range(N_FIX):                       # filler: at most 5 of the 20-dims, random residual dims
        bits[r, rng.choice(TWENTY, rng.integers(0, 6), replace=False)] = 1
    bits[:, RES] = rng.integers(0, 2, (N_FIX, 1000))
    bits[WINNERS] = 0
    bits[np.ix_(WINNERS, TWENTY[:22])] = 1       # u = 440, s' = 440 - 0.45 * (1000 - npos)
    bits[np.ix_(WINNERS, RES[sig < 0])] = 1
    bits[VICTIM] = 0
    bits[VICTIM, RES[sig > 0]] = 1               # u = 0, s' = 0.45 * npos: the true best row
    qf = np.stack([q, -q]).astype(np.float32)    # (-q: the mirrored roles; its top-k is the filler's)
    return dict(mode="binary", k=K_FIX, qf=qf, codes=_pack(bits), victim=VICTIM, winners=WINNERS)


def _int8_rows(rng, sig):
    x = rng.integers(-3, 4, (N_FIX, D))
    x[:, ANCHOR] = 0
    x[::97] = 0                                   # a few zero-norm rows (u NaN, score -inf)
    w = np.zeros(D)
    w[TWENTY], w[RES] = 10, -4 * sig              # u = 34.0, s' = 20.7
    v = np.zeros(D)
    v[TWENTY], v[RES] = 2, 4 * sig                # u = 7.25, s' = 21.4: the true best row
    x[WINNERS], x[VICTIM] = w, v
    return x


def _query3(rng):
    sig = rng.choice([-1.0, 1.0], 1000)
    q = np.zeros(D)
    q[ANCHOR], q[TWENTY], q[RES] = 127.0, 20.0, 0.45 * sig
    return q, sig


def _cosine_fixture(seed):
    rng = np.random.default_rng(seed)
    q, sig = _query3(rng)
    x = _int8_rows(rng, sig)
    return dict(mode="int8_cosine", k=K_FIX, qf=q[None].astype(np.float32), x8=x.astype(np.int8), victim=VICTIM,
                winners=WINNERS)


def _float_fixture(seed):
    """Rows b + e with b the int8 image flat_ip_prepare recovers (every row holds 127 at the anchor,
    so its scale is 1) and e = +-0.45 sign(q) the row's own quantisation residual: the victim's adds to
    its score, the winners' subtracts.  Row 7 has 8 times the norm (scale 8) and a negative score."""
    rng = np.random.default_rng(seed)
    q, sig = _query3(rng)
    b = _int8_rows(rng, sig).astype(np.float64)
    b[::97] = rng.integers(-3, 4, (len(b[::97]), D))
    b[:, ANCHOR] = 100.0                          # filler: scale 100 / 127, scores far below the winners'
    e = np.zeros((N_FIX, D))
    sq = np.sign(q)
    sq[ANCHOR] = 0.0
    b[WINNERS, ANCHOR] = b[VICTIM, ANCHOR] = 127.0
    e[WINNERS], e[VICTIM] = -0.45 * sq, 0.45 * sq
    F = b + e
    F[7] = 8.0 * (b[VICTIM] + e[VICTIM])
    F[7, ANCHOR] = -8.0 * 127.0
    F = F.astype(np.float32)
    x8, scales, bounds = flat_prepare_reference(F)
    return dict(mode="float_ip", k=K_FIX, qf=q[None].astype(np.float32), F=F, x8=x8, scales=scales, bounds=bounds,
                victim=VICTIM, winners=WINNERS)


FIXTURES = ("binary_sym", "binary_asym", "int8_cosine", "float_ip")
_cache = {}


def fixture(name):
    """One adversarial fixture (built once, shared; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = {"binary_sym": lambda: _binary_fixture(500, 41), "binary_asym": lambda: _binary_fixture(600, 42),
                        "int8_cosine": lambda: _cosine_fixture(43), "float_ip": lambda: _float_fixture(44)}[name]()
        for v in _cache[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _cache[name]


# ------------------------------------------------------------------------------------------------
# select-kernel inputs: Phase-II corpora whose matrix-core values are chosen integers
W127 = 516                       # dims of weight 127; the other 508 have weight 1


def value_query():
    """q with a = q: u = 127 * p + j for a row with p of the first 516 and j of the last 508 dims set."""
    q = np.ones(D, np.float32)
    q[:W127] = 127.0
    return q


def rows_for_values(v):
    """Packed codes whose u under value_query() are the integers v (0 <= v <= 66040)."""
    v = np.asarray(v, np.int64)
    assert v.min() >= 0 and v.max() <= 127 * W127 + (D - W127)
    p = np.minimum(v // 127, W127)
    j = v - 127 * p
    assert j.max() <= D - W127
    bits = np.zeros((v.size, D), np.uint8)
    bits[:, :W127] = np.arange(W127)[None, :] < p[:, None]
    bits[:, W127:] = np.arange(D - W127)[None, :] < j[:, None]
    return _pack(bits)


def select_values(case, n, seed=0):
    """Target u of n rows for one radix-select case (the queries of a case: +value_query, its negation
    and the zero query).
      top22   1100 rows in one aligned block of 8 integers at 65536 (one value of the low 10 key bits'
              range), the rest spread below: > k rows share the top 22 key bits of U for every k <= 1024
      top11   2000 rows spread over [32768, 40960) (one value of the top 11 key bits), the rest below:
              the second pass decides
      equal   every row the same value
    """
    rng = np.random.default_rng(seed)
    if case == "top22":
        v = rng.integers(1, 65000, n)
        v[rng.permutation(n)[:1100]] = 65536 + np.arange(1100) % 8
    elif case == "top11":
        v = rng.integers(1, 32768, n)
        v[rng.permutation(n)[:2000]] = rng.integers(32768, 40960, 2000)
    else:
        v = np.full(n, 40000)
    return v
