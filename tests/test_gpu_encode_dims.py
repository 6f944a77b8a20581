"""GPU parity of the encoders (``vrq_encode``) at the dims whose pairwise-sum plans the rest of the suite
never reaches: the second and later passes of ``pairwise_sum_f32``'s batch loop (more than 8 leaves:
1032, 1536, 2048, 2056, 4096, 8192) and its LDS stack fold (every unbalanced plan, 264 being the smallest),
next to the one-leaf, the balanced and the dedicated d = 1024 paths.  ``pairwise_model.plan_shape`` decides
what a dim exercises, and the dim list is asserted to cover every shape.

Codes, quantised values and (min, max) are compared bit for bit with the NumPy oracle (oracle/oracle_np.py;
tests/binary_oracle.py for ``sbin``) -- no tolerance anywhere.  The inputs are made so that a slightly
wrong mean changes a code bit: the near-mean rows hold 32 elements within 16 ulp of the row's float32
mean, and a CPU check (it runs before any GPU call, and on its own in the CPU suite) shows that the codes
of a sequential float32 sum, and of the right leaf sums folded in the wrong order, differ from NumPy's on
most of them."""
import functools

import numpy as np
import pytest
import torch

import binary_oracle as B
import pairwise_model as P
from oracle import oracle_np as O

gpu = pytest.mark.gpu

DIMS = (16, 136, 264, 512, 1024, 1032, 1536, 2048, 2056, 4096, 8192)
BIN16_DIMS = (16, 264, 1024, 1536, 8192)
MODES = ("int8g", "int16g", "int4g", "int8", "int4", "cohere", "sbin")
GLOBAL_MODES = ("int8g", "int16g", "cohere")            # the modes that use their limit
DENORMAL_MODES = ("int8g", "int16g", "cohere", "sbin")  # no 127 / max|x| (inf for a denormal row)
LIMITS = (0.3, 0.1, 1.0)
N_RANDOM, N_NEAR = 27, 40
# sensitivity floors of the near-mean rows, out of N_NEAR (these inputs reach 35-40 and 9-27)
MIN_SEQUENTIAL, MIN_LEFT_FOLD = 30, 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


# ----------------------------------------------------------------------------- inputs
def _random_rows(rng, n, d):
    """Per-row scales 0.01 .. 2.0 and a per-row offset of +-(0.05 .. 0.5): the mean is well away from 0 (so
    the sign codes of ``cohere`` differ from the mean codes) and the partial sums round at every step.
    The offset is independent of the scale: some rows are dominated by it (leaf sums of one sign and
    size), others by their spread (leaf sums of either sign)."""
    off = rng.uniform(0.05, 0.5, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    return (rng.standard_normal((n, d)) * rng.uniform(0.01, 2.0, (n, 1)) + off).astype(np.float32)


def _ulp_steps(m, ks):
    """m + k ulp(m) for every k, float32 (exact in float64 before the cast)."""
    m = np.float32(m)
    return (np.float64(m) + np.asarray(ks, np.float64) * np.float64(np.spacing(np.abs(m)))).astype(np.float32)


def _near_mean_rows(rng, n, d):
    """Random rows in which 32 slots (d / 2 at d < 64) hold mean + k ulp, k = -16 .. 15: a fixed-point
    iteration (recompute np.mean, plant again) until the mean stops moving.

    Every other row (every row at d < 128) also holds one cancelling pair +A, -A, A = 2^6 .. 2^10 standard
    deviations, at two random slots.  The pair leaves the mean where it was, but every sum that meets A
    before -A rounds to ulp(A) in between, far above the ulp of the final sum: any change of the
    association then moves the mean by many ulp.  Without it two associations of a short row agree too
    often to tell them apart (16 random elements: sequential and pairwise sums agree on 4 rows of 10)."""
    X = _random_rows(rng, n, d)
    ns = min(32, d // 2)
    ks = np.arange(-(ns // 2), ns // 2)
    for i, x in enumerate(X):
        slots = rng.choice(d, ns + 2, replace=False)
        if i % 2 == 1 or d < 128:
            a = np.float32(np.std(x) * 2.0 ** rng.integers(6, 11))
            x[slots[-2]], x[slots[-1]] = a, -a
        slots = slots[:ns]
        prev = None
        for _ in range(64 if d < 256 else 12):
            m = np.mean(x)
            if prev is not None and m == prev:
                break
            x[slots] = _ulp_steps(m, ks)
            prev = m
    return X


def _tie_values(limit):
    """+-limit and its float32 neighbours, values far outside, and the half-way points (k + 0.5) / scale
    of the int8 and int16 global quantisers with the two float32 neighbours on each side."""
    lim = np.float32(limit)
    v = [lim, -lim, np.nextafter(lim, np.float32(np.inf)), np.nextafter(lim, np.float32(0)),
         np.nextafter(-lim, np.float32(-np.inf)), np.nextafter(-lim, np.float32(0)),
         np.float32(2 * limit), np.float32(-2 * limit)]
    for top in (127.0, 32767.0):
        scale = np.float32(top / limit)
        for k in (0, 1, 2, int(top) // 2, int(top) - 2, int(top) - 1):
            x = np.float32((k + 0.5) / np.float64(scale))
            for _ in range(2):
                x = np.nextafter(x, np.float32(0))
            for _ in range(5):
                v += [x, -x]
                x = np.nextafter(x, np.float32(np.inf))
    return np.asarray(v, np.float32)


def _limit_rows(rng, d):
    """Rows holding the tie values of every limit (as many rows as they need at this dim), the rest random
    inside the smallest limit; four more slots hold +-1e30 and +-1e38."""
    v = np.concatenate([_tie_values(lim) for lim in LIMITS])
    nrows = -(-(v.size + 4) // d)
    R = rng.uniform(-0.1, 0.1, (nrows, d)).astype(np.float32)
    flat = R.reshape(-1)
    pos = rng.choice(flat.size, v.size + 4, replace=False)
    flat[pos[:v.size]] = v
    flat[pos[v.size:]] = np.asarray([1e30, -1e30, 1e38, -1e38], np.float32)
    return R


def _edge_rows(rng, d):
    rows = [np.full((1, d), 0.25, np.float32)]                           # flat: min == max
    h = np.ones((1, d), np.float32)
    h[0, d // 2:] = -1.0                                                 # +-1.0 halves, mean 0
    rows.append(h)
    rows.append(np.round(_random_rows(rng, 1, d) * 8) / 8)               # multiples of 1/8
    rows.append(_limit_rows(rng, d))
    rows.append(_random_rows(rng, 1, d) * np.float32(1e-30))
    rows.append(_random_rows(rng, 1, d) * np.float32(1e30))
    z = np.zeros((2, d), np.float32)
    z[:, rng.random(d) < 0.5] = -0.0                                     # +0.0 / -0.0: flat, mean +-0
    z[1, rng.choice(d, max(2, d // 8), replace=False)] = rng.choice([-1e-3, 1e-3], max(2, d // 8))
    rows.append(z)
    return np.concatenate(rows).astype(np.float32)


def _denormal_row(rng, d):
    """Every element denormal, 1e-40 .. 9e-40, and so is the mean: about half the bits are set."""
    return (rng.integers(1, 10, (1, d)) * 1e-40).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(d):
    """-> dict(random, near, edge, denormal), built once per dim and shared read-only."""
    rng = np.random.default_rng(1000 + d)
    parts = dict(random=_random_rows(rng, N_RANDOM, d), near=_near_mean_rows(rng, N_NEAR, d),
                 edge=_edge_rows(rng, d), denormal=_denormal_row(rng, d))
    for v in parts.values():
        assert np.isfinite(v).all()
        v.setflags(write=False)
    return parts


@functools.lru_cache(maxsize=None)
def _batch(d, denormal):
    p = _inputs(d)
    X = np.concatenate([p["random"], p["near"], p["edge"]] + ([p["denormal"]] if denormal else []))
    X.setflags(write=False)
    return X


def _row_kind(d, r):
    p = _inputs(d)
    for name in ("random", "near", "edge", "denormal"):
        if r < p[name].shape[0]:
            return f"{name}[{r}]"
        r -= p[name].shape[0]
    return "?"


# ----------------------------------------------------------------------------- reference
def _codes_of_sums(X, sums, ge=False):
    m = P.mean_of_sum(sums, X.shape[1])[:, None]
    return np.packbits(X >= m if ge else X > m, axis=1)


@functools.lru_cache(maxsize=None)
def _reference(mode, d, limit):
    X = _batch(d, mode in DENORMAL_MODES)
    if mode == "sbin":
        return B.sbin_codes(X), None, None
    return O.encode_batch(mode, X, limit)


@functools.lru_cache(maxsize=None)
def _check_sensitivity(d):
    """The condition on the inputs, on the CPU: the near-mean rows tell a wrong mean from np.mean.
    Returns (rows whose codes a sequential sum changes, rows whose codes a left fold of the leaf sums
    changes), out of N_NEAR."""
    X = _inputs(d)["near"]
    ref = np.stack([O.to_binary(x) for x in X])
    assert np.array_equal(_codes_of_sums(X, P.replay(X)), ref)            # the model is the oracle's mean
    near = [(np.abs(x.astype(np.float64) - np.float64(np.mean(x))) <= 24 * np.spacing(np.abs(np.mean(x)))).sum()
            for x in X]
    assert min(near) >= min(32, d // 2), "the planted slots are not within 24 ulp of the final mean"
    seq = int((_codes_of_sums(X, P.sum_sequential(X)) != ref).any(axis=1).sum())
    fold = int((_codes_of_sums(X, P.sum_leaves_left_fold(X)) != ref).any(axis=1).sum())
    print(f"d={d}: codes differ from np.mean's on {seq} (sequential) / {fold} (left fold) of {N_NEAR} rows")
    assert seq >= MIN_SEQUENTIAL, (d, seq)
    if P.plan_shape(d)[0] >= 3:
        assert fold >= MIN_LEFT_FOLD, (d, fold)
    # the other parts: offsets keep the sign codes apart from the mean codes; the denormal row has a
    # denormal mean that splits it (a flush to zero anywhere would set every bit, or none)
    R = _inputs(d)["random"]
    apart = sum(not np.array_equal(O.to_binary(x), O.to_binary_sign(x)) for x in R)
    assert apart >= N_RANDOM // 2, apart
    dn = _inputs(d)["denormal"][0]
    m = np.mean(dn)
    assert 0 < m < np.finfo(np.float32).tiny and dn.max() < np.finfo(np.float32).tiny
    ones = int(np.unpackbits(O.to_binary(dn)).sum())
    assert d // 4 <= ones <= 3 * d // 4, ones
    return seq, fold


def _explain(d, X, got, ref):
    """Which rows' codes differ, and whether a known wrong sum explains them."""
    bad = np.flatnonzero((got != ref).any(axis=1))
    seq = _codes_of_sums(X[bad], P.sum_sequential(X[bad]))
    fold = _codes_of_sums(X[bad], P.sum_leaves_left_fold(X[bad]))
    out = []
    for i, r in enumerate(bad[:12]):
        why = " and ".join(name for name, c in (("leaf sums folded left to right", fold[i]), ("sequential sum", seq[i]))
                           if np.array_equal(got[r], c)) or "neither known wrong sum"
        out.append(f"row {r} ({_row_kind(d, r)}): {int(np.unpackbits(got[r] ^ ref[r]).sum())} bits, {why}")
    return f"{bad.size} rows differ at d={d}, plan {P.plan_shape(d)[:2]}: " + "; ".join(out)


# ----------------------------------------------------------------------------- the conditions, on the CPU
def test_dims_cover_every_plan_shape():
    """One leaf; balanced with unequal (and equal) leaves; the stack fold within one batch; a second batch
    with 1 leaf (9), full (16) and with one more (17); 4 and 8 batches."""
    covered = set().union(*(P.shape_classes(d) for d in DIMS))
    assert covered == P.ALL_SHAPE_CLASSES, P.ALL_SHAPE_CLASSES - covered
    shapes = {d: P.plan_shape(d) for d in DIMS}
    assert shapes[16][:2] == (1, 0)
    assert shapes[136][:2] == (2, 1) and len(set(shapes[136][2])) == 2
    assert shapes[264][:2] == (3, -1)
    assert [shapes[d][0] for d in (1032, 1536, 2048, 2056, 4096, 8192)] == [9, 16, 16, 17, 32, 64]
    assert all(shapes[d][1] == -1 for d in (1032, 1536, 2048, 2056, 4096, 8192))
    assert max(d for d in DIMS) == P.MAX_DIM


@pytest.mark.parametrize("d", DIMS)
def test_near_mean_rows_tell_means_apart(d):
    _check_sensitivity(d)


@pytest.mark.parametrize("d", (16, 1536))
def test_limit_rows_hold_exact_ties(d):
    """The edge rows hold, for every limit and both global quantisers, products x * scale that are exactly
    k + 0.5 in float32 (np.round's half-to-even decides them), values at +-limit and values clipped by it."""
    X = _inputs(d)["edge"]
    for lim in LIMITS:
        for top in (127.0, 32767.0):
            p = np.clip(X, -lim, lim) * np.float32(top / lim)
            assert p.dtype == np.float32
            ties = np.unique(np.abs(p[np.abs(p) - np.floor(np.abs(p)) == 0.5]))
            assert ties.size >= 4 and ties.min() == 0.5 and ties.max() >= top - 2, (lim, top, ties)
            assert ((p > 0) & (np.abs(p) - np.floor(np.abs(p)) == 0.5)).any() and \
                ((p < 0) & (np.abs(p) - np.floor(np.abs(p)) == 0.5)).any()
        assert (X == np.float32(lim)).any() and (X == -np.float32(lim)).any()
        assert (X > np.float32(lim)).any() and (X < -np.float32(lim)).any()
        assert (X == np.nextafter(np.float32(lim), np.float32(0))).any()


# ----------------------------------------------------------------------------- float encoders
def _compare(d, mode, X, r, ref):
    c, q, mm = ref
    got = r["codes"].cpu().numpy()
    assert got.shape == c.shape and got.dtype == np.uint8
    assert np.array_equal(got, c), mode if mode == "cohere" else f"{mode}: " + _explain(d, X, got, c)
    if q is None:
        assert r["q"] is None
    else:
        gq = r["q"].cpu().numpy()
        assert gq.dtype == q.dtype and gq.shape == q.shape
        bad = np.flatnonzero((gq != q).any(axis=1))
        assert bad.size == 0, f"{mode} d={d}: q differs in rows {[(int(b), _row_kind(d, b)) for b in bad[:8]]}"
    if mm is None:
        assert r["minmax"] is None
    else:
        assert np.array_equal(r["minmax"].cpu().numpy(), mm), mode


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", DIMS)
def test_encoders_vs_oracle(dev, d, mode):
    from vectorragquantization_amd.quant import encode
    _check_sensitivity(d)                                   # before any GPU call
    X = _batch(d, mode in DENORMAL_MODES)
    for lim in (LIMITS if mode in GLOBAL_MODES else LIMITS[:1]):
        ref = _reference(mode, d, lim)
        r = encode(mode, X, lim, dev)
        torch.cuda.synchronize()
        _compare(d, mode, X, r, ref)


@gpu
@pytest.mark.parametrize("n", (1, 2, 3, 5))
def test_d1024_partial_workgroups(dev, n):
    """encode1024_kernel runs 4 waves per workgroup, one vector each: every partial last workgroup."""
    from vectorragquantization_amd.quant import encode
    _check_sensitivity(1024)
    X = _inputs(1024)["near"]
    for s in (0, 7, 35):
        Y = X[s:s + n]
        for mode in MODES:
            ref = (B.sbin_codes(Y), None, None) if mode == "sbin" else O.encode_batch(mode, Y, 0.3)
            r = encode(mode, Y, 0.3, dev)
            torch.cuda.synchronize()
            c, q, mm = ref
            assert np.array_equal(r["codes"].cpu().numpy(), c), (mode, s)
            if q is not None:
                assert np.array_equal(r["q"].cpu().numpy(), q), (mode, s)
            if mm is not None:
                assert np.array_equal(r["minmax"].cpu().numpy(), mm), (mode, s)


# ----------------------------------------------------------------------------- bin16
@functools.lru_cache(maxsize=None)
def _bin16_inputs(d):
    rng = np.random.default_rng(16 + d)
    X = rng.integers(-32768, 32768, (24, d)).astype(np.int16)
    X[8:16] = (rng.integers(-40, 41, (8, d)) + rng.integers(-3000, 3000, (8, 1))).astype(np.int16)
    E = np.zeros((6, d), np.int16)
    E[0], E[1], E[2] = -32768, 32767, 1234
    k = 777
    E[3] = k                                                # {k-1, k, k+1}, as many below as above: mean k
    pos = rng.permutation(d)
    E[3, pos[:d // 4]], E[3, pos[d // 4:2 * (d // 4)]] = k - 1, k + 1
    E[4, pos[:d // 2]] = -1                                 # -1 and 0 in equal parts: mean -0.5
    E[5] = E[3]
    E[5, pos[-1]] = k + 1                                   # one more above: mean k + 1/d, k no longer above it
    X = np.concatenate([X, E])
    assert np.mean(E[3]) == k and np.mean(E[4]) == -0.5
    X.setflags(write=False)
    return X


@gpu
@pytest.mark.parametrize("d", BIN16_DIMS)
def test_bin16_vs_oracle(dev, d):
    """VectorDBInt16._to_binary, packbits(int16 > float64 mean): the dim == 1024 branch and the generic one."""
    from vectorragquantization_amd.quant import encode
    X = _bin16_inputs(d)
    ref = O.encode_batch("bin16", X)[0]
    assert not ref[24].any() and not ref[25].any() and not ref[26].any()       # constant rows: nothing above
    assert int(np.unpackbits(ref[27]).sum()) == d // 4 and int(np.unpackbits(ref[28]).sum()) == d - d // 2
    for n in (X.shape[0], 1, 3):
        r = encode("bin16", X[-n:], device=dev)
        torch.cuda.synchronize()
        assert r["q"] is None and r["minmax"] is None
        got = r["codes"].cpu().numpy()
        bad = np.flatnonzero((got != ref[-n:]).any(axis=1))
        assert bad.size == 0, f"bin16 d={d} n={n}: rows {bad.tolist()} differ"
