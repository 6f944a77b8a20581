"""GPU parity of the dequantiser (``vrq_dequantize``), the dequantised-dot rescoring (``vrq_rescore_dequant``)
and the int8 row norms (``vrq_int8_row_norms``) away from dim 1024: odd dims (the ``(dim + 1) / 2`` byte
stride of the int4 rows, the scalar branch of the norms), dims that are no multiple of the 64-lane or
256-thread strides, and the largest dim.  Every mode takes odd dims here: ``quant.dequantize`` and
``O.dequantize`` express them for the int8 / int16 rows as well as for the nibble rows.

The stored rows hold every value of their type -- int8 -128 and int16 -32768, which the encoders never
write, included -- and every byte 0 .. 255 for the nibble modes; the (min, max) rows hold the cases of
``deq_row``.  References: ``O.dequantize`` bit for bit; the exact sum ``math.fsum`` of the float64
products rounded once to float32 for the scores; ``math.sqrt`` of the exact integer sum of squares for the
norms.  No tolerance anywhere."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import oracle_np as O

gpu = pytest.mark.gpu

MODES = ("int8g", "int16g", "int4g", "int8", "int4")
DEQ_DIMS = (7, 8, 1000, 1001, 1536, 2048, 8192)
RESCORE_DIMS = (8, 1000, 1536)
NORM_DIMS = (1, 7, 8, 24, 1000, 1001, 1040, 8192)
LIMITS = (0.3, 1.0, 1e-3)
N_ROWS = 72           # 72 rows of 4 bytes (dim 7, int4) hold every byte value

# (min, max) cases, repeated down the rows
MINMAX_CASES = [
    (0.25, 0.25),                                    # min == max with non-zero q: a zero row
    (-0.7, 0.3),                                     # |min| > |max|
    (-0.2, 0.9),                                     # |min| < |max|
    (-0.9, -0.1),                                    # both negative
    (-1.0 / 3.0, 2.0 / 3.0),                         # doubles that are no float32 values
    (-math.pi / 10, math.e / 10),
    (0.1, 0.1 + 1e-12),                              # differ as doubles, equal as float32: int8 zero, int4 not
    (float(np.float32(-0.123)), float(np.float32(0.456))),   # what the encoder writes: float32 values
    (0.0, 0.0),
    (-0.0, 0.0),                                     # equal: a zero row
    (-1e-30, 3e-30), (-2e30, 1e30),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(dev)      # (the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _stored(mode, d):
    """-> (q, minmax | None) of N_ROWS rows: every value of the type, in an order that puts each of them
    at many offsets of a row, then random values."""
    rng = np.random.default_rng(d + 31 * MODES.index(mode))
    if mode == "int16g":
        q = rng.integers(-32768, 32768, (N_ROWS, d)).astype(np.int16)
        flat = q.reshape(-1)
        flat[rng.choice(flat.size, 6, replace=False)] = [-32768, 32767, -32767, 0, -1, 1]
        q[3] = -32768
        assert q.min() == -32768 and q.max() == 32767
    else:
        w = (d + 1) // 2 if mode in ("int4g", "int4") else d
        flat = rng.integers(0, 256, N_ROWS * w)
        pos = 5 * w + rng.permutation(flat.size - 5 * w)[:256]         # (below the two constant rows)
        flat[pos] = np.arange(256)                                     # every byte / every int8 value
        q = flat.astype(np.uint8).view(np.int8).reshape(N_ROWS, w).copy()
        q[3] = -128                                                    # int8 -128; byte 0x80 = nibbles 0, -8
        q[4] = 127                                                     # byte 0x7f = nibbles -1, 7
        assert np.unique(q[5:].view(np.uint8)).size == 256
    mm = None
    if mode in ("int8", "int4"):
        mm = np.array([MINMAX_CASES[r % len(MINMAX_CASES)] for r in range(N_ROWS)], np.float64)
        mm[len(MINMAX_CASES) * 2:] = np.sort(rng.standard_normal((N_ROWS - 2 * len(MINMAX_CASES), 2)), axis=1)
        mm.setflags(write=False)
    q.setflags(write=False)
    return q, mm


def test_minmax_cases_are_what_they_claim():
    """On the CPU oracle (the GPU never enters): the equal-after-the-cast pair is a zero row for int8 and a
    non-zero row for int4; min == max gives zeros from non-zero q."""
    q8, mm = _stored("int8", 8)
    q4, _ = _stored("int4", 8)
    a, b = mm[6]
    assert a != b and np.float32(a) == np.float32(b)
    d8, d4 = O.dequantize("int8", q8, mm, None, 8), O.dequantize("int4", q4, mm, None, 8)
    assert q8[6].any() and not d8[6].any() and d4[6].any()
    for r in (0, 8, 9):
        assert q8[r].any() and not d8[r].any() and not d4[r].any()
    assert d8[1].any() and d8[3].any() and d4[1].any()
    assert np.float32(mm[4, 0]) != mm[4, 0] and np.float32(mm[5, 1]) != mm[5, 1]


# ----------------------------------------------------------------------------- vrq_dequantize
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", DEQ_DIMS)
def test_dequantize_vs_oracle(dev, d, mode):
    from vectorragquantization_amd.quant import dequantize
    q, mm = _stored(mode, d)
    for lim in (LIMITS if mm is None else LIMITS[:1]):
        ref = O.dequantize(mode, q, mm, lim, d)
        got = dequantize(mode, q, mm, lim, d, dev)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == (N_ROWS, d) and got.dtype == np.float32 and ref.dtype == np.float32
        bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))      # by bits: the sign of a zero too
        assert bad.size == 0, f"{mode} d={d} limit={lim}: {bad.shape[0]} elements differ, first (row, col) {bad[:5].tolist()}"
    for n in (1, 3):                                                   # the last rows alone
        got = dequantize(mode, q[-n:], None if mm is None else mm[-n:], 0.3, d, dev).cpu().numpy()
        assert np.array_equal(got, O.dequantize(mode, q[-n:], None if mm is None else mm[-n:], 0.3, d))


# ----------------------------------------------------------------------------- vrq_rescore_dequant
def _rescore(mode_id, qf, d, q, mm, limit, cand, dev):
    from vectorragquantization_amd import _native as N
    lib = N.load()
    qf_t, q_t, cand_t = _t(qf, dev), _t(q, dev), _t(cand, dev)
    mm_t = None if mm is None else _t(mm, dev)
    out = torch.empty(cand.shape, dtype=torch.float64, device=dev)
    N.check(lib.vrq_rescore_dequant(mode_id, N.ptr(qf_t), qf.shape[0], d, N.ptr(q_t), N.ptr(mm_t), float(limit),
                                    q.shape[0], N.ptr(cand_t), cand.shape[1], N.ptr(out), N.stream_handle(dev)),
            "vrq_rescore_dequant")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _candidates(rng, n, nq=3, nc=32):
    cand = rng.integers(0, n, (nq, nc)).astype(np.int64)
    cand[:, :12] = np.arange(12)                       # every (min, max) case, the -128 and the 127 rows
    cand[:, 12], cand[:, 13], cand[:, 14], cand[:, 15], cand[:, 16] = -1, n, n - 1, 5, 5
    cand[1, 20], cand[2, 21] = -7, n + 100
    return cand


def _check_scores(got, qf, rows, cand, tag):
    n = rows.shape[0]
    for qi in range(cand.shape[0]):
        q64 = qf[qi].astype(np.float64)
        for j in range(cand.shape[1]):
            r = cand[qi, j]
            if r < 0 or r >= n:
                assert np.isnan(got[qi, j]), (tag, qi, j)
                continue
            want = np.float32(math.fsum((q64 * rows[r].astype(np.float64)).tolist()))
            assert got[qi, j] == float(want), (tag, qi, j, int(r), got[qi, j], float(want))


@gpu
@pytest.mark.parametrize("mode", MODES + ("f32",))
@pytest.mark.parametrize("d", RESCORE_DIMS)
def test_rescore_dequant_exact(dev, d, mode):
    """The score is the exact sum of the exact float32 x float32 products, rounded once to float32.  The
    kernel accumulates in float64: it can differ from the exact sum only where that lies within about
    2^-50 relative of a float32 rounding midpoint, which none of these seeds hits."""
    from vectorragquantization_amd import _native as N
    rng = np.random.default_rng(100 + d)
    qf = (rng.standard_normal((3, d)) * rng.uniform(0.01, 2.0, (3, 1))).astype(np.float32)
    cand = _candidates(rng, N_ROWS)
    if mode == "f32":
        rows = (rng.standard_normal((N_ROWS, d)) * rng.uniform(1e-3, 10.0, (N_ROWS, 1))).astype(np.float32)
        rows[3], rows[4], rows[5, ::2] = 0.0, -1.5, 1e-40
        _check_scores(_rescore(N.VRQ_RESCORE_F32, qf, d, rows, None, 0.0, cand, dev), qf, rows, cand, mode)
        return
    q, mm = _stored(mode, d)
    for lim in (LIMITS if mm is None else LIMITS[:1]):
        rows = O.dequantize(mode, q, mm, lim, d)
        _check_scores(_rescore(N.ENC_MODES[mode], qf, d, q, mm, lim, cand, dev), qf, rows, cand, (mode, lim))


# ----------------------------------------------------------------------------- vrq_int8_row_norms
@functools.lru_cache(maxsize=None)
def _norm_rows(d):
    rng = np.random.default_rng(7 + d)
    x = rng.integers(-128, 128, (777, d)).astype(np.int8)
    x[0], x[1], x[2], x[3] = -128, 127, 0, 0
    x[3, d - 1] = -3                                   # a single non-zero element, the last one
    x[776], x[775] = -128, 0
    x[775, 0] = 1
    x.setflags(write=False)
    return x


@gpu
@pytest.mark.parametrize("d", NORM_DIMS)
def test_int8_row_norms_exact(dev, d):
    """Both branches of the kernel (16-byte loads at dim % 16 == 0, the scalar loop otherwise), one row,
    fewer rows than the waves of a workgroup, and many workgroups."""
    from vectorragquantization_amd.quant import int8_row_norms
    x = _norm_rows(d)
    ss = (x.astype(np.int64) ** 2).sum(axis=1)         # exact integers
    ref = np.array([math.sqrt(int(s)) for s in ss], np.float64)
    assert ref[0] == math.sqrt(d * 16384) and ref[2] == 0.0 and ref[3] == 3.0
    for n in (1, 5, 777):
        got = int8_row_norms(_t(x[:n], dev))
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (n,)
        assert np.array_equal(got, ref[:n]), (d, n, np.flatnonzero(got != ref[:n])[:8].tolist())
