"""K5gb on the GPU (gemm_topk("binary", rows=...)) against float64 NumPy over the allowed rows (grid queries: every sum
of +-q is exact, every assertion is on bits) and against the unfiltered matrix call on the gathered copy."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_exhaustive_dims import _grid_queries, _rows, dev  # noqa: F401
from vectorragquantization_amd import _native as N
from vectorragquantization_amd.enhanced import gemm_topk

pytestmark = pytest.mark.gpu
DIMS = (256, 384, 512, 768, 1024, 1536, 2048)


def _plan(m, dim, nq, k):  # chunk rows, chunks, list capacity, query blocks, sample chunks, their rows, bytes, qpb
    info = (C.c_int64 * 8)()
    assert N.load().vrq_binary_topk_gather_plan(m, dim, nq, k, info) == N.VRQ_OK
    return [int(v) for v in info]


def _search(codes, qf, k, allowed=None, flags=0, engine=None):
    rows = None if allowed is None else torch.from_numpy(np.asarray(allowed, dtype=np.uint32)).to(codes.device)
    out = gemm_topk("binary", torch.from_numpy(qf).to(codes.device), k, codes=codes, flags=flags, rows=rows,
                    engine=engine if allowed is not None else "mfma")
    return [t.cpu().numpy() for t in out]


def _case(dim, n, nq, k, allowed, dev, seed, plant=None, engine=None):
    """counts, rows, score bits == float64 top-k (score desc, row asc) of the allowed rows == the call on the copy"""
    rng, allowed = np.random.default_rng(seed), np.asarray(allowed, dtype=np.int64)
    X, qf = _rows(rng, "binary", n, dim), _grid_queries(rng, nq, dim)
    if plant is not None:
        plant(X, qf)
    codes, kc = torch.from_numpy(X).to(dev), min(k, len(allowed))
    cnt, rows, sc = _search(codes, qf, k, allowed, engine=engine)
    assert np.all(cnt == kc) and np.all(rows[:, kc:] == -1) and np.all(np.isnan(sc[:, kc:]))
    if kc:
        S = np.concatenate([qf.astype(np.float64) @ (2.0 * np.unpackbits(X[allowed[i:i + 8192]], axis=1) - 1.0).T
                            for i in range(0, len(allowed), 8192)], axis=1)
        order = np.lexsort((np.broadcast_to(allowed, S.shape), -S), axis=1)[:, :kc]
        assert np.array_equal(rows[:, :kc], allowed[order])
        assert np.array_equal(sc[:, :kc].view(np.int64), np.take_along_axis(S, order, 1).view(np.int64))
        copy = codes[torch.from_numpy(allowed).to(dev)].contiguous()
        c2, r2, s2 = _search(copy, qf, k, np.arange(len(allowed)) if dim == 1024 else None)
        assert np.array_equal(c2, cnt) and np.array_equal(s2.view(np.int64), sc.view(np.int64))
        assert np.array_equal(np.where(r2 >= 0, allowed[np.maximum(r2, 0)], -1), rows)
    return codes, qf, rows, sc


# (dim, n, m, nq, k): every instance on half the rows (m None: random, rows 0 and n - 1 allowed); the piece maps at the
# tile edges; the shifted last tile of a two-tile chunk; more than one query block (nq None: the block + 2)
SHAPES = [(d, 4096, None, 3, 10) for d in DIMS] + \
    [(d, 300, m, 3, 5) for d in (256, 384, 1024, 1536, 2048) for m in (0, 1, 3, 31, 32, 33, 97)] + \
    [(d, 40000, 32768 + 64 + 33, 3, 5) for d in (256, 1536)] + [(d, 2048, 1000, None, 5) for d in (256, 2048)]


@pytest.mark.parametrize("dim,n,m,nq,k", SHAPES)
def test_shapes(dev, dim, n, m, nq, k):
    rng = np.random.default_rng(dim + (m or 0))
    mask = rng.random(n) < 0.5
    mask[[0, n - 1]] = True
    allowed = np.flatnonzero(mask) if m is None else np.sort(rng.choice(n, m, replace=False))
    info = _plan(len(allowed), dim, nq or 1, k)
    assert m != 32768 + 64 + 33 or info[0] == 64
    _case(dim, n, nq or info[7] + 2, k, allowed, dev, 100 + dim + (m or 0), engine=(None, "mfma", "auto")[dim % 3])


def test_the_filter_decides(dev):
    """packbits(q > 0) is a query's best code: disallowed, no planted row comes back; allowed, it comes first."""
    dim, n, planted = 384, 2000, np.array([5, 700, 1999])
    def plant(X, qf):
        X[planted] = np.packbits(qf > 0, axis=1)
    rest = np.setdiff1d(np.arange(n)[::2], planted)
    codes, qf, rows, _ = _case(dim, n, 3, 4, rest, dev, 500, plant)
    assert not np.isin(rows, planted).any()
    assert np.array_equal(_search(codes, qf, 1)[1][:, 0], planted)  # unfiltered: they are the top
    assert np.array_equal(_case(dim, n, 3, 4, np.union1d(rest, planted), dev, 500, plant)[2][:, 0], planted)


def test_real_sample_and_tie_order(dev):
    """A strict-subset sample; four copies of query 0's best code at a tile and a chunk boundary come back first."""
    dim, n, m, nq, k = 256, 100000, 40000, 3, 10
    info = _plan(m, dim, nq, k)
    assert info[0] == 64 and info[4] * info[5] < m  # chunk rows; sample chunks x rows per sample chunk
    allowed = np.sort(np.random.default_rng(7).choice(n, m, replace=False))
    dup = allowed[[31, 32, 63, 64]]
    def plant(X, qf):
        X[dup] = np.packbits(qf[:1] > 0, axis=1)
    _, _, rows, sc = _case(dim, n, nq, k, allowed, dev, 600, plant)
    assert np.array_equal(rows[0, :4], dup) and len(np.unique(sc[0, :4])) == 1


def test_retry_fallback_and_python_surface(dev):
    """Identical codes, every second row allowed, chunks longer than the list capacity: every list overflows twice."""
    dim, nq, k = 256, 2, 5
    m = next(c for c in range(1 << 15, 1 << 22, 1 << 15) if _plan(c, dim, nq, k)[0] > _plan(c, dim, nq, k)[2])
    rng = np.random.default_rng(700)
    row, qf = _rows(rng, "binary", 1, dim), _grid_queries(rng, nq, dim)
    codes, allowed = torch.from_numpy(row).to(dev).expand(2 * m, dim // 8).contiguous(), np.arange(0, 2 * m, 2)
    assert np.all(_search(codes, qf, k, allowed, flags=N.VRQ_GEMM_NO_FALLBACK)[0] == -1)
    cnt, rows, sc = _search(codes, qf, k, allowed)
    assert np.all(cnt == k) and np.array_equal(rows, np.tile(allowed[:k], (nq, 1)))
    ref = qf.astype(np.float64) @ (2.0 * np.unpackbits(row[0]) - 1.0)
    assert np.array_equal(sc.view(np.int64), np.repeat(ref[:, None], k, 1).view(np.int64))
    with pytest.raises(N.VrqNativeError):  # the exact scan takes no list
        _search(codes, qf, k, allowed, engine="exact")
    with pytest.raises(N.VrqNativeError):  # checked_rows: not ascending
        _search(codes, qf, k, allowed[:8][::-1].copy())
