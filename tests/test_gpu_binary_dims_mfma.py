"""K5mb (vrq_binary_topk_dim_mfma, enhanced.gemm_topk("binary", engine="mfma")): exhaustive binary (Phase-II)
top-k on the matrix cores at the embedding dims other than 1024, against the oracle
(oracle_np.exhaustive_scores / exhaustive_topk).  Inputs and exactness argument as
tests/test_gpu_exhaustive_dims.py: query values on the 2^-20 grid, so every +-q sum is exact in float64 in
any order and rows and scores must equal the oracle's with no tolerance.  The last test is host-only (plan,
workspace size, argument validation, engine choice)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests.test_gpu_exhaustive_dims import DIMS, _assert_exact, _grid_queries, _rows, _upload, dev  # noqa: F401
from vectorragquantization_amd import _native as N

gpu = pytest.mark.gpu
P8 = C.c_void_p(8)


def _plan(n, dim, nq, k):
    info = (C.c_int64 * 8)()
    assert N.load().vrq_binary_topk_dim_mfma_plan(n, dim, nq, k, info) == N.VRQ_OK
    return [int(v) for v in info]  # chunk rows, chunks, capacity, query blocks, sample chunks, rows, bytes, q / block


def _layout(n, dim, nq, k):
    lay = (C.c_int64 * 8)()
    assert N.load().vrq_binary_topk_dim_mfma_prep_layout(n, dim, nq, k, lay) == N.VRQ_OK
    return [int(v) for v in lay]  # Delta, alpha, beta, flags, thresholds, nq_pad, list lengths, lists


def _run(Xd, qf, k, dev, row_offset=0, flags=0, workspace=None):
    from vectorragquantization_amd.enhanced import gemm_topk
    q = torch.from_numpy(np.ascontiguousarray(qf)).to(dev)
    cnt, rows, sc = gemm_topk("binary", q, k, codes=Xd, row_offset=row_offset, flags=flags, workspace=workspace,
                              engine="mfma")
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy()


def _overflowing_n(dim, nq, k):
    """The smallest n (in steps of 2^15 rows) whose main chunks are longer than a list."""
    return next(c for c in range(1 << 15, 1 << 22, 1 << 15) if _plan(c, dim, nq, k)[0] > _plan(c, dim, nq, k)[2])


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_parity_per_dim(dev, dim):
    """Two query blocks (the second holds one query), >= 3 chunks, and a last chunk of more than one tile whose
    last tile is shifted back."""
    k = 10
    nq = _plan(100_000, dim, 10_000, k)[7] + 1
    n = next(c for c in range(39, 100_000, 32)
             if _plan(c, dim, nq, k)[1] >= 3 and c % _plan(c, dim, nq, k)[0] > 32)
    assert _plan(n, dim, nq, k)[3] == 2 and n % 32 != 0
    rng = np.random.default_rng(12000 + dim)
    X, qf = _rows(rng, "binary", n, dim), _grid_queries(rng, nq, dim)
    out = _run(_upload("binary", X, dev)[0], qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)
    assert np.all(out[0] == k)                        # the matrix path alone served the batch
    _assert_exact("binary", X, qf, k, out)


@gpu
@pytest.mark.parametrize("dim", (256, 384, 2048))     # one dim of each wave layout; 384: the 12-step k-loop
def test_parity_long_chunks(dev, dim):
    """Chunks of >= 4 tiles: both ring slots and both register sets of the loads two tiles ahead, hits staged
    from inside the tile loop, the drain at the chunk's end."""
    n, nq, k = 100_003, 5, 10
    p = _plan(n, dim, nq, k)
    assert p[0] >= 128 and n % p[0] > 32 and n % 32 != 0
    rng = np.random.default_rng(12500 + dim)
    X, qf = _rows(rng, "binary", n, dim), _grid_queries(rng, nq, dim)
    out = _run(_upload("binary", X, dev)[0], qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)
    assert np.all(out[0] == k)
    _assert_exact("binary", X, qf, k, out)


@gpu
@pytest.mark.parametrize("dim", (384, 2048))
@pytest.mark.parametrize("n,nq,k,row_offset", [(1, 1, 10, 0), (31, 1, 10, 0), (33, 1, 10, 0), (1500, 3, 1, 0),
                                               (1500, 3, 1024, 0), (1500, 3, 10, 7000)])
def test_shape_edges(dev, dim, n, nq, k, row_offset):
    rng = np.random.default_rng(13000 + dim + n + k)
    X, qf = _rows(rng, "binary", n, dim), _grid_queries(rng, nq, dim)
    out = _run(_upload("binary", X, dev)[0], qf, k, dev, row_offset=row_offset, flags=N.VRQ_GEMM_NO_FALLBACK)
    _assert_exact("binary", X, qf, k, out, row_offset=row_offset)


@gpu
def test_retry_serves_an_overflowed_list(dev):
    """A whole main chunk that no sample chunk touches holds query 0's sign code with a falling number of random
    bit flips, the best row last: every row passes the sampled threshold, the list keeps `capacity` of them and
    overflows, and rows of the true top-k are among those it dropped.  The retry at the raised threshold must
    serve the query without the exact scan."""
    dim, nq, k = 256, 3, 10
    n = _overflowing_n(dim, nq, k)
    cr, nchunks, capc, _, nsc, scr = _plan(n, dim, nq, k)[:6]
    sstride = n // nsc
    m = next(c for c in range(nchunks // 2, nchunks - 1)
             if all(not (s * sstride < (c + 1) * cr and c * cr < s * sstride + scr) for s in range(n // sstride + 1)))
    rng = np.random.default_rng(17000)
    X, qf = _rows(rng, "binary", n, dim), _grid_queries(rng, nq, dim)
    bits = np.tile(qf[0] > 0, (cr, 1))
    for i, f in enumerate(np.linspace(dim // 8, 0, cr).astype(int)):
        bits[i, rng.choice(dim, f, replace=False)] ^= True
    X[m * cr:(m + 1) * cr] = np.packbits(bits, axis=1)
    Xd = _upload("binary", X, dev)[0]
    ws = torch.empty((_plan(n, dim, nq, k)[6],), dtype=torch.uint8, device=dev)
    _run(Xd, qf, k, dev, flags=N.VRQ_GEMM_STAGE_SAMPLE | N.VRQ_GEMM_STAGE_MAIN, workspace=ws)
    off = _layout(n, dim, nq, k)[6] + 4 * m                                    # (query 0, chunk m)
    assert int(ws[off:off + 4].cpu().numpy().view(np.int32)[0]) > capc
    out = _run(Xd, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK, workspace=ws)
    assert np.all(out[0] == k) and np.any(out[1][0] >= m * cr + capc)          # rows the list had dropped
    _assert_exact("binary", X, qf, k, out)


@gpu
@pytest.mark.parametrize("dim", (256, 1536))
def test_identical_rows_and_zero_query(dev, dim):
    """Identical codes: every pair passes the threshold.  At n = 300 no list can overflow (capacity >= 64, chunks
    of one tile) and the matrix path serves the ties itself; at the smallest n whose chunks exceed the capacity
    every list overflows, in the retry too, and the exact scan serves rows 0..k-1 -- or, with
    VRQ_GEMM_NO_FALLBACK, the queries come back unserved.  A query of +-0 entries scores every row 0."""
    nq, k = 3, 10
    rng = np.random.default_rng(14000 + dim)
    row, qf = _rows(rng, "binary", 1, dim), _grid_queries(rng, nq, dim)
    X = np.repeat(row, 300, axis=0)
    _assert_exact("binary", X, qf, k, _run(_upload("binary", X, dev)[0], qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK))
    n = _overflowing_n(dim, nq, k)
    Xd = torch.from_numpy(row).to(dev).expand(n, dim // 8).contiguous()
    cnt, rows, sc = _run(Xd, qf, k, dev)
    ref = O.exhaustive_scores("binary", qf, codes=row)            # every row's score
    assert np.all(cnt == k) and np.array_equal(rows, np.tile(np.arange(k), (nq, 1)))
    assert np.array_equal(sc, np.repeat(ref, k, axis=1))
    assert np.all(_run(Xd, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)[0] == -1)
    X = _rows(rng, "binary", 300, dim)
    zero = np.where(rng.random((nq, dim)) < 0.5, np.float32(0.0), np.float32(-0.0))
    out = _run(_upload("binary", X, dev)[0], zero, k, dev)
    assert np.array_equal(out[1], np.tile(np.arange(k), (nq, 1)))
    _assert_exact("binary", X, zero, k, out)


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_bound_and_threshold(dev, dim):
    """Gaussian queries off the grid: the pieces, Delta and thr as the SAMPLE stage leaves them, against f64
    NumPy -- the piece in K5's fragment order, |u - (alpha s + beta)| <= Delta over all rows, and
    u >= ceil(thr) for every row of the oracle's top-k."""
    n, nq, k = 4096, 8, 10
    rng = np.random.default_rng(16000 + dim)
    X = _rows(rng, "binary", n, dim)
    qf = (rng.standard_normal((nq, dim)) * np.exp(rng.standard_normal((nq, dim)))).astype(np.float32)
    ws = torch.empty((_plan(n, dim, nq, k)[6],), dtype=torch.uint8, device=dev)
    _run(_upload("binary", X, dev)[0], qf, k, dev, flags=N.VRQ_GEMM_STAGE_SAMPLE, workspace=ws)
    lay, raw = _layout(n, dim, nq, k), ws.cpu().numpy()
    delta = raw[lay[0]:lay[0] + 8 * nq].view(np.float64)
    thr = raw[lay[4]:lay[4] + 4 * nq].view(np.float32).astype(np.float64)
    inv_s = 127.0 / np.abs(qf).max(axis=1).astype(np.float64)
    a = np.clip(np.rint(qf.astype(np.float64) * inv_s[:, None]), -127, 127)
    i = np.arange(dim)                                 # ph2_pos: dim 8 b + 7 - x of a k-step, x = 4 h + t
    b, x = (i & 31) >> 3, 7 - (i & 7)
    pos = (i & ~31) + (x >> 2) * 16 + 4 * (x & 3) + b
    assert np.array_equal(raw[:nq * dim].view(np.int8).reshape(nq, dim)[:, pos], a.astype(np.int8))
    u = a @ np.unpackbits(X, axis=1).astype(np.float64).T                       # exact integers below 2^24
    S = O.exhaustive_scores("binary", qf, codes=X)
    alpha, beta = 0.5 * inv_s, 0.5 * inv_s * qf.astype(np.float64).sum(axis=1)
    assert np.all(np.abs(u - (alpha[:, None] * S + beta[:, None])) <= delta[:, None])
    assert np.all(np.take_along_axis(u, O.exhaustive_topk(S, k), 1) >= np.ceil(thr)[:, None])
    assert np.all(np.isfinite(thr))


def test_plan_workspace_validation_engine():
    lib = N.load()
    for dim in DIMS:
        for n, nq, k in ((1, 1, 1), (5000, 3, 1024), (10_000_000, 1024, 10)):
            p = _plan(n, dim, nq, k)
            assert p[6] == lib.vrq_binary_topk_dim_mfma_workspace_size(n, dim, nq, k) > 0
            assert p[0] % 32 == 0 and p[1] * p[0] >= n > (p[1] - 1) * p[0] and p[3] * p[7] >= nq > (p[3] - 1) * p[7]
            assert _layout(n, dim, nq, k)[5] == p[3] * p[7] and _layout(n, dim, nq, k)[7] < p[6]
        assert lib.vrq_binary_topk_dim_engine(1_000_000, dim, 1, 10) == N.VRQ_GEMM_ENGINE_EXACT
    info = (C.c_int64 * 8)()

    def call(n, dim, k, flags=0, ws_bytes=1 << 40):
        return lib.vrq_binary_topk_dim_mfma(P8, n, dim, 0, P8, 1, k, flags, P8, P8, P8, P8, ws_bytes, None)

    for n, dim, k in ((1000, 1032, 10), (1000, 384, 1025), (1 << 32, 384, 10)):
        assert lib.vrq_binary_topk_dim_mfma_plan(n, dim, 1, k, info) == N.VRQ_EUNSUPPORTED
        assert lib.vrq_binary_topk_dim_mfma_prep_layout(n, dim, 1, k, info) == N.VRQ_EUNSUPPORTED
        assert lib.vrq_binary_topk_dim_mfma_workspace_size(n, dim, 1, k) == 0
        assert call(n, dim, k) == N.VRQ_EUNSUPPORTED
    assert call(1000, 384, 10, flags=N.VRQ_GEMM_SCAN_EXACT) == N.VRQ_EUNSUPPORTED
    assert call(1000, 1024, 10, flags=N.VRQ_GEMM_SCAN_EXACT) == N.VRQ_EUNSUPPORTED
    assert call(1000, 384, 10, ws_bytes=16) == N.VRQ_EWORKSPACE
    assert lib.vrq_binary_topk_dim_mfma(None, 1000, 384, 0, P8, 1, 10, 0, P8, P8, P8, P8, 1 << 40, None) == N.VRQ_EINVAL
    # at 1024 the size and plan calls answer for the forwarded K5 call; K5's layout calls are its own
    assert (lib.vrq_binary_topk_dim_mfma_workspace_size(1000, 1024, 1, 10)
            == lib.vrq_gemm_topk_workspace_size(N.VRQ_GEMM_BINARY, 1000, 1024, 1, 10) > 0)
    ref = (C.c_int64 * 8)()
    assert lib.vrq_binary_topk_dim_mfma_plan(1000, 1024, 1, 10, info) == N.VRQ_OK
    assert lib.vrq_gemm_topk_plan(N.VRQ_GEMM_BINARY, 1000, 1024, 1, 10, ref) == N.VRQ_OK and list(info) == list(ref)
    assert lib.vrq_binary_topk_dim_mfma_prep_layout(1000, 1024, 1, 10, info) == N.VRQ_EUNSUPPORTED
    assert call(1000, 1024, 10, ws_bytes=16) == N.VRQ_EWORKSPACE                # K5's own answer
    assert lib.vrq_binary_topk_dim_engine(1_000_000, 1024, 1024, 10) == N.VRQ_GEMM_ENGINE_EXACT
    # "auto" is K5mb where the table picks it and today's route otherwise: never a forced exact scan
    assert [N.binary_topk_engine(lib, 1000, 768, 64, 10, e) for e in (None, "exact", "mfma")] == [None, "exact", "mfma"]
    assert N.binary_topk_engine(lib, 1_000_000, 1024, 1024, 10, "auto") is None
    for dim in DIMS:                                   # the measured table: K5mb from nq = 8 at every dim
        assert [N.binary_topk_engine(lib, 1_000_000, dim, nq, 10, "auto") for nq in (1, 7, 8, 1024)] == [
            None, None, "mfma", "mfma"]
    assert N.binary_topk_engine(lib, 1_000_000, 768, 64, 1025, "auto") is None  # a shape K5mb does not serve
