"""K5md (vrq_gemm_topk_dim_mfma, enhanced.gemm_topk(engine="mfma")): exhaustive int8-cosine top-k on the
matrix cores at the embedding dims other than 1024, against the oracle (oracle_np.exhaustive_scores /
exhaustive_topk).  Inputs and exactness argument as tests/test_gpu_exhaustive_dims.py: values on the 2^-20
grid, norms from oracle_np.int8_row_norms, so rows and scores must equal the oracle's with no tolerance.
The last test is host-only (plan, workspace size, argument validation, engine choice)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests.test_gpu_exhaustive_dims import DIMS, _assert_exact, _grid_queries, _rows, _upload, dev  # noqa: F401
from vectorragquantization_amd import _native as N

gpu = pytest.mark.gpu
MODE = N.VRQ_GEMM_INT8_COSINE
P8 = C.c_void_p(8)


def _plan(n, dim, nq, k):
    info = (C.c_int64 * 8)()
    assert N.load().vrq_gemm_topk_dim_mfma_plan(MODE, n, dim, nq, k, info) == N.VRQ_OK
    return [int(v) for v in info]  # chunk rows, chunks, capacity, query blocks, sample chunks, rows, bytes, q / block


def _run(Xd, norms, qf, k, dev, row_offset=0, flags=0, workspace=None):
    from vectorragquantization_amd.enhanced import gemm_topk
    q = torch.from_numpy(np.ascontiguousarray(qf)).to(dev)
    cnt, rows, sc = gemm_topk("int8_cosine", q, k, x8=Xd, norms=norms, row_offset=row_offset, flags=flags,
                              workspace=workspace, engine="mfma")
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy()


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_parity_per_dim(dev, dim):
    """Two query blocks (the second holds one query), >= 3 chunks, and a last chunk of more than one tile whose
    last tile is shifted back (n % 32 != 0 alone gives a tiny last chunk while chunks are one tile long)."""
    k = 10
    nq = _plan(100_000, dim, 10_000, k)[7] + 1
    n = next(c for c in range(39, 100_000, 32)
             if _plan(c, dim, nq, k)[1] >= 3 and c % _plan(c, dim, nq, k)[0] > 32)
    assert _plan(n, dim, nq, k)[3] == 2 and n % 32 != 0
    rng = np.random.default_rng(2000 + dim)
    X, qf = _rows(rng, "int8_cosine", n, dim), _grid_queries(rng, nq, dim)
    Xd, norms = _upload("int8_cosine", X, dev)
    out = _run(Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)
    assert np.all(out[0] == 10)                       # the matrix path alone served the batch
    _assert_exact("int8_cosine", X, qf, k, out)


@gpu
@pytest.mark.parametrize("dim", (256, 384, 2048))     # one dim of each wave layout
def test_parity_long_chunks(dev, dim):
    """Chunks of 4 tiles: the main pass's steady state (hits staged from inside the tile loop, both tile
    parities, the drain at the chunk's end), served by the matrix path alone."""
    n, nq, k = 100_003, 5, 10
    p = _plan(n, dim, nq, k)
    assert p[0] >= 128 and n % p[0] > 32 and n % 32 != 0
    rng = np.random.default_rng(2500 + dim)
    X, qf = _rows(rng, "int8_cosine", n, dim), _grid_queries(rng, nq, dim)
    Xd, norms = _upload("int8_cosine", X, dev)
    out = _run(Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)
    assert np.all(out[0] == k)
    _assert_exact("int8_cosine", X, qf, k, out)


@gpu
def test_retry_serves_an_overflowed_list(dev):
    """A whole main chunk that no sample chunk touches holds rows graded towards query 0, the best last: every
    one passes the sampled threshold, the list keeps the first `capacity` of them and overflows, and rows of
    the true top-k are among those it dropped.  The retry at the raised threshold must serve the query without
    the exact scan."""
    dim, nq, k = 256, 3, 10
    n = next(c for c in range(1 << 15, 1 << 22, 1 << 15) if _plan(c, dim, nq, k)[0] > _plan(c, dim, nq, k)[2])
    cr, nchunks, capc, _, _, scr = _plan(n, dim, nq, k)[:6]
    sstride = n // _plan(n, dim, nq, k)[4]
    m = next(c for c in range(nchunks // 2, nchunks - 1)
             if all(not (s * sstride < (c + 1) * cr and c * cr < s * sstride + scr) for s in range(n // sstride + 1)))
    rng = np.random.default_rng(7000)
    X, qf = _rows(rng, "int8_cosine", n, dim), _grid_queries(rng, nq, dim)
    g = np.linspace(0.8, 1.5, cr)[:, None]
    X[m * cr:(m + 1) * cr] = np.clip(np.rint(qf[0] * 12 * g) + rng.integers(-30, 31, (cr, dim)), -127, 127)
    Xd, norms = _upload("int8_cosine", X, dev)
    ws = torch.empty((_plan(n, dim, nq, k)[6],), dtype=torch.uint8, device=dev)
    _run(Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_STAGE_SAMPLE | N.VRQ_GEMM_STAGE_MAIN, workspace=ws)
    lay = (C.c_int64 * 8)()
    assert N.load().vrq_gemm_topk_dim_mfma_prep_layout(MODE, n, dim, nq, k, lay) == N.VRQ_OK
    assert int(ws[lay[6] + 4 * m:lay[6] + 4 * m + 4].cpu().numpy().view(np.int32)[0]) > capc   # (query 0, chunk m)
    out = _run(Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK, workspace=ws)
    assert np.all(out[0] == k) and np.any(out[1][0] >= m * cr + capc)       # rows the list had dropped
    _assert_exact("int8_cosine", X, qf, k, out)


@gpu
@pytest.mark.parametrize("dim", (384, 2048))          # 8 waves x 32 queries; 4 waves, A in the AGPR half
@pytest.mark.parametrize("n,nq,k,row_offset", [(1, 1, 10, 0), (31, 1, 10, 0), (33, 1, 10, 0), (1500, 3, 1, 0),
                                               (1500, 3, 1024, 0), (1500, 3, 10, 7000)])
def test_shape_edges(dev, dim, n, nq, k, row_offset):
    rng = np.random.default_rng(3000 + dim + n + k)
    X, qf = _rows(rng, "int8_cosine", n, dim), _grid_queries(rng, nq, dim)
    Xd, norms = _upload("int8_cosine", X, dev)
    out = _run(Xd, norms, qf, k, dev, row_offset=row_offset, flags=N.VRQ_GEMM_NO_FALLBACK)
    _assert_exact("int8_cosine", X, qf, k, out, row_offset=row_offset)


@gpu
@pytest.mark.parametrize("dim", (256, 1536))
def test_identical_rows_overflow_retry_fallback(dev, dim):
    """Identical rows: every pair passes the threshold.  At n = 300 the chunks are one tile long and no list can
    overflow (capacity >= 64): the matrix path serves the ties itself.  At the smallest n whose chunks exceed the
    list capacity every list overflows, the retry's raised threshold still admits every row, and the queries go
    to the exact scan -- or, with VRQ_GEMM_NO_FALLBACK, come back unserved."""
    nq, k = 3, 10
    rng = np.random.default_rng(4000 + dim)
    row, qf = _rows(rng, "int8_cosine", 1, dim), _grid_queries(rng, nq, dim)
    X = np.repeat(row, 300, axis=0)
    _assert_exact("int8_cosine", X, qf, k, _run(*_upload("int8_cosine", X, dev), qf, k, dev,
                                                flags=N.VRQ_GEMM_NO_FALLBACK))
    n = next(c for c in range(1 << 15, 1 << 22, 1 << 15) if _plan(c, dim, nq, k)[0] > _plan(c, dim, nq, k)[2])
    Xd = torch.from_numpy(row).to(dev).expand(n, dim).contiguous()
    norms = torch.from_numpy(O.int8_row_norms(row)).to(dev).expand(n).contiguous()
    cnt, rows, sc = _run(Xd, norms, qf, k, dev)
    ref = O.exhaustive_scores("int8_cosine", qf, x8=row)          # every row's score
    assert np.all(cnt == k) and np.array_equal(rows, np.tile(np.arange(k), (nq, 1)))
    assert np.array_equal(sc, np.repeat(ref, k, axis=1))
    assert np.all(_run(Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)[0] == -1)


@gpu
@pytest.mark.parametrize("dim", (256, 1536))
def test_zero_norm_rows_fallback(dev, dim):
    """All but k - 1 rows have zero norm: fewer than k candidates can arrive, the exact scan serves the query
    and -inf fills the rest in row order."""
    n, nq, k = 300, 3, 10
    rng = np.random.default_rng(5000 + dim)
    X, qf = _rows(rng, "int8_cosine", n, dim), _grid_queries(rng, nq, dim)
    X[np.setdiff1d(np.arange(n), rng.choice(n, k - 1, replace=False))] = 0
    Xd, norms = _upload("int8_cosine", X, dev)
    out = _run(Xd, norms, qf, k, dev)
    _assert_exact("int8_cosine", X, qf, k, out)
    assert np.all(np.isneginf(out[2][:, k - 1])) and np.all(np.isfinite(out[2][:, :k - 1]))
    assert np.all(_run(Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)[0] == -1)


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_bound_and_threshold(dev, dim):
    """Gaussian queries off the grid: Delta and thr as the SAMPLE stage leaves them, against f64 NumPy --
    |u - s'| <= Delta over all rows and u >= thr for every row of the oracle's top-k."""
    n, nq, k = 4096, 8, 10
    rng = np.random.default_rng(6000 + dim)
    X = _rows(rng, "int8_cosine", n, dim)
    qf = (rng.standard_normal((nq, dim)) * np.exp(rng.standard_normal((nq, dim)))).astype(np.float32)
    Xd, norms = _upload("int8_cosine", X, dev)
    ws = torch.empty((_plan(n, dim, nq, k)[6],), dtype=torch.uint8, device=dev)
    _run(Xd, norms, qf, k, dev, flags=N.VRQ_GEMM_STAGE_SAMPLE, workspace=ws)
    lay = (C.c_int64 * 8)()
    assert N.load().vrq_gemm_topk_dim_mfma_prep_layout(MODE, n, dim, nq, k, lay) == N.VRQ_OK
    raw = ws.cpu().numpy()
    delta = raw[lay[0]:lay[0] + 8 * nq].view(np.float64)
    thr = raw[lay[4]:lay[4] + 4 * nq].view(np.float32).astype(np.float64)
    inv_s = 127.0 / np.abs(qf).max(axis=1).astype(np.float64)
    a = np.clip(np.rint(qf.astype(np.float64) * inv_s[:, None]), -127, 127)
    assert np.array_equal(raw[:nq * dim].view(np.int8).reshape(nq, dim), a.astype(np.int8))
    nrm = O.int8_row_norms(X)
    dot = (a @ X.astype(np.float64).T).astype(np.float32)                       # exact integers below 2^25
    u = (dot * (np.float32(1) / nrm.astype(np.float32))).astype(np.float64)
    S = O.exhaustive_scores("int8_cosine", qf, x8=X)
    assert np.all(np.abs(u - S * inv_s[:, None]) <= delta[:, None])
    top = O.exhaustive_topk(S, k)
    assert np.all(np.take_along_axis(u, top, 1) >= thr[:, None])
    assert np.all(np.isfinite(thr))


def test_plan_workspace_validation_engine():
    lib = N.load()
    for dim in DIMS:
        for n, nq, k in ((1, 1, 1), (5000, 3, 1024), (10_000_000, 1024, 10)):
            p = _plan(n, dim, nq, k)
            assert p[6] == lib.vrq_gemm_topk_dim_mfma_workspace_size(MODE, n, dim, nq, k) > 0
            assert p[0] % 32 == 0 and p[1] * p[0] >= n > (p[1] - 1) * p[0] and p[3] * p[7] >= nq > (p[3] - 1) * p[7]
        assert lib.vrq_gemm_topk_dim_engine(MODE, 1_000_000, dim, 1, 10) == N.VRQ_GEMM_ENGINE_EXACT
        assert lib.vrq_gemm_topk_dim_engine(N.VRQ_GEMM_BINARY, 1_000_000, dim, 1024, 10) == N.VRQ_GEMM_ENGINE_EXACT
    info = (C.c_int64 * 8)()
    for mode, n, dim, k, rc in ((N.VRQ_GEMM_BINARY, 1000, 384, 10, N.VRQ_EUNSUPPORTED),
                                (N.VRQ_GEMM_FLOAT_IP, 1000, 384, 10, N.VRQ_EINVAL),
                                (MODE, 1000, 1032, 10, N.VRQ_EUNSUPPORTED), (MODE, 1000, 384, 1025, N.VRQ_EUNSUPPORTED),
                                (MODE, 1 << 32, 384, 10, N.VRQ_EUNSUPPORTED)):
        assert lib.vrq_gemm_topk_dim_mfma_plan(mode, n, dim, 1, k, info) == rc
        assert lib.vrq_gemm_topk_dim_mfma_workspace_size(mode, n, dim, 1, k) == 0
        assert lib.vrq_gemm_topk_dim_mfma(mode, P8, P8, P8, n, dim, 0, P8, 1, k, 0, P8, P8, P8, P8, 1 << 40, None) == rc
    assert lib.vrq_gemm_topk_dim_mfma(MODE, P8, P8, P8, 1000, 384, 0, P8, 1, 10, N.VRQ_GEMM_SCAN_EXACT, P8, P8, P8, P8,
                                      1 << 40, None) == N.VRQ_EUNSUPPORTED
    assert lib.vrq_gemm_topk_dim_mfma(MODE, P8, P8, P8, 1000, 384, 0, P8, 1, 10, 0, P8, P8, P8, P8, 16,
                                      None) == N.VRQ_EWORKSPACE
    assert (lib.vrq_gemm_topk_dim_mfma_workspace_size(MODE, 1000, 1024, 1, 10)
            == lib.vrq_gemm_topk_workspace_size(MODE, 1000, 1024, 1, 10))
    # the size and plan calls answer for the calls the entry point accepts, at 1024 too
    assert lib.vrq_gemm_topk_dim_mfma_workspace_size(N.VRQ_GEMM_BINARY, 1000, 1024, 1, 10) == 0
    assert lib.vrq_gemm_topk_dim_mfma_plan(N.VRQ_GEMM_BINARY, 1000, 1024, 1, 10, info) == N.VRQ_EUNSUPPORTED
    assert lib.vrq_gemm_topk_dim_mfma_plan(N.VRQ_GEMM_FLOAT_IP, 1000, 1024, 1, 10, info) == N.VRQ_EINVAL
    # "auto" is K5md where the table picks it and today's route otherwise: never a forced exact scan
    for mode in (MODE, N.VRQ_GEMM_BINARY):
        assert N.gemm_topk_engine(lib, mode, 1_000_000, 1024, 1024, 10, "auto") is None
    assert N.gemm_topk_engine(lib, MODE, 1_000_000, 768, 64, 10, "auto") == "mfma"
    assert N.gemm_topk_engine(lib, MODE, 1_000_000, 768, 1, 10, "auto") is None
    assert N.gemm_topk_engine(lib, N.VRQ_GEMM_BINARY, 1_000_000, 768, 64, 10, "auto") is None
    assert [N.gemm_topk_engine(lib, MODE, 1000, 768, 64, 10, e) for e in (None, "exact", "mfma")] == [None, "exact", "mfma"]
