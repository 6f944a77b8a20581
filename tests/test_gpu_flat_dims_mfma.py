"""K5mf (vrq_flat_ip_prepare_dim, vrq_flat_ip_topk_dim_mfma, flat_ip_topk(engine="mfma"), FloatIndexIDMap /
CohereVectorDBFloat(engine=)): the exact float inner-product top-k on the matrix cores at the embedding dims
other than 1024, against the oracle (oracle_np.flat_ip_scores / flat_ip_search).  Inputs and exactness argument
as tests/test_gpu_exhaustive_dims.py: values on the 2^-20 grid make every f64 sum exact, so rows and scores must
equal the oracle's with no tolerance.  The last test is host-only."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from tests.test_gpu_exhaustive_dims import DIMS, G, _assert_exact, _grid_queries, _rows, dev  # noqa: F401
from vectorragquantization_amd import _native as N

gpu = pytest.mark.gpu
P8 = C.c_void_p(8)


def _plan(n, dim, nq, k):
    info = (C.c_int64 * 8)()
    assert N.load().vrq_flat_ip_topk_dim_mfma_plan(n, dim, nq, k, info) == N.VRQ_OK
    return [int(v) for v in info]  # chunk rows, chunks, capacity, query blocks, sample chunks, rows, bytes, q / block


def _prepare(X, dev):
    from vectorragquantization_amd.flat import flat_ip_prepare
    xf = X if isinstance(X, torch.Tensor) else torch.from_numpy(X).to(dev)
    bounds = torch.zeros((2,), dtype=torch.float64, device=dev)
    return (xf, *flat_ip_prepare(xf, bounds), bounds)


def _run(ops, qf, k, dev, row_offset=0, flags=0, workspace=None, engine="mfma"):
    from vectorragquantization_amd.flat import flat_ip_topk
    q = torch.from_numpy(np.ascontiguousarray(qf)).to(dev)
    cnt, rows, sc = flat_ip_topk(*ops, q, k, row_offset=row_offset, flags=flags, workspace=workspace, engine=engine)
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), rows.cpu().numpy(), sc.cpu().numpy()


def _prepare_ref(F):
    """Section 1 restated: (b f64[n, d], 1 / s, s) of float32 rows."""
    x = F.astype(np.float64)
    mx = np.abs(x).max(axis=1)
    live = mx >= 1e-30
    b = np.clip(np.rint(x * np.where(live, 127.0 / np.where(live, mx, 1.0), 0.0)[:, None]), -127, 127)
    return b, np.where(live, 127.0 / np.where(live, mx, 1.0), 1.0), np.where(live, mx / 127.0, 0.0)


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_prepare_operands(dev, dim):
    from vectorragquantization_amd.flat import flat_ip_prepare
    rng = np.random.default_rng(100 + dim)
    F = _rows(rng, "float_ip", 70, dim, exact=False)
    F[3] = 0.0
    F[40] = 0.0
    F[40, 5] = 1e-31                                  # below the dead-row limit
    F[11, np.argmax(np.abs(F[11]))] = -2.0            # the row's maximum is negative
    bounds = torch.zeros((2,), dtype=torch.float64, device=dev)
    got = [flat_ip_prepare(torch.from_numpy(F[a:b]).to(dev), bounds) for a, b in ((0, 37), (37, 70))]
    x8 = np.concatenate([g[0].cpu().numpy() for g in got])
    inv = np.concatenate([g[1].cpu().numpy() for g in got])
    b, inv_ref, s = _prepare_ref(F)
    assert np.array_equal(x8, b.astype(np.int8)) and x8[11].min() == -127
    assert np.allclose(inv, inv_ref, rtol=1e-15, atol=0) and inv[3] == inv[40] == 1.0 and not x8[[3, 40]].any()
    ref = np.array([np.linalg.norm(s[:, None] * b, axis=1).max(),
                    np.linalg.norm(F.astype(np.float64) - s[:, None] * b, axis=1).max()])
    bd = bounds.cpu().numpy()
    assert np.all(bd >= ref) and np.all(bd <= ref * (1 + 1e-9)), (bd, ref)


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_parity_per_dim(dev, dim):
    """Two query blocks (the second holds one query), >= 3 chunks, a last chunk of more than one tile whose last
    tile is shifted back; served by the matrix path alone."""
    k = 10
    nq = _plan(100_000, dim, 10_000, k)[7] + 1
    n = next(c for c in range(39, 100_000, 32)
             if _plan(c, dim, nq, k)[1] >= 3 and c % _plan(c, dim, nq, k)[0] > 32)
    assert _plan(n, dim, nq, k)[3] == 2 and n % 32 != 0
    rng = np.random.default_rng(2000 + dim)
    X, qf = _rows(rng, "float_ip", n, dim), _grid_queries(rng, nq, dim)
    out = _run(_prepare(X, dev), qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)
    assert np.all(out[0] == k)
    _assert_exact("float_ip", X, qf, k, out)


@gpu
@pytest.mark.parametrize("dim", (256, 384, 2048))     # R = 8 / 8 with a half-wave piece round / 3
@pytest.mark.parametrize("n,nq,k,row_offset", [(1, 1, 10, 0), (31, 1, 10, 0), (33, 1, 10, 0), (1500, 3, 1, 0),
                                               (1500, 3, 1024, 0), (1500, 3, 10, 7000)])
def test_finish_edges(dev, dim, n, nq, k, row_offset):
    rng = np.random.default_rng(3000 + dim + n + k)
    X, qf = _rows(rng, "float_ip", n, dim), _grid_queries(rng, nq, dim)
    out = _run(_prepare(X, dev), qf, k, dev, row_offset=row_offset, flags=N.VRQ_GEMM_NO_FALLBACK)
    _assert_exact("float_ip", X, qf, k, out, row_offset=row_offset)


def _off_grid(dim, n=4096, nq=8):
    rng = np.random.default_rng(6000 + dim)
    X = _rows(rng, "float_ip", n, dim, exact=False)
    qf = (rng.standard_normal((nq, dim)) * np.exp(rng.standard_normal((nq, dim)))).astype(np.float32)
    return X, qf


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_bound_and_threshold(dev, dim):
    """Delta and thr as the SAMPLE stage leaves them, against f64 NumPy: |u - s'| <= Delta over all rows and
    u >= thr for every row of the oracle's top-k; u by the f32 steps of the hit rule from the prepared operands."""
    k = 10
    X, qf = _off_grid(dim)
    n, nq = X.shape[0], qf.shape[0]
    ops = _prepare(X, dev)
    ws = torch.empty((_plan(n, dim, nq, k)[6],), dtype=torch.uint8, device=dev)
    _run(ops, qf, k, dev, flags=N.VRQ_GEMM_STAGE_SAMPLE, workspace=ws)
    lay = (C.c_int64 * 8)()
    assert N.load().vrq_flat_ip_topk_dim_mfma_prep_layout(n, dim, nq, k, lay) == N.VRQ_OK
    raw = ws.cpu().numpy()
    delta = raw[lay[0]:lay[0] + 8 * nq].view(np.float64)
    thr = raw[lay[4]:lay[4] + 4 * nq].view(np.float32).astype(np.float64)
    inv_s = 127.0 / np.abs(qf).max(axis=1).astype(np.float64)
    a = np.clip(np.rint(qf.astype(np.float64) * inv_s[:, None]), -127, 127)
    assert np.array_equal(raw[:nq * dim].view(np.int8).reshape(nq, dim), a.astype(np.int8))
    dot = (a @ ops[1].cpu().numpy().astype(np.float64).T).astype(np.float32)    # exact integers below 2^25
    u = (dot * (np.float32(1) / ops[2].cpu().numpy().astype(np.float32))).astype(np.float64)
    S = O.flat_ip_scores(X, qf)
    assert np.all(np.abs(u - S * inv_s[:, None]) <= delta[:, None])
    assert np.all(np.take_along_axis(u, O.exhaustive_topk(S, k), 1) >= thr[:, None])
    assert np.all(np.isfinite(thr))


@gpu
@pytest.mark.parametrize("dim", (384, 1536))
def test_off_grid_one_ulp(dev, dim):
    """The inputs of test_bound_and_threshold through the full call: each score within one f32 ulp of the f64
    dot, rows equal to the oracle's wherever its neighbouring scores differ by more than that."""
    k = 10
    X, qf = _off_grid(dim)
    cnt, rows, sc = _run(_prepare(X, dev), qf, k, dev)
    S = X.astype(np.float64) @ qf.astype(np.float64).T
    S = S.T
    ref_rows = O.exhaustive_topk(O.flat_ip_scores(X, qf), k)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    for q in range(qf.shape[0]):
        r, rr = rows[q], ref_rows[q]
        assert cnt[q] == k and np.all(np.abs(sc[q] - S[q, r]) <= ulp(S[q, r])), q
        bad = np.nonzero(r != rr)[0]
        assert np.all(np.abs(S[q, r[bad]] - S[q, rr[bad]]) <= ulp(S[q, rr[bad]])), (q, bad)
        assert np.all(np.diff(sc[q]) <= 0), q


@gpu
@pytest.mark.parametrize("dim", (256, 1536))
def test_identical_rows_overflow_retry_fallback(dev, dim):
    """Identical rows at the smallest n whose chunks exceed the list capacity: every list overflows, the retry
    still admits every row, and the exact scan serves the queries (unserved under VRQ_GEMM_NO_FALLBACK)."""
    nq, k = 3, 10
    rng = np.random.default_rng(4000 + dim)
    row, qf = _rows(rng, "float_ip", 1, dim), _grid_queries(rng, nq, dim)
    n = next(c for c in range(1 << 15, 1 << 22, 1 << 15) if _plan(c, dim, nq, k)[0] > _plan(c, dim, nq, k)[2])
    ops = _prepare(torch.from_numpy(row).to(dev).expand(n, dim).contiguous(), dev)
    cnt, rows, sc = _run(ops, qf, k, dev)
    assert np.all(cnt == k) and np.array_equal(rows, np.tile(np.arange(k), (nq, 1)))
    assert np.array_equal(sc, np.repeat(O.flat_ip_scores(row, qf), k, axis=1))
    assert np.all(_run(ops, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK)[0] == -1)


@gpu
def test_retry_serves_an_overflowed_list(dev):
    """The construction of tests/test_gpu_gemm_dims_mfma.py over float rows: a whole main chunk that no sample
    chunk touches holds grid rows graded towards query 0, the best last.  With the plan's numbers and the oracle's
    scores (n = 557 056, chunks of 544 rows, capacity 512): the graded rows score 14.3 .. 27.0, the k-th best
    sampled row 13.3, and a row at or above that is a hit whatever Delta is (u >= s' - Delta, thr <= U - 2 Delta,
    U <= the k-th best sampled s' + Delta), so all 544 are hits: the list keeps the first 512 and overflows, and
    the true top-k, chunk rows 530 .. 543, is among those it dropped.  The retry at the raised threshold (139 rows
    pass it) must serve the query without the exact scan."""
    dim, nq, k = 256, 3, 10
    n = next(c for c in range(1 << 15, 1 << 22, 1 << 15) if _plan(c, dim, nq, k)[0] > _plan(c, dim, nq, k)[2])
    cr, nchunks, capc, _, nsc, scr = _plan(n, dim, nq, k)[:6]
    sstride = n // nsc
    m = next(c for c in range(nchunks // 2, nchunks - 1)
             if all(not (s * sstride < (c + 1) * cr and c * cr < s * sstride + scr) for s in range(n // sstride + 1)))
    rng = np.random.default_rng(7000)
    X, qf = _rows(rng, "float_ip", n, dim), _grid_queries(rng, nq, dim)
    g = np.linspace(0.8, 1.5, cr)[:, None]
    X[m * cr:(m + 1) * cr] = np.round((qf[0] * g / 14 + 0.004 * rng.standard_normal((cr, dim))) / G) * G
    ops = _prepare(X, dev)
    ws = torch.empty((_plan(n, dim, nq, k)[6],), dtype=torch.uint8, device=dev)
    _run(ops, qf, k, dev, flags=N.VRQ_GEMM_STAGE_SAMPLE | N.VRQ_GEMM_STAGE_MAIN, workspace=ws)
    lay = (C.c_int64 * 8)()
    assert N.load().vrq_flat_ip_topk_dim_mfma_prep_layout(n, dim, nq, k, lay) == N.VRQ_OK
    assert int(ws[lay[6] + 4 * m:lay[6] + 4 * m + 4].cpu().numpy().view(np.int32)[0]) > capc   # (query 0, chunk m)
    out = _run(ops, qf, k, dev, flags=N.VRQ_GEMM_NO_FALLBACK, workspace=ws)
    assert np.all(out[0] == k) and np.any(out[1][0] >= m * cr + capc)       # rows the list had dropped
    _assert_exact("float_ip", X, qf, k, out)


class _FloatProvider:
    """provider.embed over the fake HTTP service of tests/golden/fake_services.py (its table holds float rows)."""

    def __init__(self, table):
        from tests.golden.fake_services import FakeCohereRequests
        self.http = FakeCohereRequests(table)

    def embed(self, texts, input_type, embedding_types):
        r = self.http.post("/v2/embed", json={"texts": list(texts), "input_type": input_type})
        return {"float": r.json()["embeddings"]["int8"]}


@gpu
@pytest.mark.parametrize("dim", (384, 2048))
def test_class_surface(dev, dim, tmp_path):
    from vectorragquantization_amd.flat import CohereVectorDBFloat, FloatIndexIDMap
    rng = np.random.default_rng(31 + dim)
    F, q = _rows(rng, "float_ip", 700, dim), _grid_queries(rng, 5, dim)
    ids = np.arange(700, dtype=np.int64) * 3 + 5
    idx, ref = FloatIndexIDMap(dim, dev, engine="mfma"), FloatIndexIDMap(dim, dev)
    for ix in (idx, ref):
        ix.add_with_ids(F[:100], ids[:100])
        ix.add_with_ids(F[100:], ids[100:])
        assert ix.remove_ids(ids[[50, 650]]) == 2
    assert ref._x8 is None and idx._x8.view().shape == (698, dim) and idx._inv.view().shape == (698,)
    idx2 = FloatIndexIDMap.from_bytes(idx.to_bytes(), dev, engine="mfma")
    D, L = ref.search(q, 20)
    for ix in (idx, idx2):
        D2, L2 = ix.search(q, 20)
        assert np.array_equal(L2, L) and np.array_equal(D2.view(np.int32), D.view(np.int32))
    docs = [f"document number {i}" for i in range(300)]
    prov = _FloatProvider({d: F[i] for i, d in enumerate(docs)})
    res = []
    for e in ("auto", None):
        db = CohereVectorDBFloat(str(tmp_path / f"db_{e}"), embedding_dim=dim, provider=prov, device=dev, engine=e)
        db.add_documents(list(range(300)), docs, batch_size=64, save=False)
        res.append([db.search(docs[j], k=5) for j in (0, 42)])
    assert res[0] == res[1] and res[0][1][0]["doc_id"] == 42


def test_plan_workspace_validation_engine():
    lib = N.load()
    call = lib.vrq_flat_ip_topk_dim_mfma
    for dim in DIMS:
        for n, nq, k in ((1, 1, 1), (5000, 3, 1024), (10_000_000, 1024, 10)):
            p = _plan(n, dim, nq, k)
            assert p[6] == lib.vrq_flat_ip_topk_dim_mfma_workspace_size(n, dim, nq, k) > 0
            assert p[0] % 32 == 0 and p[1] * p[0] >= n > (p[1] - 1) * p[0] and p[3] * p[7] >= nq > (p[3] - 1) * p[7]
        for n in (1000, 1_000_000, 10_000_000):
            assert lib.vrq_flat_ip_dim_engine(n, dim, 1, 10) == N.VRQ_GEMM_ENGINE_EXACT
    assert (lib.vrq_flat_ip_topk_dim_mfma_workspace_size(1000, 1024, 1, 10)
            == lib.vrq_gemm_topk_workspace_size(N.VRQ_GEMM_FLOAT_IP, 1000, 1024, 1, 10) > 0)
    k5, mine = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    assert lib.vrq_gemm_topk_plan(N.VRQ_GEMM_FLOAT_IP, 1000, 1024, 1, 10, k5) == N.VRQ_OK
    assert lib.vrq_flat_ip_topk_dim_mfma_plan(1000, 1024, 1, 10, mine) == N.VRQ_OK and list(k5) == list(mine)
    info = (C.c_int64 * 8)()
    for n, dim, k in ((1000, 1032, 10), (1000, 384, 1025), (1 << 32, 384, 10)):
        assert lib.vrq_flat_ip_topk_dim_mfma_plan(n, dim, 1, k, info) == N.VRQ_EUNSUPPORTED
        assert lib.vrq_flat_ip_topk_dim_mfma_workspace_size(n, dim, 1, k) == 0
        assert call(P8, P8, P8, P8, n, dim, 0, P8, 1, k, 0, P8, P8, P8, P8, 1 << 40, None) == N.VRQ_EUNSUPPORTED
    assert lib.vrq_flat_ip_prepare_dim(P8, 10, 1032, P8, P8, P8, None) == N.VRQ_EUNSUPPORTED
    assert call(P8, P8, P8, P8, 1000, 384, 0, P8, 1, 10, N.VRQ_GEMM_SCAN_EXACT, P8, P8, P8, P8, 1 << 40,
                None) == N.VRQ_EUNSUPPORTED
    assert call(P8, P8, P8, P8, 1000, 384, 0, P8, 1, 10, 0, P8, P8, P8, P8, 16, None) == N.VRQ_EWORKSPACE
    for miss in range(1, 4):                          # x8, inv_scale, bounds
        ops = [None if i == miss else P8 for i in range(4)]
        assert call(*ops, 1000, 384, 0, P8, 1, 10, 0, P8, P8, P8, P8, 1 << 40, None) == N.VRQ_EINVAL
    assert [N.flat_ip_engine(lib, 1000, 768, 64, 10, e) for e in (None, "exact", "mfma")] == [None, "exact", "mfma"]
    assert N.flat_ip_engine(lib, 1_000_000, 768, 1, 10, "auto") is None
    assert N.flat_ip_engine(lib, 1_000_000, 768, 64, 10, "auto") == "mfma"      # profiles/flat_mfma_bench.jsonl
    assert N.flat_ip_engine(lib, 1_000_000, 1024, 1024, 10, "auto") is None
    from vectorragquantization_amd.flat import flat_ip_topk
    x = torch.zeros((4, 384))
    with pytest.raises(N.VrqNativeError, match="needs x8"):
        flat_ip_topk(x, None, None, None, x[:1], 2, engine="mfma")
