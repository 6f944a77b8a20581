"""GPU checks of the full batch calls (vrq_hamming_topk_batch, vrq_search3_batch, vrq_search2_batch) under
engine MFMA (K1hm): every output array equals, bit for bit, the *_large call (no bitmap) or the *_filtered call
(a bitmap) with the same arguments, and the Phase-I outputs equal a torch xor-popcount reference with the
disallowed rows pushed out of the sort (tests/test_gpu_filtered.py's helpers: no kernel under test appears in a
reference).  The corpus is that module's: 12 325 rows, 17 queries, duplicated rows, zero int8 rows and a
rescore_row map.  Then the Python wrappers: engine="mfma" equals engine=None, engine="auto" takes the engine
vrq_large_engine names."""
import numpy as np
import pytest
import torch

import test_gpu_filtered as F

pytestmark = pytest.mark.gpu

DIMS = (256, 384, 1024, 2048)
MASKS = (None, "r50", "range", "r01", "zeros")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def engines():
    N, _ = F._N()
    return N.VRQ_LARGE_ENGINE_AUTO, N.VRQ_LARGE_ENGINE_VALU, N.VRQ_LARGE_ENGINE_MFMA


def words_of(c, mname):
    return None if mname is None else F.pack(c["masks"][mname], True)


def mask_of(c, mname):
    return np.ones(c["n"], bool) if mname is None else c["masks"][mname]


def hamming_batch(dev, codes_t, q_t, k, words, engine, row_offset=0):
    N, lib = F._N()
    n, cb = codes_t.shape
    nq = q_t.shape[0]
    D = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    R = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    ws = F._ws(lib, "vrq_hamming_topk_batch", n, cb, nq, k, dev, fill=0xC3)
    a = F._allow(dev, words)
    N.check(lib.vrq_hamming_topk_batch(N.ptr(codes_t), n, cb, row_offset, N.ptr(q_t), nq, k, N.ptr(a), N.ptr(D),
                                       N.ptr(R), N.ptr(ws), ws.numel(), N.stream_handle(dev), engine), "hamming_batch")
    torch.cuda.synchronize()
    return D.cpu().numpy(), R.cpu().numpy()


def search3_batch(dev, c, k, K, K3, words, engine, flags=0, row_offset=0):
    N, lib = F._N()
    nq = c["qf"].shape[0]
    kout = K if flags & N.VRQ_SEARCH_PHASE1_ONLY else k
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, kout), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, kout), -7, dtype=torch.int32, device=dev)
    s2 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    s3 = torch.full((nq, kout), -7.0, dtype=torch.float64, device=dev)
    ws = F._ws(lib, "vrq_search3_batch", c["n"], c["dim"], nq, K, dev, fill=0xC3)
    rr = None if c["rr"] is None else torch.from_numpy(c["rr"]).to(dev)
    a = F._allow(dev, words)
    N.check(lib.vrq_search3_batch(N.ptr(c["codes"]), N.ptr(c["x8"]), N.ptr(c["norms"]), N.ptr(rr), c["n"], c["dim"],
                                  row_offset, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, K3, flags, N.ptr(a),
                                  N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3), N.ptr(ws), ws.numel(),
                                  N.stream_handle(dev), engine), "search3_batch")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (cnt, rows, dist, s2, s3))


def search2_batch(dev, c, deq, k, K, words, engine):
    N, lib = F._N()
    nq = c["qf"].shape[0]
    mode, q_t, mm_t, limit = deq
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    dist = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    sc = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    ws = F._ws(lib, "vrq_search2_batch", c["n"], c["dim"], nq, K, dev, fill=0xC3)
    rr = None if c["rr"] is None else torch.from_numpy(c["rr"]).to(dev)
    a = F._allow(dev, words)
    N.check(lib.vrq_search2_batch(mode, N.ptr(c["codes"]), N.ptr(q_t), N.ptr(mm_t), float(limit), N.ptr(rr), c["n"],
                                  c["dim"], 0, N.ptr(c["qf"]), N.ptr(c["qb"]), nq, k, K, 0, N.ptr(a), N.ptr(cnt),
                                  N.ptr(rows), N.ptr(dist), N.ptr(sc), N.ptr(ws), ws.numel(), N.stream_handle(dev),
                                  engine), "search2_batch")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (cnt, rows, dist, sc))


@pytest.mark.parametrize("mname", MASKS)
@pytest.mark.parametrize("dim", DIMS)
def test_hamming_topk_batch(dev, dim, mname):
    _, VALU, MFMA = engines()
    c = F.corpus(dev, dim)
    words, mask = words_of(c, mname), mask_of(c, mname)
    for K, nq in ((10, 1), (1500, 17), (8192, 5)):
        q = c["qb"][:nq].contiguous()
        got = hamming_batch(dev, c["codes"], q, K, words, MFMA, row_offset=3)
        F.same(got, F.hamming(dev, c["codes"], q, K, words, row_offset=3))
        F.same(got, hamming_batch(dev, c["codes"], q, K, words, VALU, row_offset=3))
        D0, R0 = F.ref_phase1(c["dmat"][:nq], mask, K)
        assert np.array_equal(got[0], D0) and np.array_equal(got[1], np.where(R0 >= 0, R0 + 3, -1))


@pytest.mark.parametrize("mname", MASKS)
@pytest.mark.parametrize("dim", DIMS)
def test_search3_batch(dev, dim, mname):
    N, _ = F._N()
    _, _, MFMA = engines()
    c = F.sub(F.corpus(dev, dim), 5)
    assert (c["x8"][::7] == 0).all() and (c["rr"] != np.arange(c["n"])).any()   # zero int8 rows, a rescore_row map
    words, mask = words_of(c, mname), mask_of(c, mname)
    for K, k, K3 in ((1500, 150, 450), (10, 10, 30), (8192, 300, 8192)):
        got = search3_batch(dev, c, k, K, K3, words, MFMA, row_offset=1000)
        F.same(got, F.search3(dev, c, k, K, K3, words, row_offset=1000))
        p1 = search3_batch(dev, c, k, K, K3, words, MFMA, N.VRQ_SEARCH_PHASE1_ONLY, row_offset=1000)
        F.same(p1, F.search3(dev, c, k, K, K3, words, N.VRQ_SEARCH_PHASE1_ONLY, row_offset=1000))
        D1, R1 = F.ref_phase1(c["dmat"], mask, K)
        assert np.array_equal(p1[2], D1) and np.array_equal(p1[1], np.where(R1 >= 0, R1 + 1000, -1))
        assert (p1[0] == min(K, int(mask.sum()))).all()


@pytest.mark.parametrize("mode", ("int8g", "f32", "sbin"))
@pytest.mark.parametrize("dim", DIMS)
def test_search2_batch(dev, dim, mode):
    _, _, MFMA = engines()
    c = F.sub(F.corpus(dev, dim), 5)
    deq = F._deq(dev, c, mode)
    for mname in (None, "r50", "range"):
        words, mask = words_of(c, mname), mask_of(c, mname)
        for K, k in ((1500, 150), (10, 10), (8192, 8192)):
            got = search2_batch(dev, c, deq, k, K, words, MFMA)
            F.same(got, F.search2(dev, c, deq, k, K, words))
            D1, R1 = F.ref_phase1(c["dmat"], mask, K)
            F.same_values(got, F.ref_search2(dev, c, deq, D1, R1, k))


def test_auto_equals_the_named_calls(dev):
    """Outputs do not depend on the engine; which engine AUTO runs is shown by tests/test_gpu_batch_scan.py."""
    AUTO, _, _ = engines()
    for dim in DIMS:
        c = F.corpus(dev, dim)
        for nq, filtered in ((1, 0), (17, 1)):
            words = F.pack(c["masks"]["r50"]) if filtered else None
            q = c["qb"][:nq].contiguous()
            F.same(hamming_batch(dev, c["codes"], q, 1500, words, AUTO), F.hamming(dev, c["codes"], q, 1500, words))


def test_python_wrappers(dev):
    from vectorragquantization_amd import filters, quant
    from vectorragquantization_amd.enhanced import search3 as py_search3
    from vectorragquantization_amd.index import BinaryIndexIDMap2
    c = F.sub(F.corpus(dev, 384), 5)
    allow = filters.row_bitmap(torch.from_numpy(c["masks"]["r50"]).to(dev))
    idx = BinaryIndexIDMap2(384, device=dev)
    idx.add_with_ids(c["codes"], np.arange(c["n"]) * 2)
    rr = torch.from_numpy(c["rr"]).to(dev)
    mode, q_t, mm_t, limit = F._deq(dev, c, "int8g")
    host = lambda ts: tuple(t.cpu().numpy() if torch.is_tensor(t) else t for t in ts)
    for a in (None, allow):
        for engine in ("mfma", "auto", "valu"):
            for K in (10, 2000):
                F.same(idx.search(c["qb"], K, allow=a, engine=engine), idx.search(c["qb"], K, allow=a))
            got = py_search3(c["codes"], c["x8"], c["norms"], c["qf"], c["qb"], 150, 1500, 450, rescore_row=rr,
                             allow=a, engine=engine)
            want = py_search3(c["codes"], c["x8"], c["norms"], c["qf"], c["qb"], 150, 1500, 450, rescore_row=rr, allow=a)
            torch.cuda.synchronize()
            F.same(host(got), host(want))
            for k, bo in ((150, 10), (5, 2)):
                for fn in (quant.search2, quant.vectordb_search):
                    got = fn("int8g", c["codes"], q_t, c["qf"], c["qb"], k=k, binary_oversample=bo, limit=limit,
                             rescore_row=rr, allow=a, engine=engine)
                    want = fn("int8g", c["codes"], q_t, c["qf"], c["qb"], k=k, binary_oversample=bo, limit=limit,
                              rescore_row=rr, allow=a)
                    torch.cuda.synchronize()
                    F.same(host(got), host(want))
