"""The entry points that share the Phase-I route agree on the GPU: vrq_hamming_topk and vrq_search3_dim with
VRQ_SEARCH_PHASE1_ONLY (whole call, and staged scan + finish) return the same lists on both routes, equal to
the NumPy Hamming top-K of oracle/oracle_np.py in (distance, row) order, exactly.  n = 65 543 is just above
the smallest row count at which both routes exist (the matrix-core scans start at 65 536 rows) and no
multiple of a tile or a chunk."""
import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from vectorragquantization_amd import _native as N

pytestmark = pytest.mark.gpu

N_ROWS, NQ, K = 65_543, 3, 10
DIMS = (256, 1024, 1536)
P1 = N.VRQ_SEARCH_PHASE1_ONLY
_CASE = {}


def _case(d):
    """Seeded codes and queries of one dim on the device, the oracle's lists and vrq_hamming_topk's: once."""
    if d not in _CASE:
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(9000 + d)
        codes_np = rng.integers(0, 256, (N_ROWS, d // 8), dtype=np.uint8)
        qb_np = rng.integers(0, 256, (NQ, d // 8), dtype=np.uint8)
        qb_np[1] = codes_np[N_ROWS - 1]            # an exact hit in the last, partial tile
        codes_np[77] = codes_np[40_000]            # equal distances: the order falls to the row
        D, I = O.binary_flat_search(codes_np, qb_np, K)
        codes, qb = torch.from_numpy(codes_np).to(dev), torch.from_numpy(qb_np).to(dev)
        lib = N.load()
        ws = torch.empty((lib.vrq_hamming_topk_workspace_size(N_ROWS, d // 8, NQ, K),), dtype=torch.uint8, device=dev)
        rows = torch.empty((NQ, K), dtype=torch.int64, device=dev)
        dist = torch.empty((NQ, K), dtype=torch.int32, device=dev)
        N.check(lib.vrq_hamming_topk(N.ptr(codes), N_ROWS, d // 8, 0, N.ptr(qb), NQ, K, N.ptr(dist), N.ptr(rows),
                                     N.ptr(ws), ws.numel(), N.stream_handle(dev)), "vrq_hamming_topk")
        torch.cuda.synchronize()
        _CASE[d] = (codes, qb, D, I, dist.cpu().numpy(), rows.cpu().numpy())
    return _CASE[d]


def _phase1(d, codes, qb, flags, staged):
    lib, dev = N.load(), codes.device
    ws = torch.empty((lib.vrq_search3_dim_workspace_size(N_ROWS, d, NQ, K),), dtype=torch.uint8, device=dev)
    cnt = torch.empty((NQ,), dtype=torch.int32, device=dev)
    rows = torch.empty((NQ, K), dtype=torch.int64, device=dev)
    dist = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    st = N.stream_handle(dev)
    if staged:
        N.check(lib.vrq_search3_dim_scan(N.ptr(codes), N_ROWS, d, N.ptr(qb), NQ, K, flags, N.ptr(ws), ws.numel(), st),
                "vrq_search3_dim_scan")
        N.check(lib.vrq_search3_dim_finish(N.ptr(codes), 0, 0, 0, N_ROWS, d, 0, 0, NQ, K, K, K, flags | P1,
                                           N.ptr(cnt), N.ptr(rows), N.ptr(dist), 0, 0, N.ptr(ws), ws.numel(), st),
                "vrq_search3_dim_finish")
    else:
        N.check(lib.vrq_search3_dim(N.ptr(codes), 0, 0, 0, N_ROWS, d, 0, 0, N.ptr(qb), NQ, K, K, K, flags | P1,
                                    N.ptr(cnt), N.ptr(rows), N.ptr(dist), 0, 0, N.ptr(ws), ws.numel(), st),
                "vrq_search3_dim")
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [K] * NQ
    return dist.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("route", (N.VRQ_SEARCH_SCAN_VALU, N.VRQ_SEARCH_SCAN_MFMA), ids=("wavefront", "matrix"))
@pytest.mark.parametrize("d", DIMS)
def test_entry_points_agree_on_both_routes(d, route):
    lib = N.load()
    codes, qb, D, I, topk_dist, topk_rows = _case(d)
    want_kind = N.VRQ_SCAN_KIND_MFMA if route == N.VRQ_SEARCH_SCAN_MFMA else N.VRQ_SCAN_KIND_VALU
    assert lib.vrq_scan_kind(N_ROWS, d, NQ, K, route, None) == want_kind
    # vrq_hamming_topk (no flags: the default choice, the matrix-core scan at this shape) against the oracle
    assert lib.vrq_scan_kind(N_ROWS, d, NQ, K, 0, None) == N.VRQ_SCAN_KIND_MFMA
    assert np.array_equal(topk_dist, D) and np.array_equal(topk_rows, I)
    # the staged search with the route forced
    dist, rows = _phase1(d, codes, qb, route, staged=True)
    assert np.array_equal(dist, D) and np.array_equal(rows, I)
    assert np.array_equal(dist, topk_dist) and np.array_equal(rows, topk_rows)
    # the whole call: the dims other than 1024 take SCAN_VALU only, their matrix route is the default choice
    dist, rows = _phase1(d, codes, qb, route if route == N.VRQ_SEARCH_SCAN_VALU or d == 1024 else 0, staged=False)
    assert np.array_equal(dist, D) and np.array_equal(rows, I)
    assert np.array_equal(dist, topk_dist) and np.array_equal(rows, topk_rows)
