"""K1m with one counted LDS wait per pair of k-step groups: every list entry, the dense sample's lane minima
and the final top-K at the chunk geometries where the tile loop changes path.

The geometry is the library's own (``vrq_scan_plan``: one chunk per CU, chunks of whole 64-row tiles; the
MFMA scan needs >= 65536 rows), so the short chunks are LAST chunks:

  n            chunks                       steady tiles (all but a chunk's last 4 whole tiles)
  65536        256 x 4 tiles                none
  65601        205 x 5 tiles + 1 row        1; a chunk of one partial tile (1 row)
  65727        205 x 5 + 2 tiles (63 rows)  1; a 2-tile chunk, last tile partial
  65792        205 x 5 + 3 tiles            1; a 3-tile chunk
  98241        256 x 6, last tile 1 row     2 (1 in the last chunk: its refill is partial)
  131071       256 x 8, last tile 63 rows   4 (3 in the last chunk)

MB = 2 runs them all at nq = 200 (and the dense sample pass, always the MB = 2 instance); MB = 4 is K1m's only
above 2^32 (query, row) pairs per pass, so nq = 520 runs at the smallest such n, with a partial last tile.
Near-copies of corpus rows are planted as queries at the first and last row of both n-blocks of a chunk's first
tile, of the tiles on either side of the steady -> tail hand-over and of its last tile: a wait that retired the
wrong fragment or popcount shows as a wrong listed distance or a missing entry.  One tile holds 90 hits of one
wave (> 64: the synchronous flush)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_k1m_edges import _check, _phase1, _plan
from tests.test_gpu_lists import _bits, _dist, _scan_stages, check_scan_lists

pytestmark = pytest.mark.gpu

K = 100
# (n, tiles per full chunk, rows of the last chunk)
SMALL = [(65536, 4, 256), (65601, 5, 1), (65727, 5, 127), (65792, 5, 192), (98241, 6, 321), (131071, 8, 511)]
N_MB4 = 8_260_001  # 520 * n > 2^32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    return torch.device("cuda", 0)


def _flip_bits(rows, nflip, g):
    """Copies of the [m, 128] uint8 rows with nflip distinct bits flipped each."""
    m = rows.shape[0]
    pos = torch.rand((m, 1024), generator=g, device=rows.device).argsort(dim=1)[:, :nflip]
    out = rows.clone()
    for c in range(nflip):
        p = pos[:, c]
        out[torch.arange(m, device=rows.device), p >> 3] ^= (torch.full_like(p, 0x80) >> (p & 7)).to(torch.uint8)
    return out


def _case(n, nq, dev, seed):
    """Uniform codes, queries planted on the rows named in the module docstring.  -> codes, qb, planted queries"""
    from vectorragquantization_amd import synth
    info = _plan(n, nq, K)
    cr, nch = int(info[2]), int(info[3])
    T = cr // 64
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    codes = synth.random_codes(n, device=dev, seed=seed)
    qb = torch.randint(0, 256, (nq, 128), generator=g, device=dev, dtype=torch.uint8)
    # > 64 hits of one wave in one tile: queries 0..8 and ten rows of chunk 1's second tile, all near one code
    base = torch.randint(0, 256, (1, 128), generator=g, device=dev, dtype=torch.uint8)
    qb[:9] = _flip_bits(base.expand(9, 128), 2, g)
    r0 = cr + (64 if T > 1 else 0)
    codes[r0 + 3:r0 + 63:6] = _flip_bits(base.expand(10, 128), 2, g)
    # near-copies of rows at the n-block edges of the first tile, the hand-over tiles and the last tile
    tiles = sorted({0, max(T - 5, 0), max(T - 4, 0), T - 1})
    rows = [c * cr + t * 64 + r for c in (0, nch - 2) for t in tiles for r in (0, 31, 32, 63)]
    rows += [r for r in (n - 1, (nch - 1) * cr) if r not in rows]  # the short last chunk's first and last row
    rows = torch.tensor(rows, device=dev)
    assert int(rows.max()) < n and 9 + rows.numel() <= nq
    qb[9:9 + rows.numel()] = _flip_bits(codes[rows], 3, g)
    return codes, qb, info, np.arange(9 + rows.numel())


def _check_case(codes, qb, info, planted, inst, oracle_lib, dev, nsel):
    assert (int(info[0]), int(info[1])) == inst, "shape does not run K1m MB = %d" % inst[1]
    got = check_scan_lists(codes, qb, K)
    assert np.array_equal(got[:4], info[:4])
    nq = qb.shape[0]
    qsel = np.unique(np.concatenate([planted[:nsel], np.linspace(0, nq - 1, 8).round().astype(np.int64)]))
    c, D1, I1 = _phase1(codes, qb.cpu().numpy(), K, dev)
    assert np.array_equal(c, np.full(nq, K))
    _check(oracle_lib, codes.cpu().numpy(), qb.cpu().numpy(), K, D1, I1, qsel)


@pytest.mark.parametrize("n,tiles,last_rows", SMALL)
def test_k1m2_lists_and_topk_at_chunk_geometries(dev, oracle_lib, n, tiles, last_rows):
    codes, qb, info, planted = _case(n, 200, dev, 7000 + tiles + last_rows)
    cr, nch = int(info[2]), int(info[3])
    assert cr == tiles * 64 and n - (nch - 1) * cr == last_rows, "the plan's chunks are not the ones this case names"
    _check_case(codes, qb, info, planted, (0, 2), oracle_lib, dev, len(planted))


@pytest.mark.parametrize("n,tiles,last_rows", SMALL)
def test_k1m_dense_sample_lane_minima_at_chunk_geometries(dev, n, tiles, last_rows):
    """The dense sample pass (K1m's MB = 2 instance at nq = 200) on the same corpora: every lane minimum."""
    from vectorragquantization_amd import _native as N
    nq = 200
    codes, qb, _, _ = _case(n, nq, dev, 7000 + tiles + last_rows)
    flags = N.VRQ_SEARCH_PHASE1_ONLY | N.VRQ_SEARCH_SCAN_MFMA
    sp = np.zeros(6, np.int64)
    N.check(N.load().vrq_scan_sample_plan(n, 1024, nq, K, flags, sp.ctypes.data), "sample plan")
    rows_sample, nsc, scr, _, ts, cols = (int(x) for x in sp)
    assert rows_sample == 0
    _, ws = _scan_stages(codes, qb, K, (N.VRQ_SCAN_STAGE_PREFIX,))
    dv = ws[:2 * nq * cols].view(torch.int16).view(nq, cols).int() & 0xFFFF
    T = scr // 64
    srows = (torch.arange(nsc * T, device=dev)[:, None] * ts + torch.arange(64, device=dev)[None, :]).reshape(-1)
    assert int(srows.max()) < n
    D = _dist(codes[srows], qb)
    pcq = _bits(qb).sum(1).int()
    want = D.view(nq, nsc, T, 2, 32).amin(dim=(2, 3)).int() - pcq[:, None, None] + 1024
    assert torch.equal(dv, want.view(nq, cols))


def test_k1m4_lists_and_topk_partial_last_tile(dev, oracle_lib):
    codes, qb, info, planted = _case(N_MB4, 520, dev, 7100)
    _check_case(codes, qb, info, planted, (0, 4), oracle_lib, dev, 12)
