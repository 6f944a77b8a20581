"""Accumulator seeds of K1m's MB = 4 instance (hamming_mfma.hip): where a seed can go wrong.

The thresholded pass folds tau'(q)/2 = (tau(q) - pc(q))/2 into the accumulators: the seeds of the first NSR
M-blocks of a wave stay in registers as the C operand of every n-block's first MFMA, the others are re-read
from LDS after each epilogue, and one compare of the lane's maximum over all its accumulators decides whether
an n-block holds a candidate.  A seed in the wrong M-block's or register's slot, a padded or masked query that
accepts, or an n-block whose first MFMA misses its C operand changes a candidate list, so every case

* asserts through ``vrq_scan_plan`` that the shape runs K1m with 4 M-blocks per wave (kind 0, MB 4):
  n = 4 200 007 rows (n * nq > 2^32, a ragged last tile), the smallest shape that reaches it;
* runs PREFIX + MATRIX + RECHECK by stage and requires every (query, chunk) list to hold exactly the rows with
  dist < tau(q), each once, with its exact distance, against an exact GEMM of the bit matrices
  (``check_scan_lists`` of test_gpu_lists.py);
* requires the final top-K of the planted queries plus a spread sample to equal the C restatement of
  ``hammings_knn_hc``.

Query q of a batch sits in workgroup q // 512, wave (q % 512) // 128, M-block (q % 128) // 32 and, with
i = q % 32, in lane half (i >> 2) & 1 at accumulator register (i & 3) + 4 (i >> 3).

The corpus has 4 200 007 = 65 625 * 64 + 7 rows and the plan's chunks are whole tiles, so the last, partial
tile holds 7 rows, all in its first n-block: no row exists in its second n-block.  Case 3 therefore plants
in that partial tile's first n-block (whose epilogue runs beside the masked second n-block), in the second
n-block of the last whole tile, and in the second n-block of chunk 0's last tile, which is the n-block the
epilogue after the tile loop extracts.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_k1m_edges import N_BIG, _assert_k1m4, _check, _flip, _paths, _phase1, _sample_rows, _sel
from tests.test_gpu_lists import _al, _scan_stages, check_scan_lists

pytestmark = pytest.mark.gpu

K = 100


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vectorragquantization_amd import _native
    _native.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def base(dev):
    """Uniform random codes, generated once and never written: every case plants into a clone."""
    from vectorragquantization_amd import synth
    return synth.random_codes(N_BIG, device=dev, seed=7100)


def _queries(codes, nq, seed):
    from vectorragquantization_amd import synth
    return synth.flip_queries(codes, nq, seed=seed)[0]


def _taus(codes, qb):
    """(tau the pass ran with, tau' = tau - pc(q), re-run flags) per query, from the stage-split ABI."""
    from vectorragquantization_amd import _native as N
    nq = qb.shape[0]
    info, ws = _scan_stages(codes, qb, K, (N.VRQ_SCAN_STAGE_PREFIX, N.VRQ_SCAN_STAGE_MATRIX, N.VRQ_SCAN_STAGE_RECHECK))
    off_tau, j = int(info[7]), int(info[9])
    qa = _al(4 * nq)
    tau_s = ws[off_tau:off_tau + 4 * nq].view(torch.int32).long()
    tau_p = ws[off_tau + qa:off_tau + qa + 4 * nq].view(torch.int32).long()
    rerun = ws[off_tau + 2 * qa:off_tau + 2 * qa + 4 * nq].view(torch.int32) != 0
    tau = torch.where(rerun, tau_p, tau_s if j < K else tau_p)
    pcq = torch.from_numpy(np.unpackbits(qb.cpu().numpy(), axis=1).sum(1).astype(np.int64)).to(tau.device)
    return tau.cpu().numpy(), (tau - pcq).cpu().numpy(), rerun.cpu().numpy()


def _lists_and_topk(oracle_lib, codes, qb, planted, dev, allow_overflow=False):
    info = check_scan_lists(codes, qb, K, allow_overflow=allow_overflow)
    assert (int(info[0]), int(info[1])) == (0, 4)
    nq = qb.shape[0]
    c, D1, I1 = _phase1(codes, qb.cpu().numpy(), K, dev)
    assert np.array_equal(c, np.full(nq, K))
    return _check(oracle_lib, codes.cpu().numpy(), qb.cpu().numpy(), K, D1, I1, _sel(planted, nq))


def test_k1m_seeds_padded_last_block(dev, oracle_lib, base):
    """nq = 1100: the third 512-query block holds 76 queries -- M-blocks 0 and 1 of its first wave whole,
    M-block 2 with 12 real and 20 padded queries, M-block 3 and the other three waves padded.  A padded
    query's seed must never accept (its lists would be written past nq, or into a neighbour's)."""
    nq = 1100
    _assert_k1m4(N_BIG, nq, K)
    rng = np.random.default_rng(7101)
    codes = base.clone()
    qb = _queries(codes, nq, 7102)
    planted = [0, 1023, 1024, 1087, 1088, 1099]          # first and last real query of each M-block of the last block
    rows = rng.choice(N_BIG, len(planted), replace=False)
    qn = qb.cpu().numpy()
    codes[torch.from_numpy(rows).to(dev)] = torch.from_numpy(_flip(rng, qn[planted], 3)).to(dev)
    D0, I0 = _lists_and_topk(oracle_lib, codes, qb, planted, dev)
    sel = _sel(planted, nq).tolist()
    for q, r in zip(planted, rows):
        assert D0[sel.index(q), 0] == 3 and I0[sel.index(q), 0] == r


def test_k1m_seeds_distinct_per_mblock(dev, oracle_lib, base):
    """A corpus of bit density 1/4 and queries whose density is set per M-block (wave 1 of block 0 and wave 2 of
    block 1: 0.15 / 0.3 / 0.45 / 0.6): a random row lies at about 256 + pc(q)/2, so the four M-blocks of those
    waves run with thresholds ~75 apart, and tau'(q) = tau(q) - pc(q) is odd for some queries and even for others
    inside every M-block (half-integer seeds next to integer ones).  A seed in another M-block's or register's
    slot then moves a threshold and changes a list."""
    nq = 1024
    _assert_k1m4(N_BIG, nq, K)
    g = torch.Generator(device=dev)
    g.manual_seed(7201)
    codes = base & torch.randint(0, 256, base.shape, generator=g, device=dev, dtype=torch.uint8)
    rng = np.random.default_rng(7202)
    qn = (rng.random((nq, 1024)) < 0.25)
    waves = [128, 512 + 256]
    for qbase in waves:
        for m, p in enumerate((0.15, 0.3, 0.45, 0.6)):
            qn[qbase + 32 * m:qbase + 32 * m + 32] = rng.random((32, 1024)) < p
    qb = torch.from_numpy(np.packbits(qn, axis=1)).to(dev)
    tau, taup, _ = _taus(codes, qb)
    for qbase in waves:
        tm = [tau[qbase + 32 * m:qbase + 32 * m + 32] for m in range(4)]
        for m in range(4):
            par = taup[qbase + 32 * m:qbase + 32 * m + 32] & 1
            assert par.min() == 0 and par.max() == 1, "odd and even tau' inside the M-block"
            if m:
                assert tm[m].min() > tm[m - 1].max(), "the M-blocks' thresholds must differ"
    planted = [qbase + 32 * m + i for qbase in waves for m in range(4) for i in (0, 5, 31)]
    _lists_and_topk(oracle_lib, codes, qb, planted, dev)


def test_k1m_seeds_first_mfma_and_epilogue(dev, oracle_lib, base):
    """One query per lane half of each M-block (wave 1 of block 0, wave 3 of block 1) with near-duplicate rows
    (3 flipped bits) in the first n-block of tile 0, in the second n-block of chunk 0's last tile (extracted by
    the epilogue after the tile loop), in chunk 1's first tile, in the second n-block of the corpus's last whole
    tile and in the 7-row partial tile after it."""
    nq = 1024
    info = _assert_k1m4(N_BIG, nq, K)
    cr, nch = int(info[2]), int(info[3])
    assert cr % 64 == 0 and nch >= 2 and N_BIG % 64 == 7
    rng = np.random.default_rng(7301)
    codes = base.clone()
    qb = _queries(codes, nq, 7302)
    qn = qb.cpu().numpy()
    # i = 3: lane half 0, i = 20: lane half 1
    planted = [qbase + 32 * m + i for qbase in (128, 512 + 384) for m in range(4) for i in (3, 20)]
    nqp = len(planted)
    last_whole = (N_BIG // 64 - 1) * 64
    places = {
        "tile 0, n-block 0": np.arange(nqp) * 2,                              # rows 0 .. 30
        "chunk 0's last tile, n-block 1": cr - 32 + np.arange(nqp) * 2,
        "chunk 1's first tile": cr + np.arange(nqp) * 4,                       # both n-blocks
        "last whole tile, n-block 1": last_whole + 32 + np.arange(nqp) * 2,
        "partial tile": N_BIG - 7 + np.arange(nqp) % 7,                        # 7 rows: the first 7 queries keep theirs
    }
    want = {q: [] for q in planted}
    for name, rows in places.items():
        for i in reversed(range(nqp)):                                         # (partial tile: earlier queries win)
            codes[int(rows[i])] = torch.from_numpy(_flip(rng, qn[planted[i]:planted[i] + 1], 3)[0]).to(dev)
    final = codes[torch.from_numpy(np.concatenate(list(places.values()))).to(dev)].cpu().numpy()
    allrows = np.concatenate(list(places.values()))
    for i, q in enumerate(planted):
        d = np.unpackbits(final ^ qn[q][None, :], axis=1).sum(1)
        want[q] = sorted(set(int(r) for r in allrows[d == 3]))
        assert len(want[q]) >= 4
    D0, I0 = _lists_and_topk(oracle_lib, codes, qb, planted, dev)
    sel = _sel(planted, nq).tolist()
    for q in planted:
        k = len(want[q])
        assert (D0[sel.index(q), :k] == 3).all() and I0[sel.index(q), :k].tolist() == want[q]


def test_k1m_seeds_rerun_masked_queries(dev, oracle_lib, base):
    """The sampled threshold tau_s fails for a query of M-block 0 and one of M-block 3 of one wave, and for one
    in the second 512-query block (70 near copies on sample rows, 40 more at distance 30 off the sample): the
    re-run pass masks every other query of those blocks through ``rerun[]`` -- their seeds are the padded value,
    next to live seeds in the same M-block -- and must recover the first 30 distance-30 rows in row order."""
    nq = 1024
    info = _assert_k1m4(N_BIG, nq, K)
    assert int(info[9]) < K, "the plan must take the sampled threshold"
    rng = np.random.default_rng(7401)
    codes = base.clone()
    qb = torch.from_numpy(_flip(rng, codes[torch.from_numpy(rng.integers(0, N_BIG, nq)).to(dev)].cpu().numpy(), 50)).to(dev)
    qn = qb.cpu().numpy()
    samp = _sample_rows(N_BIG, nq, K)
    insamp = np.zeros(N_BIG, bool)
    insamp[samp] = True
    planted = [256 + 5, 256 + 96 + 20, 512 + 96 + 9]      # wave 2 of block 0: M-blocks 0 and 3; block 1: M-block 3
    near_all = rng.choice(samp, 70 * len(planted), replace=False)
    far_all = rng.integers(0, N_BIG, 800)
    far_all = rng.permutation(np.unique(far_all[~insamp[far_all]]))[:40 * len(planted)]
    assert far_all.size == 40 * len(planted)
    for i, q in enumerate(planted):
        near = near_all[70 * i:70 * (i + 1)]
        codes[torch.from_numpy(near).to(dev)] = torch.from_numpy(
            _flip(rng, np.repeat(qn[q:q + 1], 70, axis=0), int(rng.integers(5, 21)))).to(dev)
        far = far_all[40 * i:40 * (i + 1)]
        codes[torch.from_numpy(far).to(dev)] = torch.from_numpy(_flip(rng, np.repeat(qn[q:q + 1], 40, axis=0), 30)).to(dev)
    _, rerun = _paths(codes, qn, K)
    assert rerun[planted].all(), "the planted queries must fail tau_s and re-run with tau_p"
    assert not rerun[[256 + 4, 256 + 96 + 21]].any(), "their neighbours in the M-block stay masked in the re-run"
    D0, _ = _lists_and_topk(oracle_lib, codes, qb, planted, dev)
    sel = _sel(planted, nq).tolist()
    for q in planted:
        assert (D0[sel.index(q)] == 30).sum() == 30
