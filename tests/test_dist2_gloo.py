"""The sharded two-phase search and the sharded search at another dim on CPU (gloo, world_size 2), in the
pattern of tests/test_dist_gloo.py: the 28-byte candidate packing, the single all-gather, and -- with the
CPU oracle standing in for the per-shard kernels (test infrastructure) -- that a host restatement of
``vrq_merge_shards2`` / ``vrq_merge_shards`` over the gathered candidates equals the single-corpus result
built from the same oracle functions.  The kernels themselves are checked against the single-index calls
in tests/test_gpu_shard_dims.py and across real processes in tests/test_gpu_dist_dims.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle_np as O
from tests.test_dist_gloo import _free_port, _merge_oracle, _shard_candidates
from vectorragquantization_amd import synth
from vectorragquantization_amd.dist import (gather_candidates, pack_candidates, pack_candidates2, unpack_candidates,
                                            unpack_candidates2)

DIM, LIMIT = 384, 0.1


def _corpus():
    """dim 384 (48-byte codes), 4000 rows, 12 queries: rows 2100-2199 duplicate rows 0-99 (Hamming and score
    ties across the shard boundary at row 2016), query 0 is all zero (every score ties: row order decides)."""
    rng = np.random.default_rng(321)
    n, nq = 4000, 12
    F = rng.standard_normal((n, DIM)).astype(np.float32) * 0.05
    F[2100:2200] = F[0:100]
    codes, q8, _ = O.encode_batch("int8g", F, LIMIT)
    _, x8, _ = O.encode_batch("cohere", F, LIMIT)
    qf = (F[rng.integers(0, n, nq)] + 0.02 * rng.standard_normal((nq, DIM))).astype(np.float32)
    qf[0] = 0.0
    qb, _, _ = O.encode_batch("int8g", qf, LIMIT)
    return codes, q8, x8, qf, qb


def _scores(q8, qf):
    """The two-phase score of every (query, row), f64 [nq, n]: a function of the query and the row alone."""
    return O.dequant_scores(qf, O.dequantize("int8g", q8, limit=LIMIT, dim=DIM))


def _shard_candidates2(codes, score, qb, r0, r1, K):
    """Oracle stand-in for vrq_shard_search2: this shard's exact top-K by (dist, global row) with scores."""
    nq = qb.shape[0]
    D, I = O.binary_flat_search(codes[r0:r1], qb, K)
    cnt = (I >= 0).sum(1).astype(np.int32)
    rows = np.where(I >= 0, I + r0, -1).astype(np.int64)
    d = D.astype(np.int32)
    sc = np.full((nq, K), np.nan)
    for q in range(nq):
        sc[q, :cnt[q]] = score[q, rows[q, :cnt[q]]]
    return cnt, rows, d, sc


def _merge2_oracle(gc, gr, gd, gs, k):
    """Host restatement of vrq_merge_shards2: top-K by (dist, global row) -> stable sort by score desc
    (Python's sort: -0.0 ties +0.0) -> first k.  Per query (rows, dist, score, src = s*K + p)."""
    S, nq, K = gr.shape
    out = []
    for q in range(nq):
        c = [(int(gd[s, q, p]), int(gr[s, q, p]), float(gs[s, q, p]), s * K + p)
             for s in range(S) for p in range(int(gc[s, q]))]
        c.sort(key=lambda t: (t[0], t[1]))
        c = sorted(c[:K], key=lambda t: -t[2])[:k]
        out.append(([t[1] for t in c], [t[0] for t in c], [t[2] for t in c], [t[3] for t in c]))
    return out


def _single2(codes, score, qb, k, K):
    """The single-corpus two-phase search (CohereVectorDBBinary.py:215-239) from the same oracle functions."""
    D, I = O.binary_flat_search(codes, qb, K)
    out = []
    for q in range(qb.shape[0]):
        c = [(int(D[q, j]), int(I[q, j]), float(score[q, I[q, j]])) for j in range(K) if I[q, j] >= 0]
        c = sorted(c, key=lambda t: -t[2])[:k]
        out.append(([t[1] for t in c], [t[0] for t in c], [t[2] for t in c]))
    return out


def _worker(rank, world, port, result_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    codes, q8, x8, qf, qb = _corpus()
    n, nq, k, osb, osi = codes.shape[0], qf.shape[0], 10, 10, 3
    K = min(k * osb, n)
    r0, r1 = synth.shard_range(n, rank, world)
    ok = 0 < r0 <= 2100 if rank else r1 > 100                     # the duplicates sit in different shards
    # ---- two-phase
    score = _scores(q8, qf)
    cnt, rows, d, sc = _shard_candidates2(codes, score, qb, r0, r1, K)
    ids = np.where(rows >= 0, rows * 3 + 11, -1)                   # external id = 3 row + 11
    buf = gather_candidates(pack_candidates2(*(torch.from_numpy(a) for a in (cnt, rows, ids, d, sc))))
    gc, gr, gi, gd, gs = (x.numpy() for x in unpack_candidates2(buf, world, nq, K))
    merged = _merge2_oracle(gc, gr, gd, gs, k)
    if rank == 0:
        ref = _single2(codes, score, qb, k, K)
        flat_ids = gi.transpose(1, 0, 2).reshape(nq, world * K)    # as ShardedSearch2 gathers them through src
        for q in range(nq):
            ok &= merged[q][0] == ref[q][0] and merged[q][1] == ref[q][1] and merged[q][2] == ref[q][2]
            ok &= flat_ids[q, merged[q][3]].tolist() == [3 * r + 11 for r in ref[q][0]]
        ok &= len(set(ref[0][2])) == 1                             # the zero query: all scores tie,
        ok &= ref[0][0] == O.binary_flat_search(codes, qb[:1], K)[1][0, :k].tolist()   # Phase-I order stays
        ok &= any(r >= 2100 and r < 2200 for q in range(nq) for r in ref[q][0])
    # ---- three-phase at the same dim
    cnt, rows, d, s2, s3 = _shard_candidates(codes, x8, qf, qb, r0, r1, K)
    ids = np.where(rows >= 0, rows + 7, -1)
    buf = gather_candidates(pack_candidates(*(torch.from_numpy(a) for a in (cnt, rows, ids, d, s2, s3))))
    gc, gr, gi, gd, g2, g3 = (x.numpy() for x in unpack_candidates(buf, world, nq, K))
    merged3 = _merge_oracle(gc, gr, gd, g2, g3, k, k * osi)
    if rank == 0:
        ref3 = O.three_phase_batch(codes, x8, np.arange(n) + 7, qf, qb, k, osb, osi)
        ok &= all(merged3[q] == ref3[q]["row"].tolist() for q in range(nq))
        ok &= bool(np.all(gi[gr >= 0] == gr[gr >= 0] + 7))
        result_q.put(bool(ok))
    dist.barrier()
    dist.destroy_process_group()


def test_pack2_unpack2_roundtrip():
    nq, K, S = 5, 7, 3
    parts = []
    for s in range(S):
        g = torch.Generator().manual_seed(s)
        sc = torch.randn((nq, K), dtype=torch.float64, generator=g)
        sc[0, 0], sc[0, 1], sc[1, 0] = -0.0, float("-inf"), float("nan")
        parts.append((torch.randint(0, K, (nq,), dtype=torch.int32, generator=g),
                      torch.randint(-1, 1 << 40, (nq, K), generator=g),
                      torch.randint(-(1 << 62), 1 << 62, (nq, K), generator=g),
                      torch.randint(0, 2049, (nq, K), dtype=torch.int32, generator=g), sc))
    one = pack_candidates2(*parts[0])
    assert one.dtype == torch.uint8 and one.numel() == 4 * nq + 28 * nq * K
    out = unpack_candidates2(torch.cat([pack_candidates2(*p) for p in parts]), S, nq, K)
    for s in range(S):
        for got, want in zip(out, parts[s]):
            assert got[s].dtype == want.dtype
            assert torch.equal(got[s].view(torch.uint8), want.view(torch.uint8))   # bit for bit (NaN, -0.0)


@pytest.mark.timeout(300)
def test_two_rank_gloo_two_phase_and_dim384_equal_single_corpus():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    assert all(p.exitcode == 0 for p in procs)
    assert q.get(timeout=5) is True
