"""One rank of tests/test_gpu_dist_large_k.py: the row-sharded search with more than 1024 Phase-I candidates
across real processes.

Started by the test as a child process with WORLD_SIZE / RANK / MASTER_* set; every rank shares cuda:0 of the
one-GPU box and the ``gloo`` group stages the packed candidates through host memory.  Each rank builds only its
row shard of the synthetic corpus and runs, with k = 150 and the default oversample (K = 1500),

* ``ShardedSearch.search_vectors`` = ``vrq_shard_search3_large`` on the shard -> ``pack_candidates`` -> one
  all-gather -> ``vrq_merge_shards_large``;
* ``ShardedSearch2.search_vectors`` with ``mode="sbin"`` = ``vrq_shard_search2_large`` -> ``pack_candidates2`` ->
  one all-gather -> ``vrq_merge_shards2_large``.

Rank 0 then builds the whole corpus and checks every merged tensor, the external ids carried through
``out_src`` included, equal to the single-index call (``enhanced.search3`` / ``quant.search2``, which take the
``_large`` calls for this K).  It writes ``OK`` or the first mismatch to $VRQ_DIST_RESULT and exits non-zero on
a mismatch."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vectorragquantization_amd import synth  # noqa: E402
from vectorragquantization_amd.dist import ShardedSearch, ShardedSearch2, shard_calls  # noqa: E402
from vectorragquantization_amd.enhanced import search3  # noqa: E402
from vectorragquantization_amd.quant import search2  # noqa: E402

DIM, NQ, K_OUT = 384, 8, 150


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    n = int(os.environ.get("VRQ_DIST_ROWS", "30000"))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sh = synth.make_corpus(n, d=DIM, rank=rank, world=world, device=dev)
    codes, x8, norms, row0 = sh["codes"], sh["x8"], sh["norms"], sh["row0"]
    ids = torch.arange(row0, row0 + codes.shape[0], dtype=torch.int64, device=dev) * 3 + 11  # external ids
    qf, qb, _ = synth.make_queries(n, NQ, d=DIM, device=dev)
    msg = "OK"
    if shard_calls(10 * K_OUT)["merge3"] != "vrq_merge_shards_large":
        msg = "K = 1500 does not take the large calls"
    res = ShardedSearch(codes, x8, norms, ids, row0, n).search_vectors(qf, qb, K_OUT, 10, 3)
    got3 = (res.count, res.row, res.hamming, res.binary, res.cosine, res.doc_id)
    c2, i2, r2, d2, s2 = ShardedSearch2("sbin", codes, codes, ids, row0, n).search_vectors(qf, qb, K_OUT, 10)
    torch.cuda.synchronize()
    dist.barrier()
    if rank == 0:
        del codes, x8, norms, sh
        full = synth.make_corpus(n, d=DIM, device=dev)
        fc, fx, fn = full["codes"], full["x8"], full["norms"]
        fids = torch.arange(n, dtype=torch.int64, device=dev) * 3 + 11
        c, r, d, b2, b3 = search3(fc, fx, fn, qf, qb, K_OUT, 10 * K_OUT, 3 * K_OUT)
        ref3 = (c, r, d, b2, b3, torch.where(r >= 0, fids[r.clamp_min(0)], r))
        for nm, a, b in zip(("count", "row", "hamming", "binary", "cosine", "doc_id"), got3, ref3):
            if msg == "OK" and not torch.equal(a, b):
                msg = f"three-phase: merged {nm} differs from the single index"
        if msg == "OK" and not bool((c == K_OUT).all()):
            msg = "three-phase: short result"
        cut = synth.shard_range(n, 1, world)[0]
        if msg == "OK" and not bool((r >= cut).any() and (r < cut).any()):
            msg = "three-phase: every result comes from one shard"
        rr, rd, rs = search2("sbin", fc, fc, qf, qb, K_OUT, 10)
        ref2 = (torch.full_like(c2, K_OUT), torch.where(rr >= 0, fids[rr.clamp_min(0)], rr), rr, rd, rs)
        for nm, a, b in zip(("count", "doc_id", "row", "hamming", "score"), (c2, i2, r2, d2, s2), ref2):
            if msg == "OK" and not torch.equal(a, b):
                msg = f"two-phase: merged {nm} differs from the single index"
        with open(os.environ["VRQ_DIST_RESULT"], "w") as f:
            f.write(msg)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if msg == "OK" else 1)


if __name__ == "__main__":
    main()
