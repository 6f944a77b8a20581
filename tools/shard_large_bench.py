#!/usr/bin/env python
"""The row-sharded search with up to 8192 Phase-I candidates on one GPU: the per-shard call
``vrq_shard_search3_large`` over 1, 2, 4 and 8 row ranges searched one after another, the merge
``vrq_merge_shards_large`` of their stacked outputs, and the single-index ``vrq_search3_large`` of the same shape;
at K = 1024 also the existing ``vrq_shard_search3`` + ``vrq_merge_shards``.  HIP-event timing on the same device
buffers in the same run, the legs alternating for ``--rounds`` rounds.

Per (dim, K, shards) at 1M rows, nq = 8, k = K / 10, K3 = 3 k, on preallocated buffers:

* ``shards_large``   all S ``vrq_shard_search3_large`` calls (``per_shard_ms`` = that over S);
* ``merge_large``    ``vrq_merge_shards_large`` on the stacked [S, nq, K] outputs;
* ``single_large``   ``vrq_search3_large`` over the whole corpus;
* ``shards_k1024`` / ``merge_k1024``   at K = 1024 only: ``vrq_shard_search3`` and ``vrq_merge_shards``.

Before timing, the merged result is compared with the single-index one bit for bit (and at K = 1024 the existing
calls' with the large ones').  One JSON line per (dim, K, shards); times in ms are the median over the rounds
with the min and max beside it.  Random codes and int8 rows; queries are corpus rows with d/16 .. d/4 flipped
bits.

    python tools/shard_large_bench.py --out profiles/shard_large_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.search2_bench import reps_for, summary, window  # noqa: E402
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd import quant as Q  # noqa: E402
from vectorragquantization_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="1024,384")
    ap.add_argument("--nq", type=int, default=8)
    ap.add_argument("--Ks", default="1024,2048,8192")
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = N.load()
    out = open(a.out, "a") if a.out else None
    n, nq = a.n, a.nq
    P = N.ptr
    st = N.stream_handle(dev)
    for d in (int(x) for x in a.dims.split(",")):
        codes = synth.random_codes(n, d // 8, device=dev)
        x8 = torch.randint(-127, 128, (n, d), dtype=torch.int8, device=dev)
        norms = Q.int8_row_norms(x8)
        qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
        qf = torch.randn((nq, d), device=dev) / d ** 0.5
        for K in (int(x) for x in a.Ks.split(",")):
            k, K3 = K // 10, 3 * (K // 10)
            need = lib.vrq_search3_large_workspace_size(n, d, nq, K)
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)
            o = [torch.empty((nq,), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev),
                 torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float64, device=dev),
                 torch.empty((nq, k), dtype=torch.float64, device=dev), torch.empty((nq, k), dtype=torch.int32, device=dev)]

            def single():
                return lib.vrq_search3_large(P(codes), P(x8), P(norms), 0, n, d, 0, P(qf), P(qb), nq, k, K, K3, 0,
                                             *(P(t) for t in o[:5]), P(ws), need, st)

            def result(call):
                for t in o:
                    t.zero_()
                N.check(call(), "call")
                torch.cuda.synchronize()
                return [t.clone() for t in o[:5]]

            ref = result(single)
            for S in (int(x) for x in a.shards.split(",")):
                cuts = [n * s // S for s in range(S + 1)]
                g = [torch.empty((S, nq), dtype=torch.int32, device=dev),
                     torch.empty((S, nq, K), dtype=torch.int64, device=dev),
                     torch.empty((S, nq, K), dtype=torch.int32, device=dev),
                     torch.empty((S, nq, K), dtype=torch.float64, device=dev),
                     torch.empty((S, nq, K), dtype=torch.float64, device=dev)]
                sizes = {cuts[s + 1] - cuts[s] for s in range(S)}
                sneed = max(max(lib.vrq_shard_search3_large_workspace_size(m, d, nq, K),
                                lib.vrq_shard_search3_workspace_size(m, d, nq, K)) for m in sizes)  # (0 past 1024)
                sws = torch.empty((sneed,), dtype=torch.uint8, device=dev)
                mneed = lib.vrq_merge_shards_large_workspace_size(S, nq, K)
                mws = torch.empty((mneed,), dtype=torch.uint8, device=dev)

                def shards(fn):
                    rc = 0
                    for s in range(S):
                        lo, m = cuts[s], cuts[s + 1] - cuts[s]
                        rc |= fn(P(codes[lo:]), P(x8[lo:]), P(norms[lo:]), 0, m, d, lo, P(qf), P(qb), nq, K, 0,
                                 *(P(t[s]) for t in g), P(sws), sneed, st)
                    return rc

                legs = {"shards_large": lambda: shards(lib.vrq_shard_search3_large),
                        "merge_large": lambda: lib.vrq_merge_shards_large(S, nq, K, *(P(t) for t in g), k, K3,
                                                                          *(P(t) for t in o), P(mws), mneed, st),
                        "single_large": single}
                N.check(legs["shards_large"](), "shards_large")
                rec = {"dim": d, "n": n, "nq": nq, "K": K, "k": k, "K3": K3, "shards": S, "rounds": a.rounds,
                       "all_gather_bytes_per_rank": nq * 4 + nq * K * 36}
                got = result(legs["merge_large"])
                rec["merged_equals_single_index"] = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8))
                                                        for x, y in zip(got, ref))
                if K <= N.VRQ_K_MAX:
                    legs["shards_k1024"] = lambda: shards(lib.vrq_shard_search3)
                    legs["merge_k1024"] = lambda: lib.vrq_merge_shards(S, nq, K, *(P(t) for t in g), k, K3,
                                                                       *(P(t) for t in o), st)
                    large = [t.clone() for t in g]
                    N.check(legs["shards_k1024"](), "shards_k1024")
                    torch.cuda.synchronize()
                    old = result(legs["merge_k1024"])
                    rec["k1024_calls_equal_large"] = (
                        all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(large, g)) and
                        all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(old, ref)))
                for name, call in legs.items():
                    N.check(call(), name)
                reps = {name: reps_for(call, a.warmup) for name, call in legs.items()}
                times = {name: [] for name in legs}
                for _ in range(a.rounds):                     # alternate the legs round by round
                    for name, call in legs.items():
                        times[name].append(window(call, reps[name]))
                for name in legs:
                    rec[name] = summary(times[name])
                rec["per_shard_ms"] = round(rec["shards_large"]["ms"] / S, 4)
                if "merge_k1024" in legs:
                    rec["merge_large_over_k1024"] = round(rec["merge_large"]["ms"] / rec["merge_k1024"]["ms"], 3)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del legs, g, mws, sws
            del ws
        del codes, x8, norms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
