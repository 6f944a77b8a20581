#!/usr/bin/env python
"""The per-shard calls and merges of the sharded search beside the single-index calls they mirror: HIP-event
timing on the same device buffers in the same run, the legs alternating for ``--rounds`` rounds.

Per dim (1M rows, nq = 1024, k = 10, K = 100 by default), on preallocated buffers:

* ``scan``         ``vrq_search3_dim_scan`` alone (every call below starts with it);
* ``search3``      ``vrq_search3_dim``: scan + the three-phase finish (Phase III for K3 = 30 survivors, two sorts);
* ``shard3``       ``vrq_shard_search3``: scan + the shard finish (Phase III for all K candidates, no sort);
* ``search2``      ``vrq_search2`` (mode sbin): scan + score + sort;
* ``shard2``       ``vrq_shard_search2`` (mode sbin): scan + score, no sort;
* ``merge3``, ``merge2``  ``vrq_merge_shards`` / ``vrq_merge_shards2`` over the outputs of two half-corpus shards.

A finish is its call minus ``scan``.  Before timing, the merged results of the two half-corpus shards are
compared with the single-index results bit for bit.  One JSON line per dim; times in ms are the median over
the rounds with the min and max beside it.  Random codes and int8 rows (the timing does not depend on their
values); queries are corpus rows with d/16 .. d/4 flipped bits.

    python tools/shard_bench.py --out profiles/shard_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.search2_bench import reps_for, summary, window  # noqa: E402
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd import dist as D  # noqa: E402
from vectorragquantization_amd import quant as Q  # noqa: E402
from vectorragquantization_amd import synth  # noqa: E402
from vectorragquantization_amd.enhanced import search3  # noqa: E402

K_OUT, OVERSAMPLE, INT8_OVERSAMPLE = 10, 10, 3
SBIN = N.VRQ_RESCORE_SIGNED_BINARY


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--dims", default="384,1536")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = N.load()
    out = open(a.out, "a") if a.out else None
    n, nq, k = a.n, a.nq, K_OUT
    K, K3 = min(k * OVERSAMPLE, n), k * INT8_OVERSAMPLE
    for d in (int(x) for x in a.dims.split(",")):
        codes = synth.random_codes(n, d // 8, device=dev)
        x8 = torch.randint(-127, 128, (n, d), dtype=torch.int8, device=dev)
        norms = Q.int8_row_norms(x8)
        qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
        qf = torch.randn((nq, d), device=dev) / d ** 0.5
        # two half-corpus shards, merged, against the single index
        h = n // 2
        sh3 = [D.shard_search3(codes[r0:r1], x8[r0:r1], norms[r0:r1], qf, qb, K, 0, r0) for r0, r1 in ((0, h), (h, n))]
        sh2 = [D.shard_search2("sbin", codes[r0:r1], codes[r0:r1], qf, qb, K, None, 0.0, 0, r0)
               for r0, r1 in ((0, h), (h, n))]
        st3 = [torch.stack(t) for t in zip(*sh3)]
        st2 = [torch.stack(t) for t in zip(*sh2)]
        same3 = all(torch.equal(x, y) for x, y in zip(D.merge_shards(*st3, k, K3),
                                                      search3(codes, x8, norms, qf, qb, k, K, K3)))
        same2 = all(torch.equal(x, y) for x, y in zip(Q.merge_shards2(*st2, k)[1:4],
                                                      Q.search2("sbin", codes, codes, qf, qb, k, OVERSAMPLE)))
        need = lib.vrq_search3_dim_workspace_size(n, d, nq, K)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
        rows = torch.empty((nq, K), dtype=torch.int64, device=dev)
        dd = torch.empty((nq, K), dtype=torch.int32, device=dev)
        s2 = torch.empty((nq, K), dtype=torch.float64, device=dev)
        s3 = torch.empty((nq, K), dtype=torch.float64, device=dev)
        src = torch.empty((nq, k), dtype=torch.int32, device=dev)
        st = N.stream_handle(dev)
        P = N.ptr
        outs3 = (P(cnt), P(rows), P(dd), P(s2), P(s3))
        outs2 = (P(cnt), P(rows), P(dd), P(s2))
        three = (P(codes), P(x8), P(norms), 0, n, d, 0, P(qf), P(qb), nq)           # ... up to nq
        two = (SBIN, P(codes), P(codes), 0, 0.0, 0, n, d, 0, P(qf), P(qb), nq)
        tail = (P(ws), need, st)
        legs = {
            "scan": lambda: lib.vrq_search3_dim_scan(P(codes), n, d, P(qb), nq, K, 0, *tail),
            "search3": lambda: lib.vrq_search3_dim(*three, k, K, K3, 0, *outs3, *tail),
            "shard3": lambda: lib.vrq_shard_search3(*three, K, 0, *outs3, *tail),
            "search2": lambda: lib.vrq_search2(*two, k, K, 0, *outs2, *tail),
            "shard2": lambda: lib.vrq_shard_search2(*two, K, 0, *outs2, *tail),
            "merge3": lambda: lib.vrq_merge_shards(2, nq, K, *(P(t) for t in st3), k, K3, *outs3, P(src), st),
            "merge2": lambda: lib.vrq_merge_shards2(2, nq, K, *(P(t) for t in st2), k, *outs2, P(src), st),
        }
        for name, call in legs.items():                   # every call succeeds before it is timed
            N.check(call(), name)
        reps = {name: reps_for(call, a.warmup) for name, call in legs.items()}
        times = {name: [] for name in legs}
        for _ in range(a.rounds):                         # alternate the legs round by round
            for name, call in legs.items():
                times[name].append(window(call, reps[name]))
        kind = "mfma" if lib.vrq_scan_kind(n, d, nq, K, 0, None) == N.VRQ_SCAN_KIND_MFMA else "valu"
        rec = {"dim": d, "n": n, "nq": nq, "k": k, "K": K, "K3": K3, "scan_kind": kind,
               "merged_equal_single": bool(same3 and same2), "rounds": a.rounds, "reps": reps}
        for name in legs:
            rec[name] = summary(times[name])
        for name in ("search3", "shard3", "search2", "shard2"):
            rec[name + "_finish_ms"] = round(rec[name]["ms"] - rec["scan"]["ms"], 4)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del legs, codes, x8, norms, ws, sh3, sh2, st3, st2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
