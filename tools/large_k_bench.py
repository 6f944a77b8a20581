#!/usr/bin/env python
"""The search with more than 1024 Phase-I candidates (``vrq_search3_large``: the counting scan K1h + the large
finish) beside the existing ``vrq_search3_dim`` at its largest K: HIP-event timing on the same device buffers
in the same run, the legs alternating for ``--rounds`` rounds.

Per (dim, nq) at 1M rows, k = K / 10, K3 = 3 k, on preallocated buffers:

* ``a_search3_dim_K1024``   the existing ``vrq_search3_dim`` at K = 1024: the yardstick;
* ``b_large_K<K>``          ``vrq_search3_large`` at K = 1024, 2048 and 8192, and its stages through
  ``vrq_scan_large``: ``count``, ``threshold``, ``emit``; ``finish`` = the call minus the whole scan (``scan``).

(The count with and without an upper bound on the counted distances was a third leg while the bound existed:
``profiles/large_k_bench_bound_ab.jsonl`` is that run; the bound bought nothing and was removed.)

Before timing, ``vrq_search3_large`` at K = 1024 is compared with ``vrq_search3_dim`` bit for bit.  One JSON
line per (dim, nq); times in ms are the median over the rounds with the min and max beside it;
``ratio_b1024_over_a`` is leg (b) at K = 1024 over leg (a).  Random codes and int8 rows (unrelated codes: the
distances pile up around dim / 2, the worst case for the histogram atomics); queries are corpus rows with
d/16 .. d/4 flipped bits.

    python tools/large_k_bench.py --out profiles/large_k_bench.jsonl
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

STAGES = {"count": N.VRQ_LARGE_STAGE_COUNT, "threshold": N.VRQ_LARGE_STAGE_THRESHOLD,
          "emit": N.VRQ_LARGE_STAGE_EMIT}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="1024,384")
    ap.add_argument("--nqs", default="1,64")
    ap.add_argument("--Ks", default="1024,2048,8192")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = N.load()
    out = open(a.out, "a") if a.out else None
    n = a.n
    Ks = [int(x) for x in a.Ks.split(",")]
    P = N.ptr
    st = N.stream_handle(dev)
    for d in (int(x) for x in a.dims.split(",")):
        codes = synth.random_codes(n, d // 8, device=dev)
        x8 = torch.randint(-127, 128, (n, d), dtype=torch.int8, device=dev)
        norms = Q.int8_row_norms(x8)
        for nq in (int(x) for x in a.nqs.split(",")):
            qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
            qf = torch.randn((nq, d), device=dev) / d ** 0.5
            Kmax = max(Ks + [1024])
            need = max([lib.vrq_search3_dim_workspace_size(n, d, nq, 1024)] +
                       [lib.vrq_search3_large_workspace_size(n, d, nq, K) for K in Ks])
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)
            cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
            rows = torch.empty((nq, Kmax), dtype=torch.int64, device=dev)
            dd = torch.empty((nq, Kmax), dtype=torch.int32, device=dev)
            s2 = torch.empty((nq, Kmax), dtype=torch.float64, device=dev)
            s3 = torch.empty((nq, Kmax), dtype=torch.float64, device=dev)
            outs = (P(cnt), P(rows), P(dd), P(s2), P(s3))
            three = (P(codes), P(x8), P(norms), 0, n, d, 0, P(qf), P(qb), nq)
            tail = (P(ws), need, st)

            def results(call, k):
                for t in (cnt, rows, dd, s2, s3):
                    t.zero_()
                N.check(call(), "call")
                torch.cuda.synchronize()
                return [cnt.clone()] + [t.reshape(-1)[:nq * k].clone() for t in (rows, dd, s2, s3)]

            legs = {"a_search3_dim_K1024": lambda: lib.vrq_search3_dim(*three, 102, 1024, 306, 0, *outs, *tail)}
            ref = results(legs["a_search3_dim_K1024"], 102)
            for K in Ks:
                k, K3 = K // 10, 3 * (K // 10)
                scan = (P(codes), n, d, P(qb), nq, K)
                legs[f"b_large_K{K}"] = lambda k=k, K=K, K3=K3: lib.vrq_search3_large(*three, k, K, K3, 0, *outs, *tail)
                legs[f"b_large_K{K}_scan"] = lambda scan=scan: lib.vrq_scan_large(*scan, 0, *tail)
                for name, bit in STAGES.items():
                    legs[f"b_large_K{K}_{name}"] = lambda scan=scan, bit=bit: lib.vrq_scan_large(*scan, bit, *tail)
            same = None
            if 1024 in Ks:
                got = results(legs["b_large_K1024"], 102)
                same = all(torch.equal(x, y) for x, y in zip(got, ref))
            # every stage leg runs on a workspace a full scan of its K has filled, in the order the legs are
            # listed (scan, count, threshold, emit): each stage finds its inputs
            for name, call in legs.items():
                N.check(call(), name)
            reps = {name: reps_for(call, a.warmup) for name, call in legs.items()}
            times = {name: [] for name in legs}
            for _ in range(a.rounds):                     # alternate the legs round by round
                for name, call in legs.items():
                    times[name].append(window(call, reps[name]))
            info = (torch.zeros(8, dtype=torch.int64)).numpy()
            rec = {"dim": d, "n": n, "nq": nq, "rounds": a.rounds, "large_K1024_equals_search3_dim": same,
                   "plans": {}}
            for K in Ks:
                N.check(lib.vrq_scan_large_plan(n, d, nq, K, info.ctypes.data), "plan")
                rec["plans"][str(K)] = {"chunk_rows": int(info[0]), "chunks": int(info[1]),
                                        "queries_per_workgroup": int(info[2]),
                                        "workspace_bytes": int(info[7])}
            for name in legs:
                rec[name] = summary(times[name])
            for K in Ks:
                rec[f"b_large_K{K}_finish_ms"] = round(rec[f"b_large_K{K}"]["ms"] - rec[f"b_large_K{K}_scan"]["ms"], 4)
            if 1024 in Ks:
                rec["ratio_b1024_over_a"] = round(rec["b_large_K1024"]["ms"] / rec["a_search3_dim_K1024"]["ms"], 3)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del legs, ws
        del codes, x8, norms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
