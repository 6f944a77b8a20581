#!/usr/bin/env python
"""The per-query filters (``vrq_scan_perquery``: a bitmap per query through the counting scan, K1h or K1hm)
beside the single-bitmap call and beside what a caller without them does -- one ``vrq_scan_batch`` per distinct
filter over that filter's queries: HIP-event timing on the same device buffers in the same run, the legs
alternating for ``--rounds`` rounds, medians (the method of ``tools/filtered_bench.py``).

Per (dim, nq, engine) at 1M rows, K = 1024, per number of sets S (1, 8, 64), per allowed fraction (0.5, 0.1;
every set its own random bits) and per order of the queries (``sorted``: runs of one set; ``interleaved``:
``q % S``):

* ``a_batch``     ``vrq_scan_batch`` with one bitmap (set 0) for every query: the cost of today's call;
* ``b_one_set``   ``vrq_scan_perquery`` with every query in set 0;
* ``c_mixed``     ``vrq_scan_perquery`` with the mixed sets;
* ``d_split``     today's route for mixed sets: one ``vrq_scan_batch`` per distinct set, over that set's
  queries (gathered beforehand, outside the timed region, into per-set query buffers).

Before timing, the K-lists and T / count pairs (c) leaves are compared with those of (d), bit for bit, query by
query.  One JSON line per case; times in ms are the median over the rounds with the min and max beside it.
``b_over_a`` comes with ``a_spread`` = (max - min) / median of (a)'s own rounds, the yardstick for it;
``c_over_d`` is the number the feature exists for.

    python tools/perquery_bench.py --out profiles/perquery_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import search2_bench  # noqa: E402
from tools.search2_bench import reps_for, summary, window  # noqa: E402
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd import filters  # noqa: E402
from vectorragquantization_amd import synth  # noqa: E402

ENGINES = {"valu": N.VRQ_LARGE_ENGINE_VALU, "mfma": N.VRQ_LARGE_ENGINE_MFMA}


def plan(lib, n, d, nq, K, engine):
    info = (N.C.c_int64 * 10)()
    N.check(lib.vrq_scan_batch_plan(n, d, nq, K, engine, info), "plan")
    return [int(v) for v in info]


def lists_of(ws, info, nq, K):
    """(T / count pairs, K-lists sorted per query) a scan left in its workspace."""
    tc = ws[info[7]:info[7] + nq * 8].view(torch.int32).reshape(nq, 2).clone()
    ls = ws[info[8]:info[8] + nq * K * 8].view(torch.int64).reshape(nq, K)
    return tc, torch.sort(ls, dim=1).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="1024,384")
    ap.add_argument("--nqs", default="64,512")
    ap.add_argument("--K", type=int, default=1024)
    ap.add_argument("--sets", default="1,8,64")
    ap.add_argument("--sels", default="0.5,0.1")
    ap.add_argument("--engines", default="valu,mfma")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=search2_bench.MIN_WINDOW_MS)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    search2_bench.MIN_WINDOW_MS = a.window_ms
    dev = torch.device("cuda", 0)
    lib = N.load()
    out = open(a.out, "a") if a.out else None
    n, K = a.n, a.K
    P = N.ptr
    st = N.stream_handle(dev)
    smax = max(int(x) for x in a.sets.split(","))
    for d in (int(x) for x in a.dims.split(",")):
        codes = synth.random_codes(n, d // 8, device=dev)
        for sel in (float(x) for x in a.sels.split(",")):
            g = torch.Generator(device=dev)
            g.manual_seed(int(sel * 1000) + d)
            allow = filters.row_bitmaps(torch.rand((smax, n), generator=g, device=dev) < sel)
            for nq in (int(x) for x in a.nqs.split(",")):
                qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
                need = lib.vrq_scan_batch_workspace_size(n, d, nq, K)
                ws = torch.empty((need,), dtype=torch.uint8, device=dev)
                zeros = torch.zeros((nq,), dtype=torch.int32, device=dev)
                for ename in a.engines.split(","):
                    eng = ENGINES[ename]
                    info = plan(lib, n, d, nq, K, eng)
                    head = (P(codes), n, d)
                    for S in (int(x) for x in a.sets.split(",")):
                        for order in (("sorted",) if S == 1 else ("sorted", "interleaved")):
                            q = np.arange(nq)
                            ids = (q * S) // nq if order == "sorted" else q % S
                            qs = torch.from_numpy(ids.astype(np.int32)).to(dev)
                            # today's route: per distinct set, that set's queries in a buffer of their own
                            parts = []
                            for s in np.unique(ids):
                                idx = torch.from_numpy(np.flatnonzero(ids == s)).to(dev)
                                m = int(idx.shape[0])
                                pws = torch.empty((lib.vrq_scan_batch_workspace_size(n, d, m, K),), dtype=torch.uint8,
                                                  device=dev)
                                parts.append((int(s), idx, qb[idx].contiguous(), m, pws))

                            def split():
                                for s, idx, pq, m, pws in parts:
                                    N.check(lib.vrq_scan_batch(*head, P(pq), m, K, 0, P(allow[s]), P(pws),
                                                               pws.numel(), st, eng), "d")

                            legs = {
                                "a_batch": lambda: N.check(lib.vrq_scan_batch(*head, P(qb), nq, K, 0, P(allow[0]), P(ws),
                                                                              need, st, eng), "a"),
                                "b_one_set": lambda: N.check(lib.vrq_scan_perquery(
                                    *head, P(qb), nq, K, 0, P(allow), P(ws), need, st, eng, S, allow.stride(0),
                                    P(zeros)), "b"),
                                "c_mixed": lambda: N.check(lib.vrq_scan_perquery(
                                    *head, P(qb), nq, K, 0, P(allow), P(ws), need, st, eng, S, allow.stride(0),
                                    P(qs)), "c"),
                                "d_split": split,
                            }
                            legs["c_mixed"]()
                            torch.cuda.synchronize()
                            tc, ls = lists_of(ws, info, nq, K)
                            split()
                            torch.cuda.synchronize()
                            same = True
                            for s, idx, pq, m, pws in parts:
                                ptc, pls = lists_of(pws, plan(lib, n, d, m, K, eng), m, K)
                                same = same and torch.equal(tc[idx], ptc) and torch.equal(ls[idx], pls)
                            if not same:
                                raise SystemExit(f"perquery != split at dim {d} nq {nq} {ename} S {S} {order}")
                            reps = {name: reps_for(call, a.warmup) for name, call in legs.items()}
                            times = {name: [] for name in legs}
                            for _ in range(a.rounds):             # alternate the legs round by round
                                for name, call in legs.items():
                                    times[name].append(window(call, reps[name]))
                            rec = {"dim": d, "n": n, "nq": nq, "K": K, "engine": ename, "sets": S, "order": order,
                                   "selectivity": sel, "rounds": a.rounds, "mixed_equals_split": same}
                            for name in legs:
                                rec[name] = summary(times[name])
                            aa = rec["a_batch"]
                            rec["a_spread"] = round((aa["max"] - aa["min"]) / aa["ms"], 3)
                            rec["b_over_a"] = round(rec["b_one_set"]["ms"] / aa["ms"], 3)
                            rec["c_over_a"] = round(rec["c_mixed"]["ms"] / aa["ms"], 3)
                            rec["c_over_d"] = round(rec["c_mixed"]["ms"] / rec["d_split"]["ms"], 3)
                            line = json.dumps(rec)
                            print(line, flush=True)
                            if out:
                                out.write(line + "\n")
                                out.flush()
                            del legs, parts
                del ws
            del allow
        del codes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
