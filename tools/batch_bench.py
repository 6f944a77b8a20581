#!/usr/bin/env python
"""The two engines of the counting scan side by side: K1h (``VRQ_LARGE_ENGINE_VALU``, the kernels of
``vrq_*_large`` / ``vrq_*_filtered``, unchanged) against K1hm (``VRQ_LARGE_ENGINE_MFMA``, the count and emit
stages on the matrix cores) -- HIP-event timing on the same device buffers in the same run, the two engines
alternating for ``--rounds`` rounds.

Per (n, dim, nq, K, allowed) with k = K / 10, K3 = 3 k, on preallocated buffers and per engine:

* ``scan``                          the whole ``vrq_scan_batch``;
* ``count`` / ``threshold`` / ``emit``   its stages, one call each, on a workspace a full scan has filled;
* ``search3``                       the whole ``vrq_search3_batch``.

``allowed`` 1.0 is the unfiltered call (no bitmap), below that a bitmap of random bits.  Before timing, the two
engines' (T, c_lt) pairs and K-lists after ``vrq_scan_batch`` and every output of ``vrq_search3_batch`` are
compared bit for bit.  One JSON line per shape; times in ms are the median over the rounds with the min and max
beside it.  ``mfma_faster`` is the criterion of the AUTO table: the MFMA engine's median scan time is below the
VALU engine's by more than the two legs' spread (max - min over the rounds) together.  Random codes and int8
rows; queries are corpus rows with d/16 .. d/4 flipped bits.

    python tools/batch_bench.py --out profiles/batch_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.search2_bench import summary, window  # noqa: E402
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd import filters  # noqa: E402
from vectorragquantization_amd import quant as Q  # noqa: E402
from vectorragquantization_amd import synth  # noqa: E402

STAGES = {"count": N.VRQ_LARGE_STAGE_COUNT, "threshold": N.VRQ_LARGE_STAGE_THRESHOLD,
          "emit": N.VRQ_LARGE_STAGE_EMIT}
ENGINES = {"valu": N.VRQ_LARGE_ENGINE_VALU, "mfma": N.VRQ_LARGE_ENGINE_MFMA}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1000000,10000000")
    ap.add_argument("--dims", default="384,1024,2048")
    ap.add_argument("--nqs", default="16,64,256,1024")
    ap.add_argument("--Ks", default="1024,8192")
    ap.add_argument("--allowed", default="1.0,0.1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=300.0, help="least length of a timed window")
    ap.add_argument("--min-reps", type=int, default=10, help="least calls per timed window")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = N.load()
    out = open(a.out, "a") if a.out else None
    P = N.ptr
    st = N.stream_handle(dev)
    gpu = torch.cuda.get_device_name(dev)

    def reps_for(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        once = window(call, 2)
        return max(a.min_reps, int(a.window_ms / max(once, 1e-3)) + 1)

    for n in (int(x) for x in a.ns.split(",")):
        for d in (int(x) for x in a.dims.split(",")):
            codes = synth.random_codes(n, d // 8, device=dev)
            x8 = torch.randint(-127, 128, (n, d), dtype=torch.int8, device=dev)
            norms = Q.int8_row_norms(x8)
            masks = {}
            for sel in (float(x) for x in a.allowed.split(",")):
                if sel < 1.0:
                    g = torch.Generator(device=dev)
                    g.manual_seed(int(sel * 1000) + 1)
                    masks[sel] = filters.row_bitmap(torch.rand((n,), generator=g, device=dev) < sel)
                else:
                    masks[sel] = None
            for nq in (int(x) for x in a.nqs.split(",")):
                qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
                qf = torch.randn((nq, d), device=dev) / d ** 0.5
                for K in (int(x) for x in a.Ks.split(",")):
                    k, K3 = K // 10, 3 * (K // 10)
                    need = lib.vrq_search3_batch_workspace_size(n, d, nq, K)
                    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
                    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
                    rows = torch.empty((nq, k), dtype=torch.int64, device=dev)
                    dd = torch.empty((nq, k), dtype=torch.int32, device=dev)
                    s2 = torch.empty((nq, k), dtype=torch.float64, device=dev)
                    s3 = torch.empty((nq, k), dtype=torch.float64, device=dev)
                    outs = (P(cnt), P(rows), P(dd), P(s2), P(s3))
                    three = (P(codes), P(x8), P(norms), 0, n, d, 0, P(qf), P(qb), nq, k, K, K3, 0)
                    scan = (P(codes), n, d, P(qb), nq, K)
                    tail = (P(ws), need, st)
                    for sel, allow in masks.items():
                        legs, plans = {}, {}
                        for ename, e in ENGINES.items():
                            info = torch.zeros(10, dtype=torch.int64)
                            N.check(lib.vrq_scan_batch_plan(n, d, nq, K, e, info.data_ptr()), "plan")
                            plans[ename] = [int(v) for v in info]
                            legs[f"{ename}_scan"] = lambda e=e: N.check(
                                lib.vrq_scan_batch(*scan, 0, P(allow), *tail, e), "scan")
                            for sname, bit in STAGES.items():
                                legs[f"{ename}_{sname}"] = lambda e=e, bit=bit: N.check(
                                    lib.vrq_scan_batch(*scan, bit, P(allow), *tail, e), "stage")
                            legs[f"{ename}_search3"] = lambda e=e: N.check(
                                lib.vrq_search3_batch(*three, P(allow), *outs, *tail, e), "search3")
                        # bit for bit before timing: (T, c_lt), the K-lists, every output of the search
                        got = {}
                        for ename in ENGINES:
                            p = plans[ename]
                            ws.fill_(0x5A)
                            legs[f"{ename}_scan"]()
                            torch.cuda.synchronize()
                            tc = ws[p[7]:p[7] + nq * 8].clone()
                            lists = ws[p[8]:p[8] + nq * K * 8].clone()
                            for t in (cnt, rows, dd, s2, s3):
                                t.zero_()
                            legs[f"{ename}_search3"]()
                            torch.cuda.synchronize()
                            got[ename] = [tc, lists] + [t.clone().view(torch.uint8) for t in (cnt, rows, dd, s2, s3)]
                        same = all(torch.equal(x, y) for x, y in zip(got["valu"], got["mfma"]))
                        del got
                        times = {name: [] for name in legs}
                        for ename in ENGINES:               # the stage legs run on a workspace a full scan has filled
                            legs[f"{ename}_scan"]()
                            reps = {name: reps_for(call) for name, call in legs.items() if name.startswith(ename)}
                            plans[ename + "_reps"] = reps
                        for _ in range(a.rounds):           # the engines alternate round by round
                            for ename in ENGINES:
                                legs[f"{ename}_scan"]()
                                for name, call in legs.items():
                                    if name.startswith(ename):
                                        times[name].append(window(call, plans[ename + "_reps"][name]))
                        rec = {"gpu": gpu, "n": n, "dim": d, "nq": nq, "K": K, "allowed": sel, "rounds": a.rounds,
                               "engines_equal": same,
                               "mfma_plan": dict(zip(("chunk_rows", "chunks", "queries_per_wave", "query_blocks",
                                                      "flush_rows"), plans["mfma"][1:6])),
                               "valu_chunks": plans["valu"][2]}
                        for name in legs:
                            rec[name] = summary(times[name])
                        v, m = rec["valu_scan"], rec["mfma_scan"]
                        rec["scan_valu_over_mfma"] = round(v["ms"] / m["ms"], 3)
                        rec["search3_valu_over_mfma"] = round(rec["valu_search3"]["ms"] / rec["mfma_search3"]["ms"], 3)
                        rec["mfma_faster"] = bool(v["ms"] - m["ms"] > (v["max"] - v["min"]) + (m["max"] - m["min"]))
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()
                        del legs
                    del ws
            del codes, x8, norms, masks
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
