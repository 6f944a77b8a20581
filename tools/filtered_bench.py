#!/usr/bin/env python
"""The filtered search (``vrq_search3_filtered``: a row allow-bitmap through the counting scan K1h) beside the
unfiltered call and beside what a caller without it does -- copy the allowed rows into a compact corpus and
search that: HIP-event timing on the same device buffers in the same run, the legs alternating for
``--rounds`` rounds.

Per (dim, nq) at 1M rows, K = 1024, k = K / 10, K3 = 3 k, and per filter (selectivity 1.0, 0.5, 0.1, 0.01, each
as random bits and as one contiguous range of rows), on preallocated buffers:

* ``a_large``       the unfiltered ``vrq_search3_large``: the yardstick;
* ``b_filtered``    ``vrq_search3_filtered``, and its stages through ``vrq_scan_filtered``: ``count``,
  ``threshold``, ``emit``;
* ``c_gather``      today's route: ``torch.index_select`` of the allowed codes, int8 rows and norms into a
  compact corpus (timed), then ``vrq_search3_large`` on it; ``c_gather_only`` is the copy alone.

Before timing, (b) is compared with (c) mapped back to the original rows, bit for bit.  One JSON line per
(dim, nq, filter); times in ms are the median over the rounds with the min and max beside it; ``b_over_a`` and
``b_over_c`` are ratios of the medians.  Random codes and int8 rows; queries are corpus rows with d/16 .. d/4
flipped bits.

    python tools/filtered_bench.py --out profiles/filtered_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import search2_bench  # noqa: E402
from tools.search2_bench import reps_for, summary, window  # noqa: E402
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd import filters  # noqa: E402
from vectorragquantization_amd import quant as Q  # noqa: E402
from vectorragquantization_amd import synth  # noqa: E402

STAGES = {"count": N.VRQ_LARGE_STAGE_COUNT, "threshold": N.VRQ_LARGE_STAGE_THRESHOLD,
          "emit": N.VRQ_LARGE_STAGE_EMIT}


def make_mask(n, sel, kind, dev):
    if kind == "random":
        g = torch.Generator(device=dev)
        g.manual_seed(int(sel * 1000) + 1)
        return torch.rand((n,), generator=g, device=dev) < sel if sel < 1.0 else torch.ones(n, dtype=torch.bool, device=dev)
    m = int(round(n * sel))
    lo = (n - m) // 2 // 64 * 64 + (37 if m < n else 0)          # a range that starts and ends inside a tile
    r = torch.arange(n, device=dev)
    return (r >= lo) & (r < lo + m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="1024,384")
    ap.add_argument("--nqs", default="1,64")
    ap.add_argument("--K", type=int, default=1024)
    ap.add_argument("--sels", default="1.0,0.5,0.1,0.01")
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
    k, K3 = K // 10, 3 * (K // 10)
    P = N.ptr
    st = N.stream_handle(dev)
    for d in (int(x) for x in a.dims.split(",")):
        codes = synth.random_codes(n, d // 8, device=dev)
        x8 = torch.randint(-127, 128, (n, d), dtype=torch.int8, device=dev)
        norms = Q.int8_row_norms(x8)
        gcodes, gx8, gnorms = torch.empty_like(codes), torch.empty_like(x8), torch.empty_like(norms)
        for nq in (int(x) for x in a.nqs.split(",")):
            qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
            qf = torch.randn((nq, d), device=dev) / d ** 0.5
            need = lib.vrq_search3_large_workspace_size(n, d, nq, K)
            assert need == lib.vrq_search3_filtered_workspace_size(n, d, nq, K)
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)
            cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
            rows = torch.empty((nq, k), dtype=torch.int64, device=dev)
            dd = torch.empty((nq, k), dtype=torch.int32, device=dev)
            s2 = torch.empty((nq, k), dtype=torch.float64, device=dev)
            s3 = torch.empty((nq, k), dtype=torch.float64, device=dev)
            outs = (P(cnt), P(rows), P(dd), P(s2), P(s3))
            three = (P(codes), P(x8), P(norms), 0, n, d, 0, P(qf), P(qb), nq, k, K, K3, 0)
            tail = (P(ws), need, st)

            def results(call):
                for t in (cnt, rows, dd, s2, s3):
                    t.zero_()
                call()
                torch.cuda.synchronize()
                return [t.clone() for t in (cnt, rows, dd, s2, s3)]

            for sel in (float(x) for x in a.sels.split(",")):
                for kind in ("random", "range"):
                    mask = make_mask(n, sel, kind, dev)
                    allow = filters.row_bitmap(mask)
                    keep = torch.nonzero(mask).reshape(-1)
                    m = int(keep.shape[0])
                    gneed = lib.vrq_search3_large_workspace_size(m, d, nq, K)
                    gws = torch.empty((gneed,), dtype=torch.uint8, device=dev)
                    scan = (P(codes), n, d, P(qb), nq, K)

                    def gather():
                        torch.index_select(codes, 0, keep, out=gcodes[:m])
                        torch.index_select(x8, 0, keep, out=gx8[:m])
                        torch.index_select(norms, 0, keep, out=gnorms[:m])

                    def compact():
                        gather()
                        N.check(lib.vrq_search3_large(P(gcodes), P(gx8), P(gnorms), 0, m, d, 0, P(qf), P(qb), nq, k,
                                                      K, K3, 0, *outs, P(gws), gneed, st), "c")

                    legs = {
                        "a_large": lambda: N.check(lib.vrq_search3_large(*three, *outs, *tail), "a"),
                        "b_filtered": lambda: N.check(lib.vrq_search3_filtered(*three, P(allow), *outs, *tail), "b"),
                        "b_scan": lambda: N.check(lib.vrq_scan_filtered(*scan, 0, P(allow), *tail), "b_scan"),
                    }
                    for name, bit in STAGES.items():
                        legs[f"b_{name}"] = lambda bit=bit: N.check(
                            lib.vrq_scan_filtered(*scan, bit, P(allow), *tail), "stage")
                    legs["c_gather"] = compact
                    legs["c_gather_only"] = gather
                    got = results(legs["b_filtered"])
                    want = results(compact)
                    want[1] = torch.where(want[1] >= 0, keep[want[1].clamp_min(0)], want[1])
                    same = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                                           y.view(torch.int64) if y.dtype == torch.float64 else y)
                               for x, y in zip(got, want))
                    # the stage legs run on a workspace a full scan has filled (scan, count, threshold, emit)
                    for name, call in legs.items():
                        call()
                    reps = {name: reps_for(call, a.warmup) for name, call in legs.items()}
                    times = {name: [] for name in legs}
                    for _ in range(a.rounds):                     # alternate the legs round by round
                        for name, call in legs.items():
                            times[name].append(window(call, reps[name]))
                    rec = {"dim": d, "n": n, "nq": nq, "K": K, "selectivity": sel, "filter": kind, "allowed": m,
                           "rounds": a.rounds, "filtered_equals_gathered": same}
                    for name in legs:
                        rec[name] = summary(times[name])
                    rec["b_finish_ms"] = round(rec["b_filtered"]["ms"] - rec["b_scan"]["ms"], 4)
                    rec["b_over_a"] = round(rec["b_filtered"]["ms"] / rec["a_large"]["ms"], 3)
                    rec["b_over_c"] = round(rec["b_filtered"]["ms"] / rec["c_gather"]["ms"], 3)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
                    del legs, gws
            del ws
        del codes, x8, norms, gcodes, gx8, gnorms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
