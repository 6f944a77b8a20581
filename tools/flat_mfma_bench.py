"""K5mf against K5d: the exact float inner-product top-k on the matrix cores (vrq_flat_ip_topk_dim_mfma) and the
exact f64 scan (vrq_flat_ip_topk_dim) on the same rows, in the same process.

Shapes: the row counts of the K5md table (tools/exhaustive_mfma_bench.py: 1 GiB of int8 rows per dim, so 4 GiB of
float rows), unit-norm Gaussian rows from a fixed seed per dim, nq = 1, 8, 64, 1024, k = 10, HIP events, 3 warm-ups
+ 20 timed calls, one event pair per call: each point carries the median, the minimum and the maximum of both
engines.  `wins` is true where K5mf's slowest call beat K5d's fastest -- the rule vrq_flat_ip_dim_engine's table
is filled by.  The run fails if counts, rows or score bits of the two engines differ at any point.  The stage
times (VRQ_GEMM_STAGE_SAMPLE / _MAIN / _FINISH) are medians of the same number of calls; `finish_share` is the
finish stage over the sum of the three.

    python tools/flat_mfma_bench.py --out profiles/flat_mfma_bench.jsonl
    python tools/flat_mfma_bench.py --lib build/libvrq_r1.so --nq 1024 --out profiles/flat_mfma_bench_r1.jsonl
(the second: a library built with -DVRQ_G5F_R=1, the one-row-per-round finish, on the same seeded rows and so the
same candidates; compare `stage_ms.finish`).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vectorragquantization_amd import _native as N  # noqa: E402

ROW_BYTES = 1 << 30  # of the int8 image; the float rows are four times that
K_OUT = 10


def timed_each(call, warmup, reps):
    for _ in range(warmup):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        call()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def stats(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def unit_rows(n, d, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    xf = torch.empty((n, d), dtype=torch.float32, device=dev)
    step = (1 << 28) // d
    for a in range(0, n, step):
        blk = torch.randn((min(step, n - a), d), generator=g, device=dev)
        xf[a:a + blk.shape[0]] = blk / blk.norm(dim=1, keepdim=True)
    return xf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="256,384,512,768,1536,2048")
    ap.add_argument("--nq", default="1,8,64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--row-bytes", type=int, default=ROW_BYTES, help="bytes of int8 rows per dim")
    ap.add_argument("--lib", default=None, help="another build of the library (the R = 1 A/B)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.lib:
        N.use_library(a.lib)
    from vectorragquantization_amd.flat import flat_ip_prepare
    dev = torch.device("cuda", 0)
    lib, st = N.load(), N.stream_handle(dev)
    ok = True
    for d in (int(x) for x in a.dims.split(",")):
        n = a.row_bytes // d
        xf = unit_rows(n, d, dev, 1000 + d)
        bounds = torch.zeros((2,), dtype=torch.float64, device=dev)
        x8, inv = flat_ip_prepare(xf, bounds)
        prep = timed_each(lambda: flat_ip_prepare(xf, bounds), 1, 5)
        for nq in (int(x) for x in a.nq.split(",")):
            g = torch.Generator(device=dev).manual_seed(2000 + d + nq)
            qf = torch.randn((nq, d), generator=g, device=dev) / d ** 0.5
            cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
            rows = torch.empty((nq, K_OUT), dtype=torch.int64, device=dev)
            sc = torch.empty((nq, K_OUT), dtype=torch.float64, device=dev)
            need = max(N.gemm_topk_dim_workspace(lib, N.VRQ_GEMM_FLOAT_IP, n, d, nq, K_OUT),
                       lib.vrq_flat_ip_topk_dim_mfma_workspace_size(n, d, nq, K_OUT))
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)

            def call(fn, flags):
                N.check(fn(N.ptr(xf), N.ptr(x8), N.ptr(inv), N.ptr(bounds), n, d, 0, N.ptr(qf), nq, K_OUT, flags,
                           N.ptr(cnt), N.ptr(rows), N.ptr(sc), N.ptr(ws), need, st), "flat top-k")

            k5d = timed_each(lambda: call(lib.vrq_flat_ip_topk_dim, 0), a.warmup, a.reps)
            ref = (cnt.clone(), rows.clone(), sc.clone())
            k5mf = timed_each(lambda: call(lib.vrq_flat_ip_topk_dim_mfma, N.VRQ_GEMM_NO_FALLBACK), a.warmup, a.reps)
            same = (torch.equal(ref[0], cnt) and torch.equal(ref[1], rows)
                    and torch.equal(ref[2].view(torch.int64), sc.view(torch.int64)))
            ok = ok and same
            stage = {}
            for name, fl in (("sample", N.VRQ_GEMM_STAGE_SAMPLE), ("main", N.VRQ_GEMM_STAGE_MAIN),
                             ("finish", N.VRQ_GEMM_STAGE_FINISH)):
                # (a stage leaves the workspace as the next one expects it; repeated, it finds its own inputs)
                stage[name] = round(statistics.median(timed_each(
                    lambda: call(lib.vrq_flat_ip_topk_dim_mfma, fl | N.VRQ_GEMM_NO_FALLBACK), 1, a.reps)), 4)
            rec = {"bench": "flat_mfma", "dim": d, "n": n, "nq": nq, "k": K_OUT, "k5d": stats(k5d),
                   "k5mf": stats(k5mf), "ratio": round(statistics.median(k5d) / statistics.median(k5mf), 2),
                   "wins": max(k5mf) < min(k5d), "same_result": same, "stage_ms": stage,
                   "finish_share": round(stage["finish"] / sum(stage.values()), 3),
                   "prepare_ms": round(statistics.median(prep), 4),
                   "prepare_gbps": round((5 * d + 8) * n / (statistics.median(prep) * 1e-3) / 1e9, 1),
                   "workspace_bytes": int(need), "lib": os.path.basename(N.lib_path())}
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del ws
        del xf, x8, inv
        torch.cuda.empty_cache()
    if not ok:
        sys.exit("flat_mfma_bench: K5mf and K5d returned different counts, rows or score bits")


if __name__ == "__main__":
    main()
