"""K5md against K5d: exhaustive int8-cosine top-k on the matrix cores (vrq_gemm_topk_dim_mfma) and the exact
f64 scan (vrq_gemm_topk_dim) on the same rows, in the same call.

Shapes: the int8-cosine rows of the K5d table (tools/dim_bench.py --exhaustive): 1 GiB of int8 rows per dim,
nq = 1, 8, 64, 1024, k = 10, HIP events, 3 warm-ups + 20 timed calls.  Every timed call has its own event pair,
so each point carries the median, the minimum and the maximum of the 20 calls of both engines; `wins` is true
where K5md's slowest call beat K5d's fastest, which is the rule the library's auto table
(vrq_gemm_topk_dim_engine) is filled by.  The stage times (VRQ_GEMM_STAGE_SAMPLE / _MAIN / _FINISH) are
medians of the same number of calls; `main_i8_frac` is 2 nq n d / main-pass time as a share of the 2.4-GHz i8
dense peak (K5 at d = 1024 reaches 0.47-0.48).

    python tools/exhaustive_mfma_bench.py --out profiles/exhaustive_mfma_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd.quant import int8_row_norms  # noqa: E402

I8_DENSE_PEAK = 1024 * 2048 * 2.4e9  # ops/s: 1024 SIMDs x 2048 i8 ops/clk x 2.4 GHz
ROW_BYTES = 1 << 30
K_OUT = 10
MODE = N.VRQ_GEMM_INT8_COSINE


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="256,384,512,768,1536,2048")
    ap.add_argument("--nq", default="1,8,64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib, st = N.load(), N.stream_handle(dev)
    for d in (int(x) for x in a.dims.split(",")):
        n = ROW_BYTES // d
        x8 = torch.randint(-127, 127, (n, d), dtype=torch.int8, device=dev)
        norms = int8_row_norms(x8)
        for nq in (int(x) for x in a.nq.split(",")):
            qf = torch.randn((nq, d), device=dev) / d ** 0.5
            cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
            rows = torch.empty((nq, K_OUT), dtype=torch.int64, device=dev)
            sc = torch.empty((nq, K_OUT), dtype=torch.float64, device=dev)
            need = max(N.gemm_topk_dim_workspace(lib, MODE, n, d, nq, K_OUT),
                       N.gemm_topk_dim_mfma_workspace(lib, MODE, n, d, nq, K_OUT))
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)

            def call(fn, flags):
                N.check(fn(MODE, None, N.ptr(x8), N.ptr(norms), n, d, 0, N.ptr(qf), nq, K_OUT, flags, N.ptr(cnt),
                           N.ptr(rows), N.ptr(sc), N.ptr(ws), need, st), "exhaustive top-k")

            k5d = timed_each(lambda: call(lib.vrq_gemm_topk_dim, 0), a.warmup, a.reps)
            ref = (cnt.clone(), rows.clone(), sc.clone())
            k5md = timed_each(lambda: call(lib.vrq_gemm_topk_dim_mfma, N.VRQ_GEMM_NO_FALLBACK), a.warmup, a.reps)
            same = all(torch.equal(x, y) for x, y in zip(ref, (cnt, rows, sc)))
            stage = {}
            for name, fl in (("sample", N.VRQ_GEMM_STAGE_SAMPLE), ("main", N.VRQ_GEMM_STAGE_MAIN),
                             ("finish", N.VRQ_GEMM_STAGE_FINISH)):
                # (a stage leaves the workspace as the next one expects it; repeated, it finds its own inputs)
                stage[name] = round(statistics.median(timed_each(
                    lambda: call(lib.vrq_gemm_topk_dim_mfma, fl | N.VRQ_GEMM_NO_FALLBACK), 1, a.reps)), 4)
            rec = {"bench": "exhaustive_mfma", "dim": d, "n": n, "nq": nq, "k": K_OUT, "k5d": stats(k5d),
                   "k5md": stats(k5md), "ratio": round(statistics.median(k5d) / statistics.median(k5md), 2),
                   "wins": max(k5md) < min(k5d), "same_result": same, "stage_ms": stage,
                   "main_i8_frac": round(2.0 * nq * n * d / (stage["main"] * 1e-3) / I8_DENSE_PEAK, 4),
                   "workspace_bytes": int(need)}
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del ws
        del x8, norms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
