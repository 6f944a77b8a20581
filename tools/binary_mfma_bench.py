"""K5mb against K5d: exhaustive binary (Phase-II) top-k on the matrix cores (vrq_binary_topk_dim_mfma) and the
exact f64 scan (vrq_gemm_topk_dim, VRQ_GEMM_BINARY) on the same codes, in the same process.

Shapes: the row counts of the K5md table (tools/exhaustive_mfma_bench.py: 2^30 / d rows per dim), random
codes of d / 8 bytes, nq = 1, 8, 64, 1024, k = 10, HIP events, 3 warm-ups + 20 timed calls.  The queries are
Gaussian values rounded to the 2^-20 grid, so every +-q sum is exact in float64 in any order and the two
engines, which add in different orders, must return identical counts, rows and score bits: the tool asserts
it at every point.  Every timed call has its own event pair, so each point carries the median, the minimum
and the maximum of the 20 calls of both engines; `wins` is true where K5mb's slowest call beat K5d's
fastest, which is the rule the library's auto table (vrq_binary_topk_dim_engine) is filled by.  The stage
times (VRQ_GEMM_STAGE_SAMPLE / _MAIN / _FINISH) are medians of the same number of calls; `cand_per_query` is
the mean list length sum per query after the main pass; `main_i8_frac` is 2 nq n d / main-pass time as a
share of the 2.4-GHz i8 dense peak.

    python tools/binary_mfma_bench.py --out profiles/binary_mfma_bench.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.exhaustive_mfma_bench import I8_DENSE_PEAK, K_OUT, ROW_BYTES, stats, timed_each  # noqa: E402
from vectorragquantization_amd import _native as N  # noqa: E402

MODE = N.VRQ_GEMM_BINARY


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
        codes = torch.randint(0, 256, (n, d // 8), dtype=torch.uint8, device=dev)
        for nq in (int(x) for x in a.nq.split(",")):
            qf = (torch.round(torch.randn((nq, d), device=dev) * 2.0 ** 20) / 2.0 ** 20).clamp(-7.0, 7.0)
            cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
            rows = torch.empty((nq, K_OUT), dtype=torch.int64, device=dev)
            sc = torch.empty((nq, K_OUT), dtype=torch.float64, device=dev)
            need = max(N.gemm_topk_dim_workspace(lib, MODE, n, d, nq, K_OUT),
                       N.binary_topk_dim_mfma_workspace(lib, n, d, nq, K_OUT))
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)
            plan, lay = (C.c_int64 * 8)(), (C.c_int64 * 8)()
            N.check(lib.vrq_binary_topk_dim_mfma_plan(n, d, nq, K_OUT, plan), "plan")
            N.check(lib.vrq_binary_topk_dim_mfma_prep_layout(n, d, nq, K_OUT, lay), "layout")

            def k5d():
                N.check(lib.vrq_gemm_topk_dim(MODE, N.ptr(codes), None, None, n, d, 0, N.ptr(qf), nq, K_OUT, 0,
                                              N.ptr(cnt), N.ptr(rows), N.ptr(sc), N.ptr(ws), need, st), "K5d")

            def k5mb(flags=0):
                N.check(lib.vrq_binary_topk_dim_mfma(N.ptr(codes), n, d, 0, N.ptr(qf), nq, K_OUT,
                                                     flags | N.VRQ_GEMM_NO_FALLBACK, N.ptr(cnt), N.ptr(rows),
                                                     N.ptr(sc), N.ptr(ws), need, st), "K5mb")

            t_d = timed_each(k5d, a.warmup, a.reps)
            ref = (cnt.clone(), rows.clone(), sc.clone())
            t_mb = timed_each(k5mb, a.warmup, a.reps)
            assert all(torch.equal(x, y) for x, y in zip(ref, (cnt, rows, sc))), (d, nq, "K5mb differs from K5d")
            stage = {}
            for name, fl in (("sample", N.VRQ_GEMM_STAGE_SAMPLE), ("main", N.VRQ_GEMM_STAGE_MAIN),
                             ("finish", N.VRQ_GEMM_STAGE_FINISH)):
                # (a stage leaves the workspace as the next one expects it; repeated, it finds its own inputs)
                stage[name] = round(statistics.median(timed_each(lambda: k5mb(fl), 1, a.reps)), 4)
            k5mb(N.VRQ_GEMM_STAGE_SAMPLE | N.VRQ_GEMM_STAGE_MAIN)
            torch.cuda.synchronize()
            lens = ws[lay[6]:lay[6] + 4 * nq * plan[1]].view(torch.int32).view(nq, plan[1])
            rec = {"bench": "binary_mfma", "dim": d, "n": n, "nq": nq, "k": K_OUT, "k5d": stats(t_d),
                   "k5mb": stats(t_mb), "ratio": round(statistics.median(t_d) / statistics.median(t_mb), 2),
                   "wins": max(t_mb) < min(t_d), "same_result": True, "stage_ms": stage,
                   "cand_per_query": round(float(lens.sum(dim=1).float().mean()), 1),
                   "overflowed_lists": int((lens > plan[2]).sum()),
                   "main_i8_frac": round(2.0 * nq * n * d / (stage["main"] * 1e-3) / I8_DENSE_PEAK, 4),
                   "workspace_bytes": int(need)}
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del ws
        del codes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
