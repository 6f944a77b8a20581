#!/usr/bin/env python
"""Search at embedding dims other than 1024: HIP-event timing of vrq_search3_dim per (dim, nq), full
three-phase (k = 10, K = 100, K3 = 30) and VRQ_SEARCH_PHASE1_ONLY, next to the yardstick -- the 1024-bit
wavefront scan (vrq_search3_dim at 1024, VRQ_SEARCH_SCAN_VALU | VRQ_SEARCH_PHASE1_ONLY) over a corpus of the same
byte count, run twice per point so that a difference can be judged against the yardstick's own spread.

One JSON line per point: ms, QPS and, for nq <= 8, the Phase-I corpus bytes per second as a share of the
8 TB/s HBM peak.  Random codes and int8 rows (the timing does not depend on their values); queries are
corpus rows with d/16 .. d/4 flipped bits.

    python tools/dim_bench.py --out profiles/dim_bench.jsonl

--exhaustive times K5d instead, the exact exhaustive top-k behind vrq_gemm_topk_dim / vrq_flat_ip_topk_dim
(VRQ_GEMM_SCAN_EXACT, so 1024 runs it too): per mode and dim, nq = 1, 8, 64, 1024 at k = 10 over a corpus
of a fixed byte count per mode (binary codes 256 MiB, int8 rows 1 GiB, float rows 2 GiB: with the int8
shadow of the 1024 matrix path the largest allocation stays under 3 GiB).  Each line carries ms, QPS, row
bytes per second as a share of the 8 TB/s HBM peak and the workspace bytes; at 1024 the forwarded matrix
path is timed on the same buffers in the same run.

    python tools/dim_bench.py --exhaustive --out profiles/exhaustive_dim_bench.jsonl

--ab times the two Phase-I scans of the other dims against each other on the same buffers in the same run
(vrq_search3_dim_scan + vrq_search3_dim_finish): the wavefront scan K1d forced by VRQ_SEARCH_SCAN_VALU --
the yardstick, timed twice per point, before and after the other leg -- and the matrix-core scan K1rd
forced by VRQ_SEARCH_SCAN_MFMA, Phase I only and full, plus "auto" (no forcing flag: the default choice).
Each matrix line carries the corpus re-read factor ceil(nq / (32 MB)) and the Phase-I rate
2 dim nq n / time in POPS and as a share of the 10.07 POPS FP4 dense peak.

    python tools/dim_bench.py --ab --nq 1,8,64,128,1024 --out profiles/dim_mfma_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd import synth  # noqa: E402
from vectorragquantization_amd.quant import int8_row_norms  # noqa: E402

HBM_PEAK = 8e12
K_OUT, K1, K3 = 10, 100, 30


def timed(call, warmup, reps):
    for _ in range(warmup):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def search_call(lib, codes, x8, norms, qf, qb, dim, flags, dev):
    n, nq = codes.shape[0], qb.shape[0]
    kout = K1 if flags & N.VRQ_SEARCH_PHASE1_ONLY else K_OUT
    ws = torch.empty((lib.vrq_search3_dim_workspace_size(n, dim, nq, K1),), dtype=torch.uint8, device=dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, kout), dtype=torch.int64, device=dev)
    dist = torch.empty((nq, kout), dtype=torch.int32, device=dev)
    s2 = torch.empty((nq, kout), dtype=torch.float64, device=dev)
    s3 = torch.empty((nq, kout), dtype=torch.float64, device=dev)
    st = N.stream_handle(dev)
    keep = (ws, cnt, rows, dist, s2, s3)

    def call():
        N.check(lib.vrq_search3_dim(N.ptr(codes), N.ptr(x8), N.ptr(norms), 0, n, dim, 0, N.ptr(qf), N.ptr(qb), nq,
                                    K_OUT, K1, K3, flags, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3),
                                    N.ptr(ws), ws.numel(), st), "vrq_search3_dim")
    return call, keep


def point(d, n, nq, mode, ms, cb):
    rec = {"dim": d, "n": n, "nq": nq, "mode": mode, "ms": round(ms, 4), "qps": round(nq / (ms * 1e-3), 1)}
    if nq <= 8 and mode != "full":
        bps = n * cb / (ms * 1e-3)
        rec["phase1_TBps"] = round(bps / 1e12, 3)
        rec["hbm_frac"] = round(bps / HBM_PEAK, 3)
    return rec


FP4_PEAK = 10.07e15


def pair_call(lib, codes, x8, norms, qf, qb, dim, flags, dev):
    """One search as the stage-able pair (the forcing flags go to both launches)."""
    n, nq = codes.shape[0], qb.shape[0]
    kout = K1 if flags & N.VRQ_SEARCH_PHASE1_ONLY else K_OUT
    ws = torch.empty((lib.vrq_search3_dim_workspace_size(n, dim, nq, K1),), dtype=torch.uint8, device=dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, kout), dtype=torch.int64, device=dev)
    dist = torch.empty((nq, kout), dtype=torch.int32, device=dev)
    s2 = torch.empty((nq, kout), dtype=torch.float64, device=dev)
    s3 = torch.empty((nq, kout), dtype=torch.float64, device=dev)
    st = N.stream_handle(dev)
    keep = (ws, cnt, rows, dist, s2, s3)

    def call():
        N.check(lib.vrq_search3_dim_scan(N.ptr(codes), n, dim, N.ptr(qb), nq, K1, flags, N.ptr(ws), ws.numel(), st),
                "vrq_search3_dim_scan")
        N.check(lib.vrq_search3_dim_finish(N.ptr(codes), N.ptr(x8), N.ptr(norms), 0, n, dim, 0, N.ptr(qf), nq, K_OUT,
                                           K1, K3, flags, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(s2), N.ptr(s3),
                                           N.ptr(ws), ws.numel(), st), "vrq_search3_dim_finish")
    return call, keep


def ab_leg(a, lib, dev, emit):
    import numpy as np
    P1 = N.VRQ_SEARCH_PHASE1_ONLY
    for d in (int(x) for x in a.dims.split(",")):
        cb, n = d // 8, a.n
        codes = synth.random_codes(n, cb, device=dev)
        x8 = torch.randint(-127, 127, (n, d), dtype=torch.int8, device=dev)
        norms = int8_row_norms(x8)
        for nq in (int(x) for x in a.nq.split(",")):
            qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
            qf = torch.randn((nq, d), device=dev) / d ** 0.5
            info = np.zeros(12, np.int64)
            N.check(lib.vrq_scan_plan(n, d, nq, K1, N.VRQ_SEARCH_SCAN_MFMA, info.ctypes.data), "vrq_scan_plan")
            mb = int(info[1])
            auto = "mfma" if lib.vrq_scan_kind(n, d, nq, K1, 0, None) == N.VRQ_SCAN_KIND_MFMA else "valu"
            for mode, mflags in (("phase1", P1), ("full", 0)):
                legs = (("valu", N.VRQ_SEARCH_SCAN_VALU, 0), ("mfma", N.VRQ_SEARCH_SCAN_MFMA, 0),
                        ("valu", N.VRQ_SEARCH_SCAN_VALU, 1), ("auto", 0, 0))
                for scan, sflags, rep in legs:
                    call, keep = pair_call(lib, codes, x8, norms, qf, qb, d, mflags | sflags, dev)
                    ms = timed(call, a.warmup, a.reps)
                    rec = {"dim": d, "n": n, "nq": nq, "mode": mode, "scan": scan, "repeat": rep, "ms": round(ms, 4),
                           "qps": round(nq / (ms * 1e-3), 1)}
                    if scan == "auto":
                        rec["auto_is"] = auto
                    if scan == "mfma":
                        rec.update({"mb": mb, "reread": -(-nq // (32 * mb)), "workspace_bytes": int(info[11])})
                        if mode == "phase1":
                            pops = 2.0 * d * nq * n / (ms * 1e-3)
                            rec.update({"phase1_pops": round(pops / 1e15, 4), "fp4_peak_frac": round(pops / FP4_PEAK, 4)})
                    emit(rec)
                    del call, keep
        del codes, x8, norms
        torch.cuda.empty_cache()


EX_BYTES = {"binary": 1 << 28, "int8_cosine": 1 << 30, "float_ip": 1 << 31}
EX_MODE = {"binary": N.VRQ_GEMM_BINARY, "int8_cosine": N.VRQ_GEMM_INT8_COSINE, "float_ip": N.VRQ_GEMM_FLOAT_IP}


def exhaustive_leg(a, lib, dev, emit):
    from vectorragquantization_amd.flat import flat_ip_prepare
    st = N.stream_handle(dev)
    for mode in a.modes.split(","):
        m = EX_MODE[mode]
        for d in (int(x) for x in a.dims.split(",")):
            rb = d // 8 if mode == "binary" else d if mode == "int8_cosine" else 4 * d
            n = EX_BYTES[mode] // rb
            codes = x8 = norms = xf = inv = bounds = None
            if mode == "binary":
                codes = synth.random_codes(n, rb, device=dev)
            elif mode == "int8_cosine":
                x8 = torch.randint(-127, 127, (n, d), dtype=torch.int8, device=dev)
                norms = int8_row_norms(x8)
            else:
                xf = torch.randn((n, d), device=dev) / d ** 0.5
                if d == 1024:
                    bounds = torch.zeros((2,), dtype=torch.float64, device=dev)
                    x8, inv = flat_ip_prepare(xf, bounds)
            for nq in (int(x) for x in a.nq.split(",")):
                qf = torch.randn((nq, d), device=dev) / d ** 0.5
                cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
                rows = torch.empty((nq, K_OUT), dtype=torch.int64, device=dev)
                sc = torch.empty((nq, K_OUT), dtype=torch.float64, device=dev)
                legs = [("k5d", N.VRQ_GEMM_SCAN_EXACT)] + ([("matrix", 0)] if d == 1024 else [])
                for leg, flags in legs:
                    need = N.gemm_topk_dim_workspace(lib, m, n, d, nq, K_OUT, flags)
                    ws = torch.empty((need,), dtype=torch.uint8, device=dev)

                    def call():
                        if mode == "float_ip":
                            rc = lib.vrq_flat_ip_topk_dim(N.ptr(xf), N.ptr(x8), N.ptr(inv), N.ptr(bounds), n, d, 0,
                                                          N.ptr(qf), nq, K_OUT, flags, N.ptr(cnt), N.ptr(rows),
                                                          N.ptr(sc), N.ptr(ws), need, st)
                        else:
                            rc = lib.vrq_gemm_topk_dim(m, N.ptr(codes), N.ptr(x8), N.ptr(norms), n, d, 0, N.ptr(qf), nq,
                                                       K_OUT, flags, N.ptr(cnt), N.ptr(rows), N.ptr(sc), N.ptr(ws),
                                                       need, st)
                        N.check(rc, "exhaustive top-k")
                    ms = timed(call, a.warmup, a.reps)
                    bps = n * rb / (ms * 1e-3)
                    emit({"kernel": leg, "mode": mode, "dim": d, "n": n, "row_bytes": rb, "nq": nq, "k": K_OUT,
                          "ms": round(ms, 4), "qps": round(nq / (ms * 1e-3), 1), "row_TBps": round(bps / 1e12, 4),
                          "hbm_frac": round(bps / HBM_PEAK, 4), "workspace_bytes": int(need)})
                    del ws
            del codes, x8, norms, xf, inv, bounds
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="256,384,512,768,1536,2048")
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", default="1,8,64,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--exhaustive", action="store_true",
                    help="time K5d (exact exhaustive top-k) per mode and dim, 1024 included, instead of the search")
    ap.add_argument("--ab", action="store_true",
                    help="time the forced wavefront scan (twice) and the forced matrix-core scan on the same buffers")
    ap.add_argument("--modes", default="binary,int8_cosine,float_ip", help="--exhaustive: modes to time")
    a = ap.parse_args()
    if a.exhaustive and a.dims == ap.get_default("dims"):
        a.dims = "256,384,512,768,1024,1536,2048"
    dev = torch.device("cuda", 0)
    lib = N.load()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if a.exhaustive:
        exhaustive_leg(a, lib, dev, emit)
        return
    if a.ab:
        ab_leg(a, lib, dev, emit)
        return
    P1 = N.VRQ_SEARCH_PHASE1_ONLY
    for d in (int(x) for x in a.dims.split(",")):
        cb, n = d // 8, a.n
        codes = synth.random_codes(n, cb, device=dev)
        x8 = torch.randint(-127, 127, (n, d), dtype=torch.int8, device=dev)
        norms = int8_row_norms(x8)
        ny = n * cb // 128                                   # the yardstick corpus: same bytes, 128-byte codes
        ycodes = synth.random_codes(ny, 128, device=dev, seed=synth.SEED + 7)
        for nq in (int(x) for x in a.nq.split(",")):
            qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
            qf = torch.randn((nq, d), device=dev) / d ** 0.5
            yqb, _ = synth.flip_queries(ycodes, nq)
            for mode, flags in (("phase1", P1), ("full", 0)):
                call, keep = search_call(lib, codes, x8, norms, qf, qb, d, flags, dev)
                emit(point(d, n, nq, mode, timed(call, a.warmup, a.reps), cb))
                del call, keep
            for rep in (0, 1):
                call, keep = search_call(lib, ycodes, None, None, None, yqb, 1024, P1 | N.VRQ_SEARCH_SCAN_VALU, dev)
                rec = point(1024, ny, nq, "yardstick_valu_phase1", timed(call, a.warmup, a.reps), 128)
                rec.update({"for_dim": d, "repeat": rep})
                emit(rec)
                del call, keep
        del codes, x8, norms, ycodes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
