#!/usr/bin/env python
"""The fused two-phase search against the composed path it can replace: HIP-event timing of
``quant.search2`` (one ``vrq_search2`` call) and ``quant.vectordb_search`` (``vrq_hamming_topk``, a gather,
``vrq_rescore_dequant``, a ``torch.sort`` and three more gathers) on the same device buffers in the same
run, alternating the two for ``--rounds`` rounds so that a difference can be judged against each leg's
own spread.  Both are timed as a caller sees them, output and workspace allocation included.

Points (k = 10, binary_oversample = 10, so K = 100): 1M x 1024 at nq = 1 and 1024, 1M x 384 at nq = 1024,
each for mode ``sbin`` (the packed codes rescored as +-1 rows) and ``int8g``.  Before timing, the two
paths' outputs are compared bit for bit at the timed size.  Every point also carries the stage split of
the fused call on preallocated buffers: the scan (``vrq_search3_dim_scan``) and the finish
(``vrq_search2_finish``) timed separately, and the two back to back (``vrq_search2``).

One JSON line per point; times in ms are the median over the rounds with the min and max beside it.
Random codes and rows (the timing does not depend on their values); queries are corpus rows with
d/16 .. d/4 flipped bits.

    python tools/search2_bench.py --out profiles/search2_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vectorragquantization_amd import _native as N  # noqa: E402
from vectorragquantization_amd import quant as Q  # noqa: E402
from vectorragquantization_amd import synth  # noqa: E402

K_OUT, OVERSAMPLE = 10, 10
LIMIT = 0.3
POINTS = ((1024, 1), (1024, 1024), (384, 1024))
MIN_WINDOW_MS = 300.0


def window(call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(call, warmup):
    """Warm the shape up, then size the timed window to at least MIN_WINDOW_MS."""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    once = window(call, 5)
    return max(10, int(MIN_WINDOW_MS / max(once, 1e-3)) + 1)


def summary(xs):
    return {"ms": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def raw_calls(lib, mode, codes, q, qf, qb, dev):
    """(scan, finish, fused) closures on preallocated buffers."""
    n, nq, d = codes.shape[0], qb.shape[0], qf.shape[1]
    K = min(K_OUT * OVERSAMPLE, n)
    need = lib.vrq_search2_workspace_size(n, d, nq, K)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, K_OUT), dtype=torch.int64, device=dev)
    dist = torch.empty((nq, K_OUT), dtype=torch.int32, device=dev)
    sc = torch.empty((nq, K_OUT), dtype=torch.float64, device=dev)
    st = N.stream_handle(dev)
    m = Q._SEARCH2_MODES[mode]

    def scan():
        N.check(lib.vrq_search3_dim_scan(N.ptr(codes), n, d, N.ptr(qb), nq, K, 0, N.ptr(ws), need, st), "scan")

    def finish():
        N.check(lib.vrq_search2_finish(m, N.ptr(codes), N.ptr(q), 0, LIMIT, 0, n, d, 0, N.ptr(qf), nq, K_OUT, K, 0,
                                       N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(sc), N.ptr(ws), need, st), "finish")

    def fused():
        N.check(lib.vrq_search2(m, N.ptr(codes), N.ptr(q), 0, LIMIT, 0, n, d, 0, N.ptr(qf), N.ptr(qb), nq, K_OUT, K, 0,
                                N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(sc), N.ptr(ws), need, st), "vrq_search2")
    return scan, finish, fused, (ws, cnt, rows, dist, sc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--modes", default="sbin,int8g")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = N.load()
    out = open(a.out, "a") if a.out else None
    n = a.n
    for d, nq in POINTS:
        codes = synth.random_codes(n, d // 8, device=dev)
        qb, _ = synth.flip_queries(codes, nq, flips=(d // 16, d // 4))
        qf = torch.randn((nq, d), device=dev) / d ** 0.5
        for mode in a.modes.split(","):
            q = codes if mode == "sbin" else torch.randint(-127, 128, (n, d), dtype=torch.int8, device=dev)
            vmode = mode

            def composed():
                if vmode == "sbin":   # vectordb_search has no name for the mode: the same five steps by hand
                    return composed_sbin(lib, codes, qf, qb, dev)
                return Q.vectordb_search(vmode, codes, q, qf, qb, K_OUT, OVERSAMPLE, None, LIMIT)

            def fused():
                return Q.search2(vmode, codes, q, qf, qb, K_OUT, OVERSAMPLE, None, LIMIT)

            same = all(torch.equal(x, y) for x, y in zip(composed(), fused()))
            scan, finish, raw, keep = raw_calls(lib, mode, codes, q, qf, qb, dev)
            legs = {"composed": composed, "fused": fused, "scan": scan, "finish": finish, "fused_raw": raw}
            reps = {name: reps_for(call, a.warmup) for name, call in legs.items()}
            times = {name: [] for name in legs}
            for _ in range(a.rounds):                     # alternate the legs round by round
                for name, call in legs.items():
                    times[name].append(window(call, reps[name]))
            kind = "mfma" if lib.vrq_scan_kind(n, d, nq, min(K_OUT * OVERSAMPLE, n), 0, None) == N.VRQ_SCAN_KIND_MFMA \
                else "valu"
            rec = {"dim": d, "n": n, "nq": nq, "mode": mode, "k": K_OUT, "K": min(K_OUT * OVERSAMPLE, n), "scan_kind": kind,
                   "outputs_equal": bool(same), "rounds": a.rounds, "reps": reps}
            for name in legs:
                rec[name] = summary(times[name])
            rec["fused_over_composed"] = round(rec["fused"]["ms"] / rec["composed"]["ms"], 4)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del q, keep, scan, finish, raw, legs
        del codes
        torch.cuda.empty_cache()


def composed_sbin(lib, codes, qf, qb, dev):
    """``quant.vectordb_search`` step for step with the rescoring mode VRQ_RESCORE_SIGNED_BINARY."""
    n, cb = codes.shape
    nq, d = qf.shape
    K = min(K_OUT * OVERSAMPLE, n)
    dist = torch.empty((nq, K), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, K), dtype=torch.int64, device=dev)
    ws = torch.empty((max(8, lib.vrq_hamming_topk_workspace_size(n, cb, nq, K)),), dtype=torch.uint8, device=dev)
    st = N.stream_handle(dev)
    N.check(lib.vrq_hamming_topk(N.ptr(codes), n, cb, 0, N.ptr(qb), nq, K, N.ptr(dist), N.ptr(rows), N.ptr(ws),
                                 ws.numel(), st), "vrq_hamming_topk")
    score = torch.empty((nq, K), dtype=torch.float64, device=dev)
    N.check(lib.vrq_rescore_dequant(N.VRQ_RESCORE_SIGNED_BINARY, N.ptr(qf), nq, d, N.ptr(codes), 0, 0.0, n,
                                    N.ptr(rows), K, N.ptr(score), st), "vrq_rescore_dequant")
    key = torch.where(rows >= 0, score + 0.0, torch.full_like(score, float("-inf")))
    o = torch.sort(-key, dim=1, stable=True).indices[:, :K_OUT]
    return torch.gather(rows, 1, o), torch.gather(dist, 1, o), torch.gather(score, 1, o)


if __name__ == "__main__":
    main()
