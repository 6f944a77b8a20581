#!/usr/bin/env python
"""The filtered exhaustive top-k over a row list (K5g: ``vrq_flat_ip_topk_rows`` / ``vrq_gemm_topk_rows``; K5gb, mode
``binary``: ``vrq_binary_topk_gather``) beside
the unfiltered matrix call on all rows and beside what a caller without it does -- ``index_select`` the allowed
rows into a copy, prepare the copy, search it: HIP-event timing on the same device buffers in the same run, the
legs alternating for ``--rounds`` rounds.

Per (mode, dim, nq) at ``--n`` rows, k = 10, and per allowed fraction (1.0 = the identity list: the cost of the
indirection alone; 0.5, 0.1, 0.01 as random rows):

* ``a_unfiltered``  ``flat_ip_topk`` / ``gemm_topk`` with ``engine="mfma"`` on all rows (off 1024: K5mf / K5md;
  at 1024: K5): the yardstick.  Its answer is not the filtered one; it is what the scan costs without a filter;
* ``b_rows``        the gathered call with a prebuilt list; ``b_list`` is ``filters.row_list`` alone (count, one
  host read, emit), paid once per filter;
* ``c_gather``      ``index_select`` of the allowed rows (float rows, int8 rows and norms, or code rows), ``flat_ip_prepare``
  of the copy for the float mode, and the unfiltered matrix call on it; ``c_gather_only`` is the copy (and
  prepare) alone;
* ``d_exact``       K5d (``engine="exact"``) over all rows: what ``b_rows`` has to beat at nq = 1.

Before timing, (b) is compared with (c) mapped back to corpus rows: rows equal, and score bits equal for the
cosine and binary modes (the float copy's own bounds may admit other candidates, never other results; at 1024 the
binary copy is searched by K5, whose scores are the same function but not the same pipeline: rows alone).  One JSON line per
(mode, dim, nq, fraction); times in ms are the median over the rounds with the min and max beside it.

    python tools/filtered_exhaustive_bench.py --out profiles/filtered_exhaustive_bench.jsonl
    python tools/filtered_exhaustive_bench.py --modes binary --out profiles/filtered_binary_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import search2_bench  # noqa: E402
from tools.search2_bench import reps_for, summary, window  # noqa: E402
from vectorragquantization_amd import filters  # noqa: E402
from vectorragquantization_amd.enhanced import gemm_topk  # noqa: E402
from vectorragquantization_amd.flat import flat_ip_prepare, flat_ip_topk  # noqa: E402
from vectorragquantization_amd.quant import int8_row_norms  # noqa: E402


def corpus(mode, n, dim, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(dim)
    if mode == "binary":
        return (torch.randint(0, 256, (n, dim // 8), generator=g, device=dev, dtype=torch.uint8),)
    if mode == "int8_cosine":
        x8 = torch.randint(-127, 128, (n, dim), generator=g, device=dev, dtype=torch.int8)
        return (x8, int8_row_norms(x8))
    xf = torch.nn.functional.normalize(torch.randn((n, dim), generator=g, device=dev), dim=1)
    bounds = torch.zeros((2,), dtype=torch.float64, device=dev)
    return (xf, *flat_ip_prepare(xf, bounds), bounds)


def search(mode, ops, qf, k, rows=None, engine="mfma"):
    if mode == "binary":
        return gemm_topk("binary", qf, k, codes=ops[0], rows=rows, engine=None if rows is not None else engine)
    if mode == "int8_cosine":
        return gemm_topk("int8_cosine", qf, k, x8=ops[0], norms=ops[1], rows=rows, engine=None if rows is not None else engine)
    if engine == "exact":
        return flat_ip_topk(ops[0], None, None, None, qf, k, engine="exact")
    return flat_ip_topk(*ops, qf, k, rows=rows, engine=None if rows is not None else engine)


def gather(mode, ops, idx):
    if mode == "binary":
        return (ops[0].index_select(0, idx),)
    if mode == "int8_cosine":
        return (ops[0].index_select(0, idx), ops[1].index_select(0, idx))
    xf = ops[0].index_select(0, idx)
    bounds = torch.zeros_like(ops[3])
    return (xf, *flat_ip_prepare(xf, bounds), bounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--modes", default="float_ip,int8_cosine")
    ap.add_argument("--dims", default="256,1024,2048")
    ap.add_argument("--nqs", default="1,64,1024")
    ap.add_argument("--fractions", default="1.0,0.5,0.1,0.01")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=search2_bench.MIN_WINDOW_MS)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    search2_bench.MIN_WINDOW_MS = a.window_ms
    dev = torch.device("cuda", 0)
    out = open(a.out, "a") if a.out else None
    n, k = a.n, a.k
    for mode in a.modes.split(","):
        for dim in (int(d) for d in a.dims.split(",")):
            ops = corpus(mode, n, dim, dev)
            for nq in (int(q) for q in a.nqs.split(",")):
                qf = torch.randn((nq, dim), device=dev)
                for frac in (float(f) for f in a.fractions.split(",")):
                    g = torch.Generator(device=dev)
                    g.manual_seed(int(frac * 1000) + 1)
                    mask = torch.rand((n,), generator=g, device=dev) < frac if frac < 1.0 else \
                        torch.ones(n, dtype=torch.bool, device=dev)
                    allow = filters.row_bitmap(mask)
                    rows = filters.row_list(allow, n)
                    idx = rows.to(torch.int64)
                    cb, rb, sb = search(mode, ops, qf, k, rows=rows)
                    cc, rc, sc = search(mode, gather(mode, ops, idx), qf, k)
                    mapped = torch.where(rc >= 0, idx[rc.clamp_min(0)], rc)
                    assert torch.equal(cb, cc) and torch.equal(rb, mapped), (mode, dim, nq, frac)
                    assert mode == "float_ip" or (mode == "binary" and dim == 1024) or \
                        torch.equal(sb.view(torch.int64), sc.view(torch.int64))
                    legs = {
                        "a_unfiltered": lambda: search(mode, ops, qf, k),
                        "b_rows": lambda: search(mode, ops, qf, k, rows=rows),
                        "b_list": lambda: filters.row_list(allow, n),
                        "c_gather": lambda: search(mode, gather(mode, ops, idx), qf, k),
                        "c_gather_only": lambda: gather(mode, ops, idx),
                        "d_exact": lambda: search(mode, ops, qf, k, engine="exact"),
                    }
                    reps = {name: reps_for(call, a.warmup) for name, call in legs.items()}
                    times = {name: [] for name in legs}
                    for _ in range(a.rounds):
                        for name, call in legs.items():
                            times[name].append(window(call, reps[name]))
                    rec = {"mode": mode, "dim": dim, "n": n, "nq": nq, "k": k, "fraction": frac, "m": int(rows.shape[0]),
                           "rounds": a.rounds, **{name: summary(t) for name, t in times.items()}}
                    for x in ("a_unfiltered", "c_gather", "d_exact"):
                        rec[f"b_over_{x[0]}"] = round(rec["b_rows"]["ms"] / rec[x]["ms"], 3)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()


if __name__ == "__main__":
    main()
