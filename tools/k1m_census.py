#!/usr/bin/env python
"""Instruction census of K1m's steady tile loop in a built gfx950 object (host side: disassembly, no GPU).

For each K1m instance (hamming_mfma_kernel<0,4>, <0,2>, <1,2>) the steady run is found as
tests/test_k1m_loop_shape.py finds it -- the innermost loop with exactly 32 * MB MFMAs on its fall-through
path -- and counted per kind: MFMA, VALU by mnemonic, SALU, DS by mnemonic, s_waitcnt, s_nop, branches,
VMEM.  One JSON line per instance; `non_mfma` is everything in the run that is not an MFMA.

Usage: k1m_census.py [--obj hamming_mfma.o] [--label parent] >> profiles/k1m_trim_census.jsonl"""
import argparse
import collections
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isa_check  # noqa: E402
import test_k1m_loop_shape as shape  # noqa: E402


def census(ins, mb):
    """Per-kind counts of the steady run of one kernel's instruction list (isa_check.parse)."""
    run = shape.steady_loop(ins, mb)
    if run is None:
        return None
    c = shape.loop_counts(ins, run)
    valu, ds = collections.Counter(), collections.Counter()
    for i in run:
        op = ins[i][1]
        if shape.is_mfma(ins[i]):
            continue
        if op.startswith("v_"):
            valu[op] += 1
        elif op.startswith("ds_"):
            ds[op] += 1
    out = dict(c)
    out["barrier"] = sum(1 for i in run if ins[i][1] == "s_barrier")
    out["non_mfma"] = len(run) - c["mfma"]
    out["bytes"] = ins[run[-1]][0] - ins[run[0]][0]  # header to back edge (cold blocks laid out after it excluded)
    out["valu_by_op"] = dict(sorted(valu.items()))
    out["ds_by_op"] = dict(sorted(ds.items()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", default=os.path.join(ROOT, "vectorragquantization_amd", "_obj", "hamming_mfma.o"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as wd:
        funcs = isa_check.parse(isa_check.disassemble(a.obj, wd))
    for inst in sorted(shape.INSTANCES):
        key, mb = shape.INSTANCES[inst]
        names = [k for k in funcs if key in k]
        if len(names) != 1:
            sys.exit("kernel %s: %d symbols" % (key, len(names)))
        c = census(funcs[names[0]], mb)
        if c is None:
            sys.exit("kernel %s: no loop with %d MFMAs on its fall-through path" % (key, 32 * mb))
        print(json.dumps({"label": a.label, "instance": inst, **c}))


if __name__ == "__main__":
    main()
