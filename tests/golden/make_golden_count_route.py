"""Table of the host-side decisions of the counting scan (K1h / K1hm) -> ``tests/golden/count_route_plans.npz``,
read by tests/test_count_route_plans.py: the plan of each engine, AUTO's choice and every workspace size of
the *_large, *_filtered, *_batch and sharded *_large calls.  It pins what the library built from the tree
computes, so run it only against a build whose answers are the ones to keep.  CPU only: every function asked
is a pure function of the call shape.

Over the grid DIMS x NS x NQS x KS (one unsupported dim; the K1hm flush boundary at 65 280 rows; both AUTO
thresholds; the second pass at 513 queries; the chunk-count caps at large n; every refusal) it records

* ``large`` [.., 9]: the return code and the 8 values of vrq_scan_large_plan;
* ``batch`` [.., engine, 11]: the return code and the 10 values of vrq_scan_batch_plan under AUTO, VALU, MFMA;
* ``engine`` [.., 2]: vrq_large_engine without and with ``filtered``;
* ``ws`` [.., 13]: the workspace-size functions WS_NAMES, in that order (code bytes for the hamming_topk ones)

(outputs a call does not write stay -1).

    python tests/golden/make_golden_count_route.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from vectorragquantization_amd import _native as N  # noqa: E402

DIMS = (256, 384, 512, 768, 1024, 1536, 2048, 320)
NS = (1, 63, 4096, 65_280, 65_281, 1_000_000, 100_000_000, 2 ** 32 - 1, 2 ** 32)
NQS = (1, 15, 16, 32, 33, 64, 65, 512, 513, 1024)
KS = (1, 1024, 1025, 8192, 8193)
ENGINES = (N.VRQ_LARGE_ENGINE_AUTO, N.VRQ_LARGE_ENGINE_VALU, N.VRQ_LARGE_ENGINE_MFMA)
WS_NAMES = tuple(f"vrq_{call}_{family}_workspace_size"
                 for family, calls in (("large", ("hamming_topk", "search3", "search2")),
                                       ("filtered", ("scan", "hamming_topk", "search3", "search2")),
                                       ("batch", ("scan", "hamming_topk", "search3", "search2")))
                 for call in calls) + ("vrq_shard_search3_large_workspace_size",
                                       "vrq_shard_search2_large_workspace_size")
OUT = os.path.join(HERE, "count_route_plans.npz")


def collect(lib) -> dict:
    g4 = (len(DIMS), len(NS), len(NQS), len(KS))
    t = {"large": np.full(g4 + (9,), -1, np.int64), "batch": np.full(g4 + (len(ENGINES), 11), -1, np.int64),
         "engine": np.zeros(g4 + (2,), np.int64), "ws": np.zeros(g4 + (len(WS_NAMES),), np.int64)}
    for i in np.ndindex(*g4):
        d, n, nq, K = DIMS[i[0]], NS[i[1]], NQS[i[2]], KS[i[3]]
        large = t["large"][i]
        large[0] = lib.vrq_scan_large_plan(n, d, nq, K, large[1:].ctypes.data)
        for e, engine in enumerate(ENGINES):
            batch = t["batch"][i + (e,)]
            batch[0] = lib.vrq_scan_batch_plan(n, d, nq, K, engine, batch[1:].ctypes.data)
        t["engine"][i] = [lib.vrq_large_engine(n, d, nq, K, f) for f in (0, 1)]
        t["ws"][i] = [getattr(lib, name)(n, d // 8 if "hamming_topk" in name else d, nq, K) for name in WS_NAMES]
    return t


if __name__ == "__main__":
    tables = collect(N.load())
    np.savez_compressed(OUT, **tables)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in tables.items()})
