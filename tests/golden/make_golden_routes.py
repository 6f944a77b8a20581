"""Table of the host-side Phase-I decisions of libvrq.so -> ``tests/golden/phase1_routes.npz``, read by
tests/test_phase1_routes.py: which scan a call shape takes, its plan and sample plan, and the workspace
sizes.  It pins what the library built from the tree computes today, so run it only against a build whose
answers are the ones to keep.  CPU only: every function asked is a pure function of the call shape.

Over the grid DIMS x NS x NQS x KS x FLAGS (the edges the planners branch on) it records

* ``ws_search3`` / ``ws_dim`` / ``ws_search2`` / ``ws_topk``: vrq_search3_workspace_size (0 off 1024),
  vrq_search3_dim_workspace_size, vrq_search2_workspace_size, vrq_hamming_topk_workspace_size -- [dim, n, nq, K];
* ``kind`` [.., flags, 2]: the return code and ``prefix_rows`` of vrq_scan_kind;
* ``plan`` [.., flags, 13]: the return code and the 12 values of vrq_scan_plan;
* ``sample`` [.., flags, 7]: the return code and the 6 values of vrq_scan_sample_plan

(outputs a call does not write stay -1), and at ROUTE_SHAPE the workspace bytes of each of the two routes
per dim, ``route_bytes`` [dim, (wavefront, matrix)]: the matrix-core plan's total, and the chunk lists'
nq * nchunks * K * 8 -- read from the size at K = 129, where no matrix-core plan exists and the chunk
count is the same (it does not depend on K).

    python tests/golden/make_golden_routes.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from vectorragquantization_amd import _native as N  # noqa: E402

DIMS = (256, 384, 512, 768, 1024, 1536, 2048)
NS = (1000, 65_535, 65_536, 300_007, 1_000_000, 4_194_305, 100_000_000)
NQS = (1, 33, 64, 128, 129, 512, 1024)
KS = (10, 128, 129, 1024)
FLAGS = (0, N.VRQ_SEARCH_SCAN_VALU, N.VRQ_SEARCH_SCAN_MFMA)
ROUTE_SHAPE = (300_007, 4, 10)  # (n, nq, K) of the workspace refusals
OUT = os.path.join(HERE, "phase1_routes.npz")


def collect(lib) -> dict:
    g4 = (len(DIMS), len(NS), len(NQS), len(KS))
    t = {name: np.zeros(g4, np.int64) for name in ("ws_search3", "ws_dim", "ws_search2", "ws_topk")}
    t["kind"] = np.full(g4 + (len(FLAGS), 2), -1, np.int64)
    t["plan"] = np.full(g4 + (len(FLAGS), 13), -1, np.int64)
    t["sample"] = np.full(g4 + (len(FLAGS), 7), -1, np.int64)
    for i in np.ndindex(*g4):
        d, n, nq, K = DIMS[i[0]], NS[i[1]], NQS[i[2]], KS[i[3]]
        t["ws_search3"][i] = lib.vrq_search3_workspace_size(n, d, nq, K)
        t["ws_dim"][i] = lib.vrq_search3_dim_workspace_size(n, d, nq, K)
        t["ws_search2"][i] = lib.vrq_search2_workspace_size(n, d, nq, K)
        t["ws_topk"][i] = lib.vrq_hamming_topk_workspace_size(n, d // 8, nq, K)
        for f, flags in enumerate(FLAGS):
            kind, plan, sample = t["kind"][i + (f,)], t["plan"][i + (f,)], t["sample"][i + (f,)]
            kind[0] = lib.vrq_scan_kind(n, d, nq, K, flags, kind[1:].ctypes.data)
            plan[0] = lib.vrq_scan_plan(n, d, nq, K, flags, plan[1:].ctypes.data)
            sample[0] = lib.vrq_scan_sample_plan(n, d, nq, K, flags, sample[1:].ctypes.data)
    n, nq, K = ROUTE_SHAPE
    t["route_bytes"] = np.zeros((len(DIMS), 2), np.int64)
    info = np.zeros(12, np.int64)
    for j, d in enumerate(DIMS):
        at129 = lib.vrq_search3_dim_workspace_size(n, d, nq, 129)
        assert at129 > 0 and at129 % (nq * 129 * 8) == 0
        t["route_bytes"][j, 0] = at129 // 129 * K
        assert lib.vrq_scan_plan(n, d, nq, K, N.VRQ_SEARCH_SCAN_MFMA, info.ctypes.data) == N.VRQ_OK
        t["route_bytes"][j, 1] = info[11]
    return t


if __name__ == "__main__":
    tables = collect(N.load())
    np.savez_compressed(OUT, **tables)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in tables.items()})
