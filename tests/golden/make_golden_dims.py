"""Golden tables of the reference's own three-phase search at embedding dims 384 and 1536:
``tests/golden/search_dims.npz`` (+ ``search_dims_int8_1536.npz``, the one array that would push the
file past 1 MiB), read by tests/test_gpu_dims.py.

Runs the reference's ``CohereEnhancedVectorDB.add_documents`` / ``remove_document`` / ``search``
(``embedding_dim`` = d) through the import machinery and stubs of ``make_golden.py`` (same reference
checkout, same FAISS / RocksDict stand-ins).  Per dim d: 600 clustered unit vectors with planted
duplicates, a duplicated code with a different int8 row, a zero int8 row, external ids != rows, 16
queries rounded to a multiple of 2^-24.  On that grid every partial sum of +-q_i is a multiple of
2^-24 below 2^11, hence exact in float64 in ANY summation order: the bit-equality check on the
Phase-II scores does not depend on how the reference's BLAS orders its sums.  The generator asserts
that, and that the reference's Phase-III order is the same under NumPy's float32 dot and under the
correctly rounded dot (no query's result depends on the float32 summation order).

    python tests/golden/make_golden_dims.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

DIMS = (384, 1536)
PARAMS = {"k10": (10, 10, 3), "k7": (7, 4, 2), "k30": (30, 10, 3)}
N, NQ = 600, 16
GRID = 2.0 ** -24


def ref_db(d: int, doc_lookup: dict, query_lookup: dict):
    CE = MG._import_ref("CohereEnhancedVectorDB").CohereEnhancedVectorDB
    db = object.__new__(CE)            # skip __init__ (env vars / folders)
    db.embedding_dim = d
    db.model = "embed-english-v3.0"
    db.folder = "/nonexistent"
    db.config = {"model": db.model}
    db.index = O.IndexBinaryIDMap2(d)
    db.doc_db = {}

    def _get_embeddings(texts, input_type, embedding_types):
        if input_type == "search_query":
            f, b = query_lookup[texts[0]]
            return {"float": [f.tolist()], "ubinary": [b.tolist()]}
        return {"int8": [doc_lookup[t][0].tolist() for t in texts],
                "ubinary": [doc_lookup[t][1].tolist() for t in texts]}

    db._get_embeddings = _get_embeddings
    return db


def check_order_independence(d, codes, int8, ids, QF, QB):
    """Phase II exact in any order; Phase-III top-k order the same under sdot and the exact dot."""
    pm = 2.0 * np.unpackbits(codes, axis=1).astype(np.float64) - 1.0
    q64 = QF.astype(np.float64)
    fwd = np.array([[np.add.reduce(pm[r] * q) for r in range(codes.shape[0])] for q in q64])
    rev = np.array([[np.add.reduce((pm[r] * q)[::-1]) for r in range(codes.shape[0])] for q in q64])
    perm = np.random.default_rng(d).permutation(d)
    shuf = np.array([[sum((pm[r] * q)[perm].tolist()) for r in range(codes.shape[0])] for q in q64])
    assert np.array_equal(fwd, rev) and np.array_equal(fwd, shuf), "Phase-II sums depend on the order"
    norms = O.int8_row_norms(int8)
    changed = 0
    for k, osb, osi in PARAMS.values():
        ref = O.three_phase_batch(codes, int8, ids, QF, QB, k, osb, osi)
        for q in range(QF.shape[0]):
            o = ref[q]
            p2 = o["p1_rows"][o["p2_order"]]
            exact = np.array([-np.inf if norms[r] == 0 else
                              float(np.float32(q64[q] @ int8[r].astype(np.float64))) / norms[r] for r in p2])
            o3 = sorted(range(p2.shape[0]), key=lambda j: -exact[j])[:k]
            changed += not np.array_equal(p2[o3], o["row"])
    assert changed == 0, f"{changed} queries order differently under the correctly rounded dot"


def gen_dim(d: int, res: dict):
    rng = np.random.default_rng(1000 + d)
    F = MG.synth_corpus(rng, N, d)
    for a, b in ((10, 300), (11, 301), (11, 302), (250, 599)):
        F[b] = F[a]
    Q8 = np.stack([O.quantize_int8_global(x, 3.0 / np.sqrt(d)) for x in F])
    CB = np.stack([O.to_binary_sign(x) for x in F])
    CB[400] = CB[20]                                    # Phase I / II tie, Phase III split
    Q8[534] = 0                                         # norm == 0 -> -inf cosine
    ids = np.arange(N, dtype=np.int64) * 3 + 1000
    src = rng.integers(0, N, NQ)
    src[:4] = (10, 11, 20, 534)
    QF = F[src] + (0.3 / np.sqrt(d)) * rng.standard_normal((NQ, d)).astype(np.float32)
    QF[0] = F[10]
    QF /= np.linalg.norm(QF, axis=1, keepdims=True)
    QF = (np.round(QF.astype(np.float64) / GRID) * GRID).astype(np.float32)   # the 2^-24 grid
    assert np.array_equal(QF.astype(np.float64) / GRID, np.round(QF.astype(np.float64) / GRID))
    QB = np.stack([O.to_binary_sign(x) for x in QF])
    check_order_independence(d, CB, Q8, ids, QF, QB)

    docs = {f"t{i}": (Q8[i], CB[i]) for i in range(N)}
    qlk = {}
    db = ref_db(d, docs, qlk)
    db.add_documents([int(x) for x in ids], [f"t{i}" for i in range(N)], batch_size=64, save=False)
    p = f"d{d}_"
    res.update({p + "int8": Q8, p + "codes": CB, p + "ids": ids, p + "qf": QF, p + "qb": QB})
    for tag, (k, osb, osi) in PARAMS.items():
        for kk, v in MG.search_table(db, QF, QB, k, osb, osi, qlk).items():
            res[f"{p}{tag}_{kk}"] = v
        res[f"{p}{tag}_params"] = np.array([k, osb, osi])
    if d != 384:
        return
    # small corpus (k * os > ntotal) with removals and a re-add, as gen_search_synth's
    db2 = ref_db(d, docs, qlk)
    small = [5, 6, 7, 8, 9, 10, 300, 11, 301, 302, 20, 400, 534, 33, 34, 35, 36, 37, 38, 39]
    db2.add_documents(small, [f"t{i}" for i in small], batch_size=8, save=False)
    db2.remove_document(8, save=False)
    db2.remove_document(36, save=False)
    db2.add_documents([36, 40, 7], ["t36", "t40", "t599"], batch_size=64, save=False)   # 7 re-added with t599
    res[p + "small_rows_ids"] = db2.index.id_map.copy()
    res[p + "small_codes"] = db2.index.xb.copy()
    res[p + "small_int8"] = np.stack([np.asarray(db2.doc_db[str(int(e))]["int8"], np.int8)
                                      for e in db2.index.id_map])
    for kk, v in MG.search_table(db2, QF, QB, 10, 10, 3, qlk).items():
        res[f"{p}small_{kk}"] = v


def main():
    res = {}
    for d in DIMS:
        gen_dim(d, res)
    # int8 rows barely compress (7.4 bits of entropy per value): the 1536-dim corpus's 0.9 MB goes to a
    # file of its own so that each committed file stays below 1 MiB
    big = {"d1536_int8": res.pop("d1536_int8")}
    for name, arrays in (("search_dims.npz", res), ("search_dims_int8_1536.npz", big)):
        out = os.path.join(HERE, name)
        np.savez_compressed(out, **arrays)
        assert os.path.getsize(out) < 1 << 20, (name, os.path.getsize(out))
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
