"""NumPy restatement of ``CohereVectorDBBinary`` (``CohereVectorDBBinary.py:133-239``) shared by the
fixture generator (tests/golden/make_golden_binary.py) and the tests of the signed-binary path
(tests/test_search2_capi.py, tests/test_gpu_binary.py); not a test module."""
import math
import os

import numpy as np

from oracle import oracle_np as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binary_synth.npz")
GOLDEN_ENCODERS = os.path.join(os.path.dirname(GOLDEN), "binary_encoders.npz")
SEARCH_DIMS = (1024, 256)
ENCODER_DIMS = (1024, 384)
SEARCHES = {"k10": (10, 10), "k5": (5, 3), "k30": (30, 2)}
NEW_ID = 9001          # the id added twice in one batch


def load_golden():
    """The search tables and the encoder tables of make_golden_binary.py in one dict."""
    return {**np.load(GOLDEN), **np.load(GOLDEN_ENCODERS)}


def sbin_codes(X) -> np.ndarray:
    """packbits(x >= float32 mean(x)) per row, MSB first (``_to_signed_binary`` + ``_pack_signed_binary``)."""
    X = np.asarray(X, np.float32).reshape(-1, np.shape(X)[-1])
    return np.stack([np.packbits(x >= x.mean(dtype=np.float32)) for x in X])


def signed_rows(codes, dim: int) -> np.ndarray:
    """The +-1 float32 rows packed codes unpack to (``_unpack_signed_binary``)."""
    return np.where(np.unpackbits(np.asarray(codes, np.uint8), axis=-1)[..., :dim] == 0, -1, 1).astype(np.float32)


def exact_dot(q, x) -> float:
    """The float32 dot as the library defines it: the exact sum of the exact products, rounded once."""
    p = np.asarray(q, np.float32).astype(np.float64) * np.asarray(x, np.float32).astype(np.float64)
    return float(np.float32(math.fsum(p.tolist())))


def apply_sequence(G, d: int, add, remove):
    """The golden document sequence at dim d through ``add(ids, X, texts)`` / ``remove(id)``: everything
    in 64-document batches, two removals, one id re-added with another vector, one new id twice in a batch."""
    F, ids = G[f"d{d}_F"], G[f"d{d}_ids"].tolist()
    texts = [f"t{i}" for i in range(len(ids))]
    for s in range(0, len(ids), 64):
        add(ids[s:s + 64], F[s:s + 64], texts[s:s + 64])
    remove(ids[10])
    remove(ids[11])
    add([ids[11], NEW_ID, NEW_ID], np.stack([F[12], F[5], F[6]]), ["t12", "t5", "t6"])


class BinaryOracleDB:
    """Document store + search of the reference class, float vectors in: ``add`` removes known ids first,
    adds the packed codes under the ids and keeps ``{id: (packed code, float row)}`` (the last write wins);
    ``search`` is ``:213-239`` with the float32 dot taken as the correctly rounded exact dot."""

    def __init__(self, dim: int):
        self.dim = dim
        self.index = O.IndexBinaryIDMap2(dim)
        self.store = {}

    def add(self, ids, X, texts=None):
        ids = [int(i) for i in ids]
        for e in ids:
            if e in self.store:
                self.remove(e)
        codes = sbin_codes(X)
        self.index.add_with_ids(codes, np.asarray(ids, np.int64))
        for j, e in enumerate(ids):
            self.store[e] = (codes[j], np.asarray(X[j], np.float32))

    def remove(self, e):
        if int(e) in self.store:
            self.index.remove_ids(np.array([int(e)], np.int64))
            del self.store[int(e)]

    def row(self, e, compare_float32: bool) -> np.ndarray:
        code, f = self.store[int(e)]
        return f if compare_float32 else signed_rows(code, self.dim)

    def score_of(self, qv, e, compare_float32: bool):
        """(score, float32 summation scale) of doc id e: ``score_of`` of test_vectordb_golden.check_table."""
        row = self.row(e, compare_float32)
        return exact_dot(qv, row), float(np.abs(np.asarray(qv, np.float64) * row.astype(np.float64)).sum())

    def search(self, qv, k: int = 10, binary_oversample: int = 10, compare_float32: bool = False):
        K = min(k * binary_oversample, self.index.ntotal)
        D, L = self.index.search(sbin_codes(qv), K)
        out = [(int(e), exact_dot(qv, self.row(e, compare_float32))) for e in L[0] if e != -1]
        out.sort(key=lambda h: h[1], reverse=True)
        return out[:k]


def result_tables(results, nq: int, k: int):
    """[(id, score), ...] per query -> (ids i64[nq, k] padded -1, scores f64[nq, k] padded NaN)."""
    gi, gs = np.full((nq, k), -1, np.int64), np.full((nq, k), np.nan)
    for j, r in enumerate(results):
        for p, (e, s) in enumerate(r):
            gi[j, p], gs[j, p] = e, s
    return gi, gs
