"""Golden tables of the reference's ``CohereVectorDBBinary`` -> ``tests/golden/binary_synth.npz`` (the search
tables) and ``tests/golden/binary_encoders.npz`` (the encoder tables, a file of their own so that each
committed file stays below 1 MiB), read by tests/test_search2_capi.py and tests/test_gpu_binary.py.

The reference module is imported in place (nothing is copied) through the machinery of ``make_golden.py``
and runs UNMODIFIED, constructor included, with these stand-ins for what is not installed:
``faiss`` (the oracle's ``IndexBinaryIDMap2``, as in ``make_golden.py``), a two-argument ``rocksdict.Rdict``
(an in-memory dict), ``azure.ai.inference.EmbeddingsClient`` / ``azure.core.credentials.AzureKeyCredential``,
the two environment variables, and ``db.client`` replaced by a table lookup that returns
``.data[0].embedding``.

* Encoder rows at d = 1024 and 384 (``x_{d}``) with the reference's packed output (``sbin_{d}`` =
  ``_pack_signed_binary(_to_signed_binary(x))``): the rows of ``make_encoder_inputs`` plus rows in which
  some but not all elements equal the float32 mean exactly (the repeating pattern 0, a, 0, -a, and one
  planted value in a constant row), which separate ``>=`` from ``>``; ``unpack_{d}`` is
  ``_unpack_signed_binary`` of those codes.
* Search tables at d = 1024 and 256: 300 clustered documents on a 2^-13 grid (the file stays below 1 MiB)
  with one identical pair under different ids, 20 queries; add in 64-document batches, remove two ids,
  re-add one id with another vector, add one id twice in a batch; ``search()`` at (k, oversample) =
  (10, 10), (5, 3), (30, 2) for both ``compare_float32`` values -> ids, scores, counts.
  The generator also runs the tests' oracle restatement (tests/binary_oracle.py: the float32 dot as the
  correctly rounded exact dot) against every table with ``check_table`` of tests/test_vectordb_golden.py
  and prints the number of queries whose order differs (the reference's sdot vs the exact dot).

    python tests/golden/make_golden_binary.py
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402
import binary_oracle as B  # noqa: E402
from test_vectordb_golden import check_table  # noqa: E402

N, NQ = 300, 20
GRID = 2.0 ** -13


class _Data:
    def __init__(self, v):
        self.embedding = v


class _Resp:
    def __init__(self, v):
        self.data = [_Data(v)] if v is not None else []


class _TableClient:
    """Stands in for the Azure ``EmbeddingsClient``: ``embed({"input": [text]})`` is a table lookup."""

    def __init__(self, table):
        self.table = table

    def embed(self, payload):
        v = self.table.get(payload["input"][0])
        return _Resp(None if v is None else v.tolist())


def _import_ref_class():
    MG._install_stubs()
    sys.modules["rocksdict"].Rdict = lambda path, options=None: {}
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            t = types.ModuleType("tqdm")
            t.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = t
    azure, ai, inf = types.ModuleType("azure"), types.ModuleType("azure.ai"), types.ModuleType("azure.ai.inference")
    core, cred = types.ModuleType("azure.core"), types.ModuleType("azure.core.credentials")
    inf.EmbeddingsClient = lambda endpoint=None, credential=None: None
    cred.AzureKeyCredential = lambda key: key
    azure.ai, ai.inference, azure.core, core.credentials = ai, inf, core, cred
    sys.modules.update({"azure": azure, "azure.ai": ai, "azure.ai.inference": inf, "azure.core": core,
                        "azure.core.credentials": cred})
    os.environ.setdefault("COHERE_EMBED_ENDPOINT", "http://embed.invalid/v2/embed")
    os.environ.setdefault("COHERE_EMBED_KEY", "none")
    if MG.REF not in sys.path:
        sys.path.insert(0, MG.REF)
    return __import__("CohereVectorDBBinary").CohereVectorDBBinary


def planted_rows(d: int) -> np.ndarray:
    """Rows with some, not all, elements exactly at the float32 mean."""
    rows = []
    for a in (0.25, 0.0625, 3.0):
        rows.append(np.tile(np.array([0.0, a, 0.0, -a]), d // 4))          # mean 0: half the elements tie
    r = np.tile(np.array([0.5, 0.5, 1.0, 0.0]), d // 4)                    # mean 0.5: half tie
    rows.append(r)
    r = np.zeros(d); r[::8] = 0.125; r[4::8] = -0.125                      # mean 0, three quarters tie
    rows.append(r)
    r = np.full(d, -0.375); r[1], r[2] = -0.375 + 2.0 ** -6, -0.375 - 2.0 ** -6   # mean = the constant
    rows.append(r)
    return np.asarray(rows, np.float32)


def gen_encoders(cls, res):
    rng = np.random.default_rng(20260101)
    for d in B.ENCODER_DIMS:
        X = np.concatenate([MG.make_encoder_inputs(d, rng), planted_rows(d)])
        for x in X[-planted_rows(d).shape[0]:]:
            at = int((x == np.mean(x)).sum())
            assert 0 < at < d, "a planted row must have some, not all, elements at the mean"
        res[f"x_{d}"] = X
        res[f"sbin_{d}"] = np.stack([cls._pack_signed_binary(cls._to_signed_binary(x)) for x in X])
        res[f"unpack_{d}"] = np.stack([cls._unpack_signed_binary(c, d) for c in res[f"sbin_{d}"][-8:]])
        res[f"planted_{d}"] = np.int64(planted_rows(d).shape[0])
        assert np.array_equal(B.sbin_codes(X), res[f"sbin_{d}"])
        differ = [not np.array_equal(np.packbits(x > np.mean(x)), c) for x, c in zip(X, res[f"sbin_{d}"])]
        assert all(differ[-planted_rows(d).shape[0]:]), ">= and > must differ on every planted row"


def gen_search(cls, d: int, res):
    rng = np.random.default_rng(7000 + d)
    F = MG.synth_corpus(rng, N, d, nclusters=12)
    F = (np.round(F.astype(np.float64) / GRID) * GRID).astype(np.float32)
    F[200] = F[7]                                         # identical vectors under different ids
    ids = np.arange(N, dtype=np.int64) * 2 + 100
    src = rng.integers(0, N, NQ)
    src[0], src[1] = 7, 12
    QF = (F[src] + (0.4 / np.sqrt(d)) * rng.standard_normal((NQ, d))).astype(np.float32)
    QF[0] = F[7]
    p = f"d{d}_"
    res.update({p + "F": F, p + "ids": ids, p + "QF": QF})
    table = {f"t{i}": F[i] for i in range(N)}
    with tempfile.TemporaryDirectory() as tmp:
        db = cls(os.path.join(tmp, "db"), embedding_dim=d)
        assert sorted(db.config) == ["embedding_dim", "model", "version"]
        db.client = _TableClient(table)
        B.apply_sequence(res, d, lambda i, X, t: db.add_documents(i, t, batch_size=64, save=False),
                         lambda e: db.remove_document(e, save=False))
        res[p + "id_map"] = db.index.id_map.copy()
        res[p + "codes"] = db.index.xb.copy()
        odb = B.BinaryOracleDB(d)
        B.apply_sequence(res, d, odb.add, odb.remove)
        assert np.array_equal(odb.index.id_map, res[p + "id_map"]) and np.array_equal(odb.index.xb, res[p + "codes"])
        for cname, (k, osb) in B.SEARCHES.items():
            for cf in (False, True):
                gi, gs, cnt = np.full((NQ, k), -1, np.int64), np.full((NQ, k), np.nan), np.zeros(NQ, np.int64)
                for j in range(NQ):
                    table[f"q{j}"] = QF[j]
                    r = db.search(f"q{j}", k=k, binary_oversample=osb, compare_float32=cf)
                    cnt[j] = len(r)
                    for i, h in enumerate(r):
                        gi[j, i], gs[j, i] = h["doc_id"], h["score"]
                key = f"{p}{cname}_{'f32' if cf else 'q'}"
                res.update({key + "_ids": gi, key + "_score": gs, key + "_cnt": cnt})
                oi, osc = B.result_tables([odb.search(QF[j], k, osb, cf) for j in range(NQ)], NQ, k)
                swapped = check_table(oi, osc, gi, gs, cnt, lambda q, e: odb.score_of(QF[q], e, cf))
                print(f"{key}: oracle (exact dot) vs reference (sdot): {swapped} of {NQ} queries order differently")


def main():
    cls = _import_ref_class()
    enc, res = {}, {}
    gen_encoders(cls, enc)
    for d in B.SEARCH_DIMS:
        gen_search(cls, d, res)
    for path, arrays in ((B.GOLDEN, res), (B.GOLDEN_ENCODERS, enc)):
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
