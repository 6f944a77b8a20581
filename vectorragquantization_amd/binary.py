"""``CohereVectorDBBinary`` on MI355X: the reference's signed-binary store (``CohereVectorDBBinary.py``).

Each float32 embedding is thresholded at its own mean with ``>=`` (``_to_signed_binary``, ``:133-141``)
and packed MSB-first (``_pack_signed_binary``, ``:143-150``); the packed code is both the FAISS
``IndexBinaryIDMap2`` entry and the stored row that the search rescoring unpacks to a +-1 float vector
(``_unpack_signed_binary``, ``:152-159``).  Here ``add_vectors`` encodes a whole batch in one
``vrq_encode`` launch (mode ``sbin``) and ``search_vectors`` is ONE fused ``vrq_search2`` call per query
batch (``quant.search2``): the Phase-I Hamming scan over the codes, then a finish kernel that scores
each candidate against the same packed codes (mode ``VRQ_RESCORE_SIGNED_BINARY``) or, with
``compare_float32=True``, against the float32 rows kept from ``add_documents`` (``VRQ_RESCORE_F32``),
sorts stably by score and cuts to k (``search``, ``:196-239``).

Constructor, ``add_documents``, ``search``, ``remove_document``, ``save``, ``__len__`` and the three
static methods keep the reference's names, argument meaning, result dicts (``doc_id`` / ``score`` /
``doc``) and error behaviour; ``config.json`` has the reference's keys.  Like the reference, float32
rows live only in memory: after reopening a folder ``search(..., compare_float32=True)`` raises
``KeyError`` for a hit without one.  The rescoring of a duplicated id reads the vector of its last add (the
reference's ``doc_db[str(id)]``).  Storage: ``index.bin`` (FAISS's IBM2 format) plus this build's
``vrq_docs/`` (texts and ``packed_binary``); the reference ships no persisted folder of this class.
Embeddings come from ``provider.embed_floats(texts)`` (``embed.TableProvider`` offline; by default
``embed.AzureEmbeddingsHTTPProvider``, the reference's ``{"input": [text]}`` request).
"""
from __future__ import annotations

import json
import logging
import os

import numpy as np
import torch

from . import quant as Q
from .docstore import DocStoreError
from .filters import class_filter, ids_bitmap
from .index import _GrowBuffer, as_device_tensor
from .vectordb import _QuantizedVectorDB

logger = logging.getLogger(__name__)


class CohereVectorDBBinary(_QuantizedVectorDB):
    """``CohereVectorDBBinary.py:31``: signed-binary codes, two-phase search (Hamming, then the float
    query against the +-1 row or the float32 row)."""
    MODE, QKEY, QDTYPE = "sbin", "packed_binary", torch.uint8
    EMPTY_MSG = "To create a new database, the folder must be empty."

    def __init__(self, folder: str, model: str = "cohere-embed-english-v3.0", embedding_dim: int = 1024,
                 rdict_options=None, provider=None, device=None):
        if provider is None:   # raises like the reference's constructor when the variables are unset (:52-61)
            from .embed import AzureEmbeddingsHTTPProvider
            provider = AzureEmbeddingsHTTPProvider(embedding_dim=embedding_dim)
        super().__init__(folder, model, embedding_dim, None, rdict_options, getattr(provider, "endpoint", None),
                         provider, device)

    # -- the reference's host-side static methods (one vector, NumPy) ------------------------
    @staticmethod
    def _to_signed_binary(embedding: np.ndarray) -> np.ndarray:
        """+1 where ``embedding >= np.mean(embedding)``, else -1 (int8); ``:133-141``."""
        embedding = np.asarray(embedding)
        return np.where(embedding >= np.mean(embedding), 1, -1).astype(np.int8)

    @staticmethod
    def _pack_signed_binary(signed_binary: np.ndarray) -> np.ndarray:
        """-1 -> 0, +1 -> 1, ``np.packbits`` (MSB first); ``:143-150``."""
        return np.packbits(((np.asarray(signed_binary) + 1) // 2).astype(np.uint8))

    @staticmethod
    def _unpack_signed_binary(packed: np.ndarray, length: int) -> np.ndarray:
        """The +-1 float32 vector of a packed code; ``:152-159``."""
        bits = np.unpackbits(np.asarray(packed, np.uint8))[:length]
        return np.where(bits == 0, -1, 1).astype(np.float32)

    # -- layout: the stored row is the index code itself; only the float rows are kept beside it --
    def _reset_rows(self):
        self._f = _GrowBuffer((self.embedding_dim,), torch.float32, self.device)

    def _load_docs(self):
        n = self.index.ntotal
        tj = os.path.join(self._docs_path(), "texts.json")
        if os.path.exists(tj):
            with open(tj) as fh:
                self.texts = {int(a): b for a, b in json.load(fh).items()}
        elif n:
            raise DocStoreError(f"{self.folder}: index.bin holds {n} rows but there is no vrq_docs/ store")
        if n:   # one (absent) float row per index row, so that candidate rows index the buffer
            self._f.append(torch.zeros((n, self.embedding_dim), dtype=torch.float32, device=self.device))

    def save(self):
        """index.bin in FAISS's IBM2 format + vrq_docs/ (texts.json and packed_binary.npy, the value the
        reference keeps per document in its RocksDict); float rows are not persisted, as in the reference."""
        self.index.write(os.path.join(self.folder, "index.bin"))
        p = self._docs_path()
        os.makedirs(p, exist_ok=True)
        np.save(os.path.join(p, "packed_binary.npy"), self.index.codes.cpu().numpy())
        with open(os.path.join(p, "texts.json"), "w") as f:
            json.dump({str(a): b for a, b in self.texts.items()}, f)
        logger.info("FAISS index saved to disk.")

    # -- documents ---------------------------------------------------------------------------
    def add_vectors(self, doc_ids, X, docs=None, save: bool = False) -> None:
        """Append float32 embeddings (f32[m, d]) without HTTP: one ``vrq_encode`` launch packs the batch."""
        ids = np.asarray(doc_ids.cpu() if isinstance(doc_ids, torch.Tensor) else doc_ids, dtype=np.int64).reshape(-1)
        X = as_device_tensor(X, torch.float32, self.device).reshape(ids.shape[0], self.embedding_dim)
        self.index.add_with_ids(Q.encode("sbin", X, device=self.device)["codes"], ids)
        self._f.append(X)
        self._float_ids.update(ids.tolist())
        if docs is None:
            docs = [""] * ids.shape[0]
        for i, d in zip(ids.tolist(), docs):
            self.texts[i] = d
        if save:
            self.save()

    def remove_document(self, doc_id: int, save: bool = True):
        if int(doc_id) in self.texts:
            keep = self.index.id_map != int(doc_id)
            self.index._compact(keep)
            self._f.keep(keep)
            del self.texts[int(doc_id)]
            self._float_ids.discard(int(doc_id))
            logger.info(f"Document {doc_id} removed from the database.")
        else:
            logger.warning(f"Document {doc_id} not found in the database.")
        if save:
            self.save()

    # -- search ------------------------------------------------------------------------------
    def search_vectors(self, query, k: int = 10, binary_oversample: int = 10, compare_float32: bool = False,
                       allowed_ids=None, engine=None, allowed_ids_per_query=None):
        """Batched search of float32 query embeddings (f32[nq, d]) on the device, one ``vrq_search2`` call.
        Returns (doc_id i64[nq, kk], row i64[nq, kk], hamming i32[nq, kk], score f64[nq, kk]) with
        kk = min(k, K); rows past the candidates are -1.  ``allowed_ids`` (None: all): only these documents
        are searched (``vrq_search2_filtered``); ids the index does not hold are ignored.  ``engine`` ("auto",
        "mfma", "valu"; default None): ``vrq_search2_batch``, the counting scan on the named engine.
        ``allowed_ids_per_query`` (exclusive with ``allowed_ids``): a sequence of nq entries, each None
        (unfiltered) or a collection of ids, one filter per query through the ``*_perquery`` call, where
        ``engine=None`` means "auto"; an empty collection, or one of unknown ids, finds nothing."""
        if k < 0 or binary_oversample < 0:
            raise ValueError("k and binary_oversample must be non-negative")
        qv = as_device_tensor(query, torch.float32, self.device).reshape(-1, self.embedding_dim)
        qb = Q.encode("sbin", qv, device=self.device)["codes"]
        codes = self.index.codes
        allow, qset = class_filter(self.index.id_map, allowed_ids, allowed_ids_per_query, qv.shape[0])
        with torch.cuda.device(self.device):
            rows, ham, sc = Q.search2("f32" if compare_float32 else "sbin", codes,
                                      self._f.view() if compare_float32 else codes, qv, qb, k, binary_oversample,
                                      rescore_row=self.index.rescore_rows(), allow=allow, engine=engine,
                                      query_set=qset)
        if compare_float32:
            self._check_float_rows(rows)
        ids = torch.where(rows >= 0, self.index.id_map[rows.clamp_min(0)], rows) if self.index.ntotal else rows
        return ids, rows, ham, sc
