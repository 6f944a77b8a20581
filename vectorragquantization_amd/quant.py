"""Scalar-quantise + packbits encode path of the ``VectorDBInt{4,8,16}{,Global}`` classes on MI355X.

``encode(mode, X, limit)`` runs one gfx950 kernel launch (``vrq_encode``, one
wave per vector) over a whole batch of embeddings resident in HBM and returns
device tensors.  The classes below mirror the reference's static encoder
methods (same names, same argument meaning, same return types: NumPy arrays,
plus ``(q, min, max)`` tuples for the local quantizers) so reference call sites
keep working; they accept one vector (1-D) or a batch (2-D):

=====================  ==========================================  ==================
reference              method                                       mode
=====================  ==========================================  ==================
VectorDBInt8Global     ``_quantize_to_int8`` (``:130-142``)          ``int8g``
VectorDBInt16Global    ``_quantize_to_int16`` (``:130-142``)         ``int16g``
VectorDBInt4Global     ``_quantize_to_int4`` (``:129-164``, bug)     ``int4g``
VectorDBInt8           ``_quantize_to_int8`` (``:114-126``)          ``int8``
VectorDBInt4           ``_quantize_to_int4`` (``:116-154``)          ``int4``
VectorDBInt16          ``_to_binary`` on int16 (``:148-157``)        ``bin16``
all of them            ``_to_binary`` (e.g. ``VectorDBInt8Global.py:154-160``)
CohereVectorDBBinary   ``_to_signed_binary`` + ``_pack_signed_binary``  ``sbin`` (codes only)
=====================  ==========================================  ==================
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from .filters import checked as checked_bitmap, checked_filter
from .index import _device, as_device_tensor


def encode(mode: str, X, limit: float = 0.3, device=None) -> dict:
    """Batch encode on device.  X: f32[n, d] (i16[n, d] for ``bin16``).

    Returns ``{"codes": u8[n, d/8], "q": int8[n,d] | int16[n,d] | int8[n,d/2] | None,
    "minmax": f64[n,2] | None}`` as device tensors.  ``sbin`` (``CohereVectorDBBinary``,
    ``packbits(x >= mean(x))``) and ``bin16`` give codes only; ``limit`` is ignored by them.
    """
    if mode not in N.ENC_MODES:
        raise ValueError(f"unknown encode mode {mode!r}")
    dev = _device(device)
    in_dtype = torch.int16 if mode == "bin16" else torch.float32
    X = as_device_tensor(X, in_dtype, dev)
    if X.dim() == 1:
        X = X.reshape(1, -1)
    n, d = X.shape
    codes = torch.empty((n, d // 8), dtype=torch.uint8, device=dev)
    q = None
    if mode in ("int8g", "int8", "cohere"):
        q = torch.empty((n, d), dtype=torch.int8, device=dev)
    elif mode == "int16g":
        q = torch.empty((n, d), dtype=torch.int16, device=dev)
    elif mode in ("int4g", "int4"):
        q = torch.empty((n, (d + 1) // 2), dtype=torch.int8, device=dev)
    mm = torch.empty((n, 2), dtype=torch.float64, device=dev) if mode in ("int8", "int4") else None
    lib = N.load()
    with torch.cuda.device(dev):
        rc = lib.vrq_encode(N.ENC_MODES[mode], N.ptr(X), n, d, float(limit), N.ptr(codes), N.ptr(q), N.ptr(mm),
                            N.stream_handle(dev))
    N.check(rc, f"vrq_encode({mode})")
    return {"codes": codes, "q": q, "minmax": mm}


_DEQ_MODES = {"int8g": 0, "int16g": 1, "int4g": 2, "int8": 3, "int4": 4}


def dequantize(mode: str, q, minmax=None, limit: float = 0.0, dim: int = None, device=None) -> torch.Tensor:
    """Device ``_dequantize_*`` of the VectorDB* classes for a batch of rows (``vrq_dequantize``):
    ``int8g``/``int16g``/``int4g`` take the global ``limit``, ``int8``/``int4`` the per-row
    (min, max) f64[n, 2].  Returns f32[n, dim] on the device, bit-identical to the reference."""
    dev = _device(device)
    dt = {"int8g": torch.int8, "int8": torch.int8, "int16g": torch.int16, "int4g": torch.int8, "int4": torch.int8}[mode]
    q = as_device_tensor(q, dt, dev)
    if q.dim() == 1:
        q = q.reshape(1, -1)
    n = q.shape[0]
    d = dim if dim is not None else (2 * q.shape[1] if mode in ("int4g", "int4") else q.shape[1])
    mm = as_device_tensor(np.asarray(minmax, np.float64).reshape(n, 2), torch.float64, dev) if minmax is not None else None
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    lib = N.load()
    with torch.cuda.device(dev):
        rc = lib.vrq_dequantize(_DEQ_MODES[mode], N.ptr(q), N.ptr(mm), n, d, float(limit), N.ptr(out),
                                N.stream_handle(dev))
    N.check(rc, f"vrq_dequantize({mode})")
    return out


def vectordb_search(mode: str, codes: torch.Tensor, q: torch.Tensor, qf: torch.Tensor, qb: torch.Tensor, k: int = 10,
                    binary_oversample: int = 10, minmax: torch.Tensor = None, limit: float = 0.0,
                    rescore_row: torch.Tensor = None, allow: torch.Tensor = None, engine: str = None,
                    query_set: torch.Tensor = None):
    """``VectorDBInt{4,8,16}{,Global}.search`` for a query batch (e.g. VectorDBInt8Global.py:205-252):
    Phase I Hamming top-``k * binary_oversample`` over the ubinary codes (``vrq_hamming_topk``, FAISS
    order), Phase II ``float(np.dot(query_float, doc_emb))`` (``vrq_rescore_dequant``), Python's stable
    sort by score descending, first k.  ``doc_emb`` is the dequantised row of ``mode`` or, for
    ``mode="f32"`` (the ``compare_float32`` branch, ``:239-240``), the f32 float row ``q``.
    ``mode="bin16"`` (VectorDBInt16.search) stops after Phase I and ranks by Hamming distance.
    ``rescore_row`` (i64[n], optional) maps an index row to the row whose stored vector the
    reference's ``doc_db[str(id)]`` lookup returns (the last add of a duplicated id).
    ``allow`` (``filters.row_bitmap``): Phase I over the allowed rows only (``vrq_hamming_topk_filtered``, the
    counting scan, for every K up to VRQ_K_LARGE_MAX), then the same rescoring.
    ``engine`` ("auto", "mfma", "valu"; default None = the routes above): Phase I through
    ``vrq_hamming_topk_batch``, the counting scan on the named engine, with or without ``allow``.
    ``query_set`` (an int tensor [nq]) with a 2-D ``allow`` (``filters.row_bitmaps``): a bitmap per query
    (-1: unfiltered), Phase I through ``vrq_hamming_topk_perquery``, where ``engine=None`` means "auto".
    Returns (rows i64[nq, k], hamming i32[nq, k], score f64[nq, k]) on the device; rows past the
    corpus are -1 (score NaN)."""
    dev = codes.device
    n, cb = codes.shape
    nq = qb.shape[0]
    K = min(k * binary_oversample, n)
    lib = N.load()
    dist = torch.empty((nq, K), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, K), dtype=torch.int64, device=dev)
    # more than 1024 candidates, a bitmap or an engine: the counting scan, up to VRQ_K_LARGE_MAX
    call = N.SearchCall("vrq_hamming_topk", K, 0, allow, engine, "vectordb_search", query_set=query_set)
    allow, query_set = checked_filter(allow, query_set, n, nq, dev)
    ws = call.workspace(lib, n, cb, nq, K, dev)
    with torch.cuda.device(dev):
        call(lib, (N.ptr(codes), n, cb, 0, N.ptr(qb), nq, K), (N.ptr(dist), N.ptr(rows)), allow, ws, dev,
             query_set=query_set)
    if mode == "bin16":
        kk = min(k, K)
        return rows[:, :kk], dist[:, :kk], dist[:, :kk].to(torch.float64)
    if q is None or q.shape[0] != n or (minmax is not None and minmax.shape[0] != n):
        # the ABI indexes q / minmax by candidate row and cannot see their lengths
        raise N.VrqNativeError(f"vectordb_search: {n} code rows but {None if q is None else q.shape[0]} stored rows")
    cand = rows
    if rescore_row is not None:
        cand = torch.where(rows >= 0, rescore_row[rows.clamp_min(0)], rows).contiguous()
    score = torch.empty((nq, K), dtype=torch.float64, device=dev)
    d = qf.shape[1]
    m = N.VRQ_RESCORE_F32 if mode == "f32" else _DEQ_MODES[mode]
    with torch.cuda.device(dev):
        N.check(lib.vrq_rescore_dequant(m, N.ptr(qf), nq, d, N.ptr(q), N.ptr(minmax), float(limit), n,
                                        N.ptr(cand), K, N.ptr(score), N.stream_handle(dev)), "vrq_rescore_dequant")
    # Python's stable sort by score desc over the Phase-I order (VectorDBInt8Global.py:251);
    # missing candidates (-1) sort last, -0.0 ties +0.0
    key = torch.where(rows >= 0, score + 0.0, torch.full_like(score, float("-inf")))
    o = torch.sort(-key, dim=1, stable=True).indices[:, :k]
    return torch.gather(rows, 1, o), torch.gather(dist, 1, o), torch.gather(score, 1, o)


_SEARCH2_MODES = {**_DEQ_MODES, "f32": N.VRQ_RESCORE_F32, "sbin": N.VRQ_RESCORE_SIGNED_BINARY}


def search2(mode: str, codes: torch.Tensor, q: torch.Tensor, qf: torch.Tensor, qb: torch.Tensor, k: int = 10,
            binary_oversample: int = 10, minmax: torch.Tensor = None, limit: float = 0.0,
            rescore_row: torch.Tensor = None, flags: int = 0, allow: torch.Tensor = None, engine: str = None,
            query_set: torch.Tensor = None):
    """The two-phase search of ``vectordb_search`` as ONE fused call (``vrq_search2``: the Phase-I scan and
    a finish kernel that merges, rescores, sorts and cuts; ``CohereVectorDBBinary.py:215-239`` and the same
    loop of the ``VectorDBInt*`` classes).  ``mode`` is a ``vectordb_search`` rescoring mode (``int8g`` ...
    ``int4``, ``f32``) or ``sbin``: ``q`` = packed sign codes (normally ``codes`` itself) scored as +-1
    rows.  ``flags``: 0, ``VRQ_SEARCH_SCAN_VALU`` or ``VRQ_SEARCH_SCAN_MFMA``.  Same return contract as
    ``vectordb_search``: (rows i64[nq, kk], hamming i32[nq, kk], score f64[nq, kk]) on the device,
    kk = min(k, K); rows past the corpus are -1 (score NaN).  ``allow`` (``filters.row_bitmap``): Phase I over
    the allowed rows only, ``vrq_search2_filtered`` for every K up to VRQ_K_LARGE_MAX (no flags).
    ``engine`` ("auto", "mfma", "valu"; default None = the routes above): ``vrq_search2_batch``, the counting
    scan on the named engine for every K up to VRQ_K_LARGE_MAX, with or without ``allow`` (no flags).
    ``query_set`` (an int tensor [nq]) with a 2-D ``allow`` (``filters.row_bitmaps``): a bitmap per query
    (-1: unfiltered), ``vrq_search2_perquery``, where ``engine=None`` means "auto" (no flags)."""
    if mode not in _SEARCH2_MODES:
        raise ValueError(f"unknown search2 mode {mode!r}")
    dev = codes.device
    n, cb = codes.shape
    nq, d = qf.shape
    K = min(k * binary_oversample, n)
    kk = min(k, K)
    rows = torch.empty((nq, kk), dtype=torch.int64, device=dev)
    dist = torch.empty((nq, kk), dtype=torch.int32, device=dev)
    score = torch.empty((nq, kk), dtype=torch.float64, device=dev)
    if nq == 0 or kk == 0:
        return rows, dist, score
    if d != cb * 8 or qb.shape != (nq, cb):
        raise N.VrqNativeError(f"search2: {cb}-byte codes but queries of dim {d} / codes {tuple(qb.shape)}")
    if q is None or q.shape[0] != n or (minmax is not None and minmax.shape[0] != n) or \
            (rescore_row is not None and rescore_row.shape[0] != n):
        # the ABI indexes q / minmax / rescore_row by candidate row and cannot see their lengths
        raise N.VrqNativeError(f"search2: {n} code rows but {None if q is None else q.shape[0]} stored rows")
    lib = N.load()
    call = N.SearchCall("vrq_search2", K, flags, allow, engine, "search2", query_set=query_set)
    if flags and call.name != "vrq_search2":  # the counting scan takes no scan flags
        why = f"engine={engine!r}" if call.engine is not None else \
            "a row filter" if allow is not None else f"K = {K} > {N.VRQ_K_MAX}"
        raise N.VrqNativeError(f"search2: flags {flags} with {why} ({call.name} takes none)")
    allow, query_set = checked_filter(allow, query_set, n, nq, dev)
    count = torch.empty((nq,), dtype=torch.int32, device=dev)
    ws = call.workspace(lib, n, d, nq, K, dev)
    with torch.cuda.device(dev):
        call(lib, (_SEARCH2_MODES[mode], N.ptr(codes), N.ptr(q), N.ptr(minmax), float(limit), N.ptr(rescore_row), n,
                   d, 0, N.ptr(qf), N.ptr(qb), nq, kk, K, flags),
             (N.ptr(count), N.ptr(rows), N.ptr(dist), N.ptr(score)), allow, ws, dev, f"{call.name}({mode})",
             query_set=query_set)
    return rows, dist, score


def merge_shards2(cnt, rows, dist, score, k: int):
    """``vrq_merge_shards2`` (``vrq_merge_shards2_large`` for K > 1024) on the stacked [S, nq, K] outputs of
    ``vrq_shard_search2`` (``cnt`` [S, nq]) ->
    (count, rows, dist, score, src): the two-phase result of the whole corpus, ``src`` = shard * K + position
    of each result in the stacked inputs (-1 for padding)."""
    S, nq, K = rows.shape
    dev = rows.device
    oc = torch.empty((nq,), dtype=torch.int32, device=dev)
    orow = torch.empty((nq, k), dtype=torch.int64, device=dev)
    od = torch.empty((nq, k), dtype=torch.int32, device=dev)
    osc = torch.empty((nq, k), dtype=torch.float64, device=dev)
    src = torch.empty((nq, k), dtype=torch.int32, device=dev)
    cnt, rows, dist, score = (t.contiguous() for t in (cnt, rows, dist, score))  # held until the launch returns
    lib = N.load()
    # more than 1024 candidates per shard: vrq_merge_shards2_large, which takes a workspace
    large = N.large_k(K, "merge_shards2")
    name = "vrq_merge_shards2_large" if large else "vrq_merge_shards2"
    extra = ()
    with torch.cuda.device(dev):
        if large:
            ws = torch.empty((max(8, lib.vrq_merge_shards_large_workspace_size(S, nq, K)),), dtype=torch.uint8,
                             device=dev)
            extra = (N.ptr(ws), ws.numel())
        rc = getattr(lib, name)(S, nq, K, N.ptr(cnt), N.ptr(rows), N.ptr(dist), N.ptr(score), k, N.ptr(oc),
                                N.ptr(orow), N.ptr(od), N.ptr(osc), N.ptr(src), *extra, N.stream_handle(dev))
    N.check(rc, name)
    return oc, orow, od, osc, src


def int8_row_norms(x8: torch.Tensor) -> torch.Tensor:
    """float64 ``np.linalg.norm`` of every int8 row (``CohereEnhancedVectorDB.py:308``)."""
    x8 = x8.contiguous()
    n, d = x8.shape
    out = torch.empty((n,), dtype=torch.float64, device=x8.device)
    lib = N.load()
    with torch.cuda.device(x8.device):
        rc = lib.vrq_int8_row_norms(N.ptr(x8), n, d, N.ptr(out), N.stream_handle(x8.device))
    N.check(rc, "vrq_int8_row_norms")
    return out


def _host(x: torch.Tensor, one: bool):
    a = x.cpu().numpy()
    return a[0] if one else a


def _to_binary(embedding, mode="int8g"):
    one = np.ndim(embedding) == 1
    return _host(encode(mode, embedding, 1.0)["codes"], one)


class _Binary:
    @staticmethod
    def _to_binary(embedding):
        """packbits(embedding > np.mean(embedding)) (MSB-first)."""
        return _to_binary(embedding, "int8g")


class VectorDBInt8Global(_Binary):
    @staticmethod
    def _quantize_to_int8(embedding, limit: float):
        one = np.ndim(embedding) == 1
        return _host(encode("int8g", embedding, limit)["q"], one)

    @staticmethod
    def _dequantize_int8(emb_int8, limit: float):
        """``VectorDBInt8Global.py:144-152``: int8 * float32(limit/127) (on the device)."""
        one = np.ndim(emb_int8) == 1
        return _host(dequantize("int8g", emb_int8, limit=limit), one)


class VectorDBInt16Global(_Binary):
    @staticmethod
    def _quantize_to_int16(embedding, limit: float):
        one = np.ndim(embedding) == 1
        return _host(encode("int16g", embedding, limit)["q"], one)

    @staticmethod
    def _dequantize_int16(emb_int16, limit: float):
        """``VectorDBInt16Global.py:144-152`` (on the device)."""
        one = np.ndim(emb_int16) == 1
        return _host(dequantize("int16g", emb_int16, limit=limit), one)


class VectorDBInt4Global(_Binary):
    @staticmethod
    def _quantize_to_int4(embedding, limit: float):
        """Reproduces the reference: ``limit`` is ignored (per-vector 7/max|x| scale)."""
        one = np.ndim(embedding) == 1
        return _host(encode("int4g", embedding, 1.0)["q"], one)

    @staticmethod
    def _dequantize_int4(q_packed, length: int, limit: float):
        """``VectorDBInt4Global.py:166-188`` (on the device)."""
        one = np.ndim(q_packed) == 1
        return _host(dequantize("int4g", np.asarray(q_packed).astype(np.int8), limit=limit, dim=length), one)


class VectorDBInt8(_Binary):
    @staticmethod
    def _quantize_to_int8(embedding):
        one = np.ndim(embedding) == 1
        r = encode("int8", embedding)
        q, mm = _host(r["q"], one), r["minmax"].cpu().numpy()
        if one:
            return q, np.float32(mm[0, 0]), np.float32(mm[0, 1])
        return q, mm.astype(np.float32)[:, 0], mm.astype(np.float32)[:, 1]

    @staticmethod
    def _dequantize_int8(emb_int8, min_max):
        """``VectorDBInt8.py:129-138`` (on the device); min_max = (min, max) or an [n, 2] array."""
        one = np.ndim(emb_int8) == 1
        return _host(dequantize("int8", emb_int8, minmax=np.asarray(min_max, np.float64)), one)


class VectorDBInt4(_Binary):
    @staticmethod
    def _quantize_to_int4(embedding):
        one = np.ndim(embedding) == 1
        r = encode("int4", embedding)
        q, mm = _host(r["q"], one), r["minmax"].cpu().numpy()
        if one:
            return q, float(mm[0, 0]), float(mm[0, 1])
        return q, mm[:, 0], mm[:, 1]

    @staticmethod
    def _dequantize_int4(q_packed, length: int, min_max):
        """``VectorDBInt4.py:157-184`` (on the device)."""
        one = np.ndim(q_packed) == 1
        return _host(dequantize("int4", np.asarray(q_packed).astype(np.int8), minmax=np.asarray(min_max, np.float64),
                                dim=length), one)


class VectorDBInt16:
    @staticmethod
    def _to_binary(embedding):
        """``VectorDBInt16.py:148-157``: packbits(int16 > float64 mean)."""
        return _to_binary(embedding, "bin16")
