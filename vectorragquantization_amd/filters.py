"""Row allow-bitmaps for the filtered searches (``vrq_*_filtered``, ``vrq_*_perquery``; ``allow=`` of the wrappers).

A bitmap is an int64 tensor of ``ceil(n / 64)`` words: row ``r`` takes part in Phase I iff bit ``r & 63`` of
word ``r >> 6`` is set -- the bytes of FAISS's ``IDSelectorBitmap`` and of
``np.packbits(mask, bitorder="little")``.  Bits past ``n`` in the last word are ignored by the kernels (the
helpers here leave them 0).  Only torch ops: the helpers run wherever their input lives, CPU included.

A batch whose queries carry different filters takes a bitmap per distinct filter, int64 ``[S, words]``
(``row_bitmaps`` / ``ids_bitmaps``), and an int32 ``query_set`` of one set id per query: ``-1`` for an unfiltered
query, any other id outside ``[0, S)`` for a query that may see no row.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N


def words(n: int) -> int:
    """Words of a bitmap over n rows."""
    return (n + 63) >> 6


def row_bitmap(mask: torch.Tensor) -> torch.Tensor:
    """bool[n] (True: the row is allowed) -> int64[ceil(n / 64)] on the mask's device."""
    mask = mask.reshape(-1)
    n = mask.shape[0]
    bits = torch.zeros((words(n) * 64,), dtype=torch.uint8, device=mask.device)
    bits[:n] = mask.to(torch.bool)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=mask.device)
    by = (bits.view(words(n) * 8, 8) * w).sum(dim=1, dtype=torch.uint8)   # byte b holds rows 8 b ... 8 b + 7, low bit first
    return by.view(torch.int64)                                 # 8 bytes = one little-endian word


def ids_bitmap(id_map: torch.Tensor, allowed_ids) -> torch.Tensor:
    """The bitmap of the rows of ``id_map`` (i64[n], external id per row) that carry one of ``allowed_ids``:
    every row of a duplicated id is allowed, ids that no row carries are ignored."""
    if isinstance(allowed_ids, torch.Tensor):
        a = allowed_ids.to(device=id_map.device, dtype=torch.int64).reshape(-1)
    else:
        a = torch.from_numpy(np.array(list(allowed_ids), dtype=np.int64).reshape(-1)).to(id_map.device)
    return row_bitmap(torch.isin(id_map, a))


def checked(allow: torch.Tensor, n: int, device) -> torch.Tensor:
    """``allow`` as the ABI wants it (contiguous int64[ceil(n / 64)] on ``device``); raises otherwise, since
    the kernels cannot see its length."""
    if not isinstance(allow, torch.Tensor) or allow.dtype != torch.int64 or allow.dim() != 1 or \
            allow.shape[0] != words(n):
        raise N.VrqNativeError(f"allow must be an int64 tensor of {words(n)} words for {n} rows (filters.row_bitmap)")
    if allow.device != torch.device(device):
        raise N.VrqNativeError(f"allow is on {allow.device}, the index on {device}")
    return allow.contiguous()


def row_bitmaps(masks: torch.Tensor) -> torch.Tensor:
    """bool[S, n] (one mask per set) -> int64[S, ceil(n / 64)] on the masks' device; row s is ``row_bitmap(masks[s])``."""
    if masks.dim() != 2:
        raise N.VrqNativeError(f"row_bitmaps takes bool[S, n] masks, got {masks.dim()} dimension(s)")
    S, n = masks.shape
    bits = torch.zeros((S, words(n) * 64), dtype=torch.uint8, device=masks.device)
    bits[:, :n] = masks.to(torch.bool)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=masks.device)
    by = (bits.view(S, words(n) * 8, 8) * w).sum(dim=2, dtype=torch.uint8)
    return by.contiguous().view(torch.int64).view(S, words(n))


def _id_tuple(ids) -> tuple:
    if isinstance(ids, torch.Tensor):
        ids = ids.reshape(-1).tolist()
    return tuple(sorted({int(i) for i in ids}))


def ids_bitmaps(id_map: torch.Tensor, id_collections):
    """One entry per query, each ``None`` (unfiltered) or a collection of external ids ->
    (allow int64[S, words], query_set int32[nq]) on ``id_map``'s device.  ``None`` becomes set ``-1``; equal
    collections share a set; an empty collection, or one of ids no row carries, gets an all-zero bitmap.  With no
    collection at all S is 1 (an all-zero bitmap no query names): the ABI wants at least one set."""
    sets, ids = {}, []
    for c in id_collections:
        ids.append(-1 if c is None else sets.setdefault(_id_tuple(c), len(sets)))
    n = id_map.shape[0]
    masks = torch.zeros((max(1, len(sets)), n), dtype=torch.bool, device=id_map.device)
    for key, s in sets.items():
        masks[s] = torch.isin(id_map, torch.tensor(key, dtype=torch.int64, device=id_map.device))
    return row_bitmaps(masks), torch.tensor(ids, dtype=torch.int32, device=id_map.device)


def checked_sets(allow: torch.Tensor, query_set: torch.Tensor, n: int, nq: int, device):
    """``(allow, query_set)`` as the per-query calls want them: int64 ``[S >= 1, >= words(n)]`` whose rows are
    contiguous, and an integer tensor of ``nq`` set ids (returned as contiguous int32), both on ``device``; raises
    otherwise, since the kernels cannot see their lengths."""
    if not isinstance(allow, torch.Tensor) or allow.dtype != torch.int64 or allow.dim() != 2 or \
            allow.shape[0] < 1 or allow.shape[1] < words(n):
        raise N.VrqNativeError(f"allow must be an int64 tensor [S >= 1, >= {words(n)} words] for {n} rows "
                               "(filters.row_bitmaps)")
    if not isinstance(query_set, torch.Tensor) or query_set.dim() != 1 or query_set.shape[0] != nq or \
            query_set.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64):
        raise N.VrqNativeError(f"query_set must be an integer tensor of {nq} set ids, one per query")
    dev = torch.device(device)
    if allow.device != dev or query_set.device != dev:
        raise N.VrqNativeError(f"allow is on {allow.device}, query_set on {query_set.device}, the index on {device}")
    if allow.stride(1) != 1 or (allow.shape[0] > 1 and allow.stride(0) < allow.shape[1]):
        allow = allow.contiguous()
    return allow, query_set.to(torch.int32).contiguous()


def checked_filter(allow, query_set, n: int, nq: int, device):
    """What a wrapper hands to its ``SearchCall``: ``(checked(allow), None)`` for a 1-D bitmap (or ``(None, None)``
    without one), ``checked_sets(allow, query_set)`` with a ``query_set``."""
    if query_set is not None:
        return checked_sets(allow, query_set, n, nq, device)
    return (checked(allow, n, device) if allow is not None else None), None


def class_filter(id_map: torch.Tensor, allowed_ids, allowed_ids_per_query, nq: int):
    """The ``(allow, query_set)`` of a class's ``search_vectors``: ``allowed_ids`` (one collection for the whole
    batch) -> a 1-D bitmap and None; ``allowed_ids_per_query`` (a sequence of ``nq`` entries, each None or a
    collection of ids) -> ``ids_bitmaps``; neither -> ``(None, None)``.  Raises for both at once, and for a
    sequence whose length is not the batch's."""
    if allowed_ids_per_query is None:
        return (ids_bitmap(id_map, allowed_ids) if allowed_ids is not None else None), None
    if allowed_ids is not None:
        raise N.VrqNativeError("allowed_ids and allowed_ids_per_query are exclusive")
    entries = list(allowed_ids_per_query)
    if len(entries) != nq:
        raise N.VrqNativeError(f"allowed_ids_per_query has {len(entries)} entries for {nq} queries")
    return ids_bitmaps(id_map, entries)
