"""Row allow-bitmaps for the filtered searches (``vrq_*_filtered``; ``allow=`` of the wrappers).

A bitmap is an int64 tensor of ``ceil(n / 64)`` words: row ``r`` takes part in Phase I iff bit ``r & 63`` of
word ``r >> 6`` is set -- the bytes of FAISS's ``IDSelectorBitmap`` and of
``np.packbits(mask, bitorder="little")``.  Bits past ``n`` in the last word are ignored by the kernels (the
helpers here leave them 0).  Only torch ops: the helpers run wherever their input lives, CPU included.
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
