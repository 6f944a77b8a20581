"""Row-sharded search over several MI355X (one process per GPU): the three-phase search
(``ShardedSearch``) and the two-phase search of the ``CohereVectorDBBinary`` / ``VectorDBInt*``
classes (``ShardedSearch2``), at every embedding dim of ``vrq_dim_supported``.

The reference is single-process; sharding is this
build's only scaling axis.  Rank r owns a contiguous global row range
``[row0, row0 + m)`` (codes, int8 rows, norms, external ids).  A query batch is
replicated to every rank and searched in three steps:

1. local ``vrq_shard_search3`` (at 1024 dims: ``vrq_search3`` in ``VRQ_SEARCH_SHARD``
   mode): the shard's exact top-K
   (K = the GLOBAL ``binary_k``, because the global top-K may sit in one shard)
   by (dist, global row), each with its Phase-II and Phase-III score;
2. ONE ``all_gather_into_tensor`` (RCCL over xGMI with the ``nccl`` backend) of
   the packed candidate tuples -- ``nq * K * 36`` bytes per rank (3.7 MB at
   nq = 1024, K = 100: latency-bound, one collective per batch);
3. ``vrq_merge_shards`` on every rank: global top-K by (dist, global row) ->
   stable sort by s2 -> first K3 -> stable sort by s3 -> first k, which is
   exactly the single-index semantics of ``CohereEnhancedVectorDB.py:267-322``,
   so results are identical for 1/2/4/8 ranks.

``ShardedSearch2`` is the same three steps with one score per candidate: ``vrq_shard_search2``,
one all-gather of 28-byte records, ``vrq_merge_shards2`` (global top-K -> stable sort by score ->
first k: ``CohereVectorDBBinary.py:215-239``, ``VectorDBInt8Global.py:224-252``).

More than 1024 Phase-I candidates (``k * binary_oversample`` up to ``VRQ_K_LARGE_MAX`` = 8192; the default
oversample of 10 passes 1024 at k = 103) take the same three steps through ``vrq_shard_search3_large`` /
``vrq_shard_search2_large`` (the counting scan K1h, every candidate scored) and ``vrq_merge_shards_large`` /
``vrq_merge_shards2_large``; ``shard_calls(K)`` names the calls of a K.  Packing and the all-gather are the
same, and their size is what it is: ``nq * K * 36`` B per rank for the three-phase search and ``nq * K * 28`` B
for the two-phase one -- 18.9 MB per rank at nq = 64, K = 8192, linear in nq -- so a large K is a small-batch
regime, as K1h itself is.  (Exchanging per-shard distance histograms first, so that each shard scores and
sends only its share of the global K, is the recorded follow-up: DESIGN section 10.)

Not sharded: ``mode="bin16"`` (``VectorDBInt16`` ranks by Phase I alone), a ``rescore_row`` that
crosses shards (an id added twice must live in one shard), class-level ``add_documents``, and
``CohereVectorDBFloat`` (``merge_topk_shards`` covers the exhaustive paths through ``row_offset``).
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _native as N
from .enhanced import SearchBatch
from .quant import _SEARCH2_MODES, merge_shards2

# packed per-candidate record: row i64 | doc id i64 | s2 f64 | s3 f64 | dist i32  (36 B)
_REC = 36


def pack_candidates(count: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, dist_: torch.Tensor,
                    s2: torch.Tensor, s3: torch.Tensor) -> torch.Tensor:
    """Pack one rank's [nq, K] candidate tuples (+ counts) into a flat uint8 buffer."""
    nq, K = rows.shape
    parts = [count.to(torch.int32).contiguous().view(torch.uint8).reshape(-1),
             rows.contiguous().view(torch.uint8).reshape(-1),
             ids.contiguous().view(torch.uint8).reshape(-1),
             s2.contiguous().view(torch.uint8).reshape(-1),
             s3.contiguous().view(torch.uint8).reshape(-1),
             dist_.to(torch.int32).contiguous().view(torch.uint8).reshape(-1)]
    return torch.cat(parts)


def unpack_candidates(buf: torch.Tensor, S: int, nq: int, K: int):
    """Inverse of ``pack_candidates`` for S stacked ranks -> [S, nq(, K)] views."""
    b = buf.reshape(S, -1)
    o = 0

    def take(nbytes, dtype, shape):
        nonlocal o
        t = b[:, o:o + nbytes].contiguous().view(dtype).reshape(S, *shape)
        o += nbytes
        return t

    cnt = take(4 * nq, torch.int32, (nq,))
    rows = take(8 * nq * K, torch.int64, (nq, K))
    ids = take(8 * nq * K, torch.int64, (nq, K))
    s2 = take(8 * nq * K, torch.float64, (nq, K))
    s3 = take(8 * nq * K, torch.float64, (nq, K))
    d = take(4 * nq * K, torch.int32, (nq, K))
    return cnt, rows, ids, d, s2, s3


def gather_candidates(local: torch.Tensor, group=None) -> torch.Tensor:
    """All-gather the packed buffers of every rank (single collective).  With the ``nccl`` backend
    (RCCL) device buffers travel GPU to GPU; a ``gloo`` group (CPU tests, several ranks sharing one
    GPU) stages the device buffer through host memory."""
    world = dist.get_world_size(group)
    stage = local.is_cuda and dist.get_backend(group) == "gloo"
    src = local.cpu() if stage else local
    out = torch.empty((world * src.numel(),), dtype=src.dtype, device=src.device)
    dist.all_gather_into_tensor(out, src, group=group)
    return out.to(local.device) if stage else out


# packed per-candidate record of the two-phase search: row i64 | doc id i64 | score f64 | dist i32  (28 B)
_REC2 = 28


def pack_candidates2(count: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, dist_: torch.Tensor,
                     score: torch.Tensor) -> torch.Tensor:
    """``pack_candidates`` for the one-score candidates of ``vrq_shard_search2``."""
    parts = [count.to(torch.int32).contiguous().view(torch.uint8).reshape(-1),
             rows.contiguous().view(torch.uint8).reshape(-1),
             ids.contiguous().view(torch.uint8).reshape(-1),
             score.contiguous().view(torch.uint8).reshape(-1),
             dist_.to(torch.int32).contiguous().view(torch.uint8).reshape(-1)]
    return torch.cat(parts)


def unpack_candidates2(buf: torch.Tensor, S: int, nq: int, K: int):
    """Inverse of ``pack_candidates2`` for S stacked ranks -> (count, rows, ids, dist, score) [S, nq(, K)]."""
    b = buf.reshape(S, 4 * nq + _REC2 * nq * K)
    o = 0

    def take(nbytes, dtype, shape):
        nonlocal o
        t = b[:, o:o + nbytes].contiguous().view(dtype).reshape(S, *shape)
        o += nbytes
        return t

    cnt = take(4 * nq, torch.int32, (nq,))
    rows = take(8 * nq * K, torch.int64, (nq, K))
    ids = take(8 * nq * K, torch.int64, (nq, K))
    sc = take(8 * nq * K, torch.float64, (nq, K))
    d = take(4 * nq * K, torch.int32, (nq, K))
    return cnt, rows, ids, d, sc


def shard_calls(K: int, flags: int = 0) -> dict:
    """The entry points a sharded search with K Phase-I candidates takes: today's calls up to 1024, the
    ``_large`` calls (the counting scan K1h + the large merge) for 1024 < K <= ``VRQ_K_LARGE_MAX``; each
    search call's workspace size is ``<name>_workspace_size``, the large merges share
    ``vrq_merge_shards_large_workspace_size``.  Raises past the limit, and for scan flags with a large K."""
    large = N.large_k(K, "sharded search")
    if large and flags:
        raise N.VrqNativeError(f"sharded search: flags {flags} with K = {K} > {N.VRQ_K_MAX} "
                               "(the _large calls take none)")
    sfx = "_large" if large else ""
    return {"search3": "vrq_shard_search3" + sfx, "search2": "vrq_shard_search2" + sfx,
            "merge3": "vrq_merge_shards" + sfx, "merge2": "vrq_merge_shards2" + sfx}


def _merge_workspace(lib, name: str, S: int, nq: int, K: int, dev):
    """The extra (workspace, bytes) arguments of a merge call: none for the K <= 1024 merges."""
    if not name.endswith("_large"):
        return (), None
    need = lib.vrq_merge_shards_large_workspace_size(S, nq, K) if nq and K else 0
    if nq and K and need == 0:
        raise N.VrqNativeError(f"{name}: unsupported shape shards={S} nq={nq} K={K}")
    ws = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev)
    return (N.ptr(ws), ws.numel()), ws


def _workspace(ws, kind: str, n: int, qf: torch.Tensor, K: int, dev):
    """``ws`` if it holds the shard call (``kind``: "search3" / "search2") of this shape, else a new buffer
    that does."""
    size_fn = getattr(N.load(), shard_calls(K)[kind] + "_workspace_size")
    need = size_fn(n, qf.shape[1], qf.shape[0], K) if n and K and qf.shape[0] else 0
    if n and K and qf.shape[0] and need == 0:
        raise N.VrqNativeError(f"sharded search: unsupported shape n={n} dim={qf.shape[1]} nq={qf.shape[0]} K={K} "
                               "(dims: vrq_dim_supported)")
    if ws is None or ws.numel() < need:
        ws = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev)
    return ws


def _local_ids(ids: torch.Tensor, rows: torch.Tensor, row0: int) -> torch.Tensor:
    """External ids of a shard's global candidate rows (padding stays -1; no id table: the row)."""
    loc = (rows - row0).clamp_min(0)
    return torch.where(rows >= 0, ids[loc] if ids.numel() else rows, rows)


def shard_search3(codes: torch.Tensor, x8: torch.Tensor, norms: torch.Tensor, qf: torch.Tensor, qb: torch.Tensor,
                  K: int, flags: int = 0, row_offset: int = 0, rescore_row: torch.Tensor | None = None,
                  workspace: torch.Tensor | None = None):
    """Thin wrapper of ``vrq_shard_search3`` (every dim of ``vrq_dim_supported``): one shard's exact Phase-I
    top-K in (dist, row) order with both scores; returns (count, rows, dist, s2, s3) device tensors [nq, K]."""
    dev = qf.device
    nq, dim = qf.shape
    n = codes.shape[0]
    if n and (x8.shape[0] != n or norms.shape[0] != n):
        # the ABI indexes x8 / norms by code row and cannot see their lengths
        raise N.VrqNativeError(f"vrq_shard_search3: {n} code rows but {x8.shape[0]} int8 rows and "
                               f"{norms.shape[0]} norms")
    if rescore_row is not None and rescore_row.shape[0] != n:
        raise N.VrqNativeError(f"vrq_shard_search3: rescore_row has {rescore_row.shape[0]} entries for {n} rows")
    if n and (codes.shape[1] * 8 != dim or qb.shape != (nq, dim // 8) or x8.shape[1] != dim):
        raise N.VrqNativeError(f"vrq_shard_search3: {codes.shape[1]}-byte codes but queries of dim {dim} / codes "
                               f"{tuple(qb.shape)}, int8 rows of dim {x8.shape[1]}")
    lib = N.load()
    name = shard_calls(K, flags)["search3"]
    workspace = _workspace(workspace, "search3", n, qf, K, dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, K), dtype=torch.int64, device=dev)
    dist_ = torch.empty((nq, K), dtype=torch.int32, device=dev)
    s2 = torch.empty((nq, K), dtype=torch.float64, device=dev)
    s3 = torch.empty((nq, K), dtype=torch.float64, device=dev)
    rc = getattr(lib, name)(N.ptr(codes) if n else 0, N.ptr(x8) if n else 0, N.ptr(norms) if n else 0,
                            N.ptr(rescore_row), n, dim, row_offset, N.ptr(qf), N.ptr(qb), nq, K, flags,
                            N.ptr(cnt), N.ptr(rows), N.ptr(dist_), N.ptr(s2), N.ptr(s3), N.ptr(workspace),
                            workspace.numel(), N.stream_handle(dev))
    N.check(rc, name)
    return cnt, rows, dist_, s2, s3


def shard_search2(mode: str, codes: torch.Tensor, q: torch.Tensor, qf: torch.Tensor, qb: torch.Tensor, K: int,
                  minmax: torch.Tensor | None = None, limit: float = 0.0, flags: int = 0, row_offset: int = 0,
                  rescore_row: torch.Tensor | None = None, workspace: torch.Tensor | None = None):
    """Thin wrapper of ``vrq_shard_search2``: one shard's exact Phase-I top-K in (dist, row) order with the
    rescoring score of ``mode`` (a ``quant.search2`` mode name); returns (count, rows, dist, score) [nq, K]."""
    if mode not in _SEARCH2_MODES:
        raise ValueError(f"unknown search2 mode {mode!r}")
    dev = qf.device
    nq, dim = qf.shape
    n = codes.shape[0]
    if n and (codes.shape[1] * 8 != dim or qb.shape != (nq, dim // 8)):
        raise N.VrqNativeError(f"vrq_shard_search2: {codes.shape[1]}-byte codes but queries of dim {dim} / codes "
                               f"{tuple(qb.shape)}")
    if n and (q is None or q.shape[0] != n or (minmax is not None and minmax.shape[0] != n) or
              (rescore_row is not None and rescore_row.shape[0] != n)):
        # the ABI indexes q / minmax / rescore_row by candidate row and cannot see their lengths
        raise N.VrqNativeError(f"vrq_shard_search2: {n} code rows but {None if q is None else q.shape[0]} stored rows")
    lib = N.load()
    name = shard_calls(K, flags)["search2"]
    workspace = _workspace(workspace, "search2", n, qf, K, dev)
    cnt = torch.empty((nq,), dtype=torch.int32, device=dev)
    rows = torch.empty((nq, K), dtype=torch.int64, device=dev)
    dist_ = torch.empty((nq, K), dtype=torch.int32, device=dev)
    score = torch.empty((nq, K), dtype=torch.float64, device=dev)
    rc = getattr(lib, name)(_SEARCH2_MODES[mode], N.ptr(codes) if n else 0, N.ptr(q) if n else 0,
                            N.ptr(minmax) if n else 0, float(limit), N.ptr(rescore_row), n, dim, row_offset,
                            N.ptr(qf), N.ptr(qb), nq, K, flags, N.ptr(cnt), N.ptr(rows), N.ptr(dist_),
                            N.ptr(score), N.ptr(workspace), workspace.numel(), N.stream_handle(dev))
    N.check(rc, f"{name}({mode})")
    return cnt, rows, dist_, score


def merge_shards(cnt, rows, d, s2, s3, k: int, K3: int):
    """``vrq_merge_shards`` (``vrq_merge_shards_large`` for K > 1024) on stacked [S, nq, K] tensors ->
    (count, rows, dist, s2, s3, src)."""
    S, nq, K = rows.shape
    dev = rows.device
    oc = torch.empty((nq,), dtype=torch.int32, device=dev)
    orow = torch.empty((nq, k), dtype=torch.int64, device=dev)
    od = torch.empty((nq, k), dtype=torch.int32, device=dev)
    o2 = torch.empty((nq, k), dtype=torch.float64, device=dev)
    o3 = torch.empty((nq, k), dtype=torch.float64, device=dev)
    src = torch.empty((nq, k), dtype=torch.int32, device=dev)
    cnt, rows, d, s2, s3 = (t.contiguous() for t in (cnt, rows, d, s2, s3))  # held until the launch returns
    lib = N.load()
    name = shard_calls(K)["merge3"]
    with torch.cuda.device(dev):
        extra, ws = _merge_workspace(lib, name, S, nq, K, dev)  # (stream-ordered: freed after the launches)
        rc = getattr(lib, name)(S, nq, K, N.ptr(cnt), N.ptr(rows), N.ptr(d), N.ptr(s2), N.ptr(s3), k, K3,
                                N.ptr(oc), N.ptr(orow), N.ptr(od), N.ptr(o2), N.ptr(o3), N.ptr(src), *extra,
                                N.stream_handle(dev))
    N.check(rc, name)
    return oc, orow, od, o2, o3, src


def merge_topk_shards(rows: torch.Tensor, scores: torch.Tensor, k: int):
    """Merge of row-sharded ``vrq_gemm_topk`` outputs (config 5) after the all-gather.

    ``rows``/``scores`` are [S, nq, k] (global rows; -1 / NaN padding).  Result: (count, rows,
    scores) of the global top-k in the reference's (score desc, row asc) order, identical to one
    call over the whole corpus.  Two stable sorts: by row (padding last), then by score descending
    (-0.0 equal to +0.0 and padding equal to -inf, both as in Python's sort; padding stays behind
    real -inf rows because it is last in row order)."""
    S, nq, kk = rows.shape
    r = rows.permute(1, 0, 2).reshape(nq, S * kk)
    sc = scores.permute(1, 0, 2).reshape(nq, S * kk)
    o = torch.sort(torch.where(r >= 0, r, torch.full_like(r, torch.iinfo(torch.int64).max)), dim=1,
                   stable=True).indices
    r, sc = torch.gather(r, 1, o), torch.gather(sc, 1, o)
    key = torch.where(r >= 0, sc, torch.full_like(sc, float("-inf"))) + 0.0  # + 0.0 maps -0.0 to +0.0
    o = torch.sort(-key, dim=1, stable=True).indices[:, :k]
    r, sc = torch.gather(r, 1, o), torch.gather(sc, 1, o)
    return (r >= 0).sum(1).to(torch.int32), r, sc


def gather_topk(rows: torch.Tensor, scores: torch.Tensor, group=None):
    """One all-gather of a rank's [nq, k] (rows i64, scores f64) -> stacked [S, nq, k] each."""
    S = dist.get_world_size(group)
    buf = torch.cat([rows.contiguous().view(torch.uint8).reshape(-1), scores.contiguous().view(torch.uint8).reshape(-1)])
    out = gather_candidates(buf, group).reshape(S, -1)
    h = rows.numel() * 8
    return (out[:, :h].contiguous().view(torch.int64).reshape(S, *rows.shape),
            out[:, h:].contiguous().view(torch.float64).reshape(S, *scores.shape))


class ShardedSearch:
    """One rank's shard of a row-sharded corpus + the collective search."""

    def __init__(self, codes: torch.Tensor, x8: torch.Tensor, norms: torch.Tensor, ids: torch.Tensor,
                 row0: int, n_total: int, group=None):
        self.codes, self.x8, self.norms, self.ids = codes, x8, norms, ids
        self.row0, self.n_total, self.group = int(row0), int(n_total), group
        self.device = codes.device
        self._ws = None

    def local(self, qf, qb, k, binary_oversample, int8_oversample):
        K = min(k * binary_oversample, self.n_total)
        self._ws = _workspace(self._ws, "search3", self.codes.shape[0], qf, K, self.device)
        with torch.cuda.device(self.device):
            cnt, rows, d, s2, s3 = shard_search3(self.codes, self.x8, self.norms, qf, qb, K, 0, self.row0, None,
                                                 self._ws)
        return K, cnt, rows, _local_ids(self.ids, rows, self.row0), d, s2, s3

    def search_vectors(self, qf, qb, k: int = 10, binary_oversample: int = 10,
                       int8_oversample: int = 3) -> SearchBatch:
        K, cnt, rows, ids, d, s2, s3 = self.local(qf, qb, k, binary_oversample, int8_oversample)
        nq = qf.shape[0]
        S = dist.get_world_size(self.group)
        allb = gather_candidates(pack_candidates(cnt, rows, ids, d, s2, s3), self.group)
        gc, gr, gi, gd, g2, g3 = unpack_candidates(allb, S, nq, K)
        oc, orow, od, o2, o3, src = merge_shards(gc, gr, gd, g2, g3, k, k * int8_oversample)
        flat_ids = gi.permute(1, 0, 2).reshape(nq, S * K)  # [nq, S*K] in (shard, pos) order
        oid = torch.where(src >= 0, torch.gather(flat_ids, 1, src.clamp_min(0).to(torch.int64)),
                          torch.full_like(orow, -1))
        return SearchBatch(oc, oid, orow, od, o2, o3)


class ShardedSearch2:
    """One rank's shard of a row-sharded two-phase corpus (``CohereVectorDBBinary``, ``VectorDBInt*``,
    ``CohereVectorDBInt8``) + the collective search.  ``mode`` is a ``quant.search2`` rescoring mode
    (``int8g`` ... ``int4``, ``f32``, ``sbin``), ``q`` the shard's stored rows of that mode (for ``sbin``
    normally ``codes`` itself), ``minmax`` / ``limit`` as there."""

    def __init__(self, mode: str, codes: torch.Tensor, q: torch.Tensor, ids: torch.Tensor, row0: int, n_total: int,
                 minmax: torch.Tensor | None = None, limit: float = 0.0, group=None):
        if mode not in _SEARCH2_MODES:
            raise ValueError(f"unknown search2 mode {mode!r}")
        self.mode, self.codes, self.q, self.ids = mode, codes, q, ids
        self.minmax, self.limit = minmax, float(limit)
        self.row0, self.n_total, self.group = int(row0), int(n_total), group
        self.device = codes.device
        self._ws = None

    def local(self, qf, qb, k, binary_oversample):
        K = min(k * binary_oversample, self.n_total)
        self._ws = _workspace(self._ws, "search2", self.codes.shape[0], qf, K, self.device)
        with torch.cuda.device(self.device):
            cnt, rows, d, sc = shard_search2(self.mode, self.codes, self.q, qf, qb, K, self.minmax, self.limit, 0,
                                             self.row0, None, self._ws)
        return K, cnt, rows, _local_ids(self.ids, rows, self.row0), d, sc

    def search_vectors(self, qf, qb, k: int = 10, binary_oversample: int = 10):
        """-> (count i32[nq], ids i64[nq, k], rows i64[nq, k], dist i32[nq, k], score f64[nq, k]), equal to
        ``quant.search2`` over the whole corpus (padding -1 / INT32_MAX / NaN)."""
        K, cnt, rows, ids, d, sc = self.local(qf, qb, k, binary_oversample)
        nq = qf.shape[0]
        S = dist.get_world_size(self.group)
        allb = gather_candidates(pack_candidates2(cnt, rows, ids, d, sc), self.group)
        gc, gr, gi, gd, gs = unpack_candidates2(allb, S, nq, K)
        oc, orow, od, osc, src = merge_shards2(gc, gr, gd, gs, k)
        flat_ids = gi.permute(1, 0, 2).reshape(nq, S * K)  # [nq, S*K] in (shard, pos) order
        oid = torch.where(src >= 0, torch.gather(flat_ids, 1, src.clamp_min(0).to(torch.int64)),
                          torch.full_like(orow, -1))
        return oc, oid, orow, od, osc
