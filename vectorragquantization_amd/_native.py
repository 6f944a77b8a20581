"""ctypes binding of libvrq.so (include/vrq.h).

The product path has no CPU fallback: if the HIP library is missing or cannot
be loaded, every call raises ``VrqNativeError`` -- tests on a GPU box therefore
fail loudly instead of silently running something else.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import _build

VRQ_OK = 0
VRQ_EINVAL = -1
VRQ_EHIP = -2
VRQ_EUNSUPPORTED = -3
VRQ_EWORKSPACE = -4

VRQ_SEARCH_PHASE1_ONLY = 1
VRQ_SEARCH_SHARD = 2
VRQ_SEARCH_SCAN_VALU = 4
VRQ_SEARCH_SCAN_MFMA = 8
VRQ_SCAN_STAGE_PREFIX = 16
VRQ_SCAN_STAGE_MATRIX = 32
VRQ_SCAN_STAGE_SUFFIX = 64
VRQ_SCAN_STAGE_RECHECK = 128
VRQ_GEMM_BINARY = 2
VRQ_GEMM_INT8_COSINE = 3
VRQ_GEMM_FLOAT_IP = 4
VRQ_GEMM_STAGE_SAMPLE = 16
VRQ_GEMM_STAGE_MAIN = 32
VRQ_GEMM_STAGE_FINISH = 64
VRQ_GEMM_NO_FALLBACK = 128
VRQ_GEMM_SCAN_EXACT = 256  # _dim entry points: the exact exhaustive scan (K5d) at dim 1024 too
VRQ_RESCORE_F32 = 16  # vrq_rescore_dequant: compare_float32 rows
VRQ_RESCORE_SIGNED_BINARY = 17  # vrq_rescore_dequant / vrq_search2: packed sign codes as +-1 rows
VRQ_ENC_SIGNED_BINARY = 7
VRQ_K_LARGE_MAX = 8192  # the *_large entry points (K1h, the counting scan); 1024 for every other search
VRQ_K_MAX = 1024
VRQ_LARGE_STAGE_COUNT = 1
VRQ_LARGE_STAGE_THRESHOLD = 2
VRQ_LARGE_STAGE_EMIT = 4
VRQ_SCAN_KIND_VALU = 0
VRQ_SCAN_KIND_MFMA = 1
VRQ_SCAN_PLAN_K1RD = 3  # info[0] of vrq_scan_plan at the dims other than 1024

ENC_MODES = {
    "int8g": 0,   # VectorDBInt8Global
    "int16g": 1,  # VectorDBInt16Global
    "int4g": 2,   # VectorDBInt4Global (limit ignored, reference bug)
    "int8": 3,    # VectorDBInt8
    "int4": 4,    # VectorDBInt4
    "bin16": 5,   # VectorDBInt16._to_binary
    "cohere": 6,  # synthetic Cohere provider (int8 global + sign bits)
    "sbin": 7,    # CohereVectorDBBinary (packbits(x >= mean), codes only)
}

# name -> (restype, argtypes); mirrors include/vrq.h
_P, _I32, _I64, _SZ, _D = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_double
SIGNATURES = {
    "vrq_abi_version": (C.c_int, []),
    "vrq_strerror": (C.c_char_p, [C.c_int]),
    "vrq_hamming_topk_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_hamming_topk": (C.c_int, [_P, _I64, _I32, _I64, _P, _I32, _I32, _P, _P, _P, _SZ, _P]),
    "vrq_search3_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search3": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32,
                              _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_search3_scan": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _I32, _P, _SZ, _P]),
    "vrq_search3_finish": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _I32, _I32, _I32, _I32, _I32,
                                     _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_dim_supported": (C.c_int, [_I32]),
    "vrq_search3_dim_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search3_dim": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32,
                                  _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_search3_dim_scan": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _I32, _P, _SZ, _P]),
    "vrq_search3_dim_finish": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _I32, _I32, _I32, _I32, _I32,
                                         _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_rescore_binary_dim": (C.c_int, [_P, _I32, _I32, _P, _I64, _P, _I32, _P, _P]),
    "vrq_rescore_int8_cosine_dim": (C.c_int, [_P, _I32, _I32, _P, _P, _I64, _P, _I32, _P, _P]),
    "vrq_scan_kind": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _P]),
    "vrq_scan_plan": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _P]),
    "vrq_scan_sample_plan": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _P]),
    "vrq_merge_shards": (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "vrq_shard_search3_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_shard_search3": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32,
                                    _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_shard_search2_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_shard_search2": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32,
                                    _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_merge_shards2": (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _P]),
    "vrq_rescore_binary": (C.c_int, [_P, _I32, _I32, _P, _I64, _P, _I32, _P, _P]),
    "vrq_rescore_int8_cosine": (C.c_int, [_P, _I32, _I32, _P, _P, _I64, _P, _I32, _P, _P]),
    "vrq_encode": (C.c_int, [_I32, _P, _I64, _I32, _D, _P, _P, _P, _P]),
    "vrq_int8_row_norms": (C.c_int, [_P, _I64, _I32, _P, _P]),
    "vrq_dequantize": (C.c_int, [_I32, _P, _P, _I64, _I32, _D, _P, _P]),
    "vrq_rescore_dequant": (C.c_int, [_I32, _P, _I32, _I32, _P, _P, _D, _I64, _P, _I32, _P, _P]),
    "vrq_search2_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search2": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32,
                              _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_search2_finish": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _I32, _I32, _I32, _I32,
                                     _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_hamming_topk_large_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_hamming_topk_large": (C.c_int, [_P, _I64, _I32, _I64, _P, _I32, _I32, _P, _P, _P, _SZ, _P]),
    "vrq_search3_large_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search3_large": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32,
                                    _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_search2_large_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search2_large": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32,
                                    _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_shard_search3_large_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_shard_search3_large": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32,
                                          _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_shard_search2_large_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_shard_search2_large": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32,
                                          _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_merge_shards_large_workspace_size": (_SZ, [_I32, _I32, _I32]),
    "vrq_merge_shards_large": (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P,
                                         _P, _SZ, _P]),
    "vrq_merge_shards2_large": (C.c_int, [_I32, _I32, _I32, _P, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _SZ,
                                          _P]),
    "vrq_scan_large_plan": (C.c_int, [_I64, _I32, _I32, _I32, _P]),
    "vrq_scan_large": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _I32, _P, _SZ, _P]),
    "vrq_scan_filtered_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_scan_filtered": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _SZ, _P]),
    "vrq_hamming_topk_filtered_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_hamming_topk_filtered": (C.c_int, [_P, _I64, _I32, _I64, _P, _I32, _I32, _P, _P, _P, _P, _SZ, _P]),
    "vrq_search3_filtered_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search3_filtered": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32, _P,
                                       _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_search2_filtered_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search2_filtered": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32,
                                       _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "vrq_large_engine": (C.c_int, [_I64, _I32, _I32, _I32, _I32]),
    "vrq_scan_batch_plan": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _P]),
    "vrq_scan_batch_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_scan_batch": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _SZ, _P, _I32]),
    "vrq_hamming_topk_batch_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_hamming_topk_batch": (C.c_int, [_P, _I64, _I32, _I64, _P, _I32, _I32, _P, _P, _P, _P, _SZ, _P, _I32]),
    "vrq_search3_batch_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search3_batch": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32, _P,
                                    _P, _P, _P, _P, _P, _P, _SZ, _P, _I32]),
    "vrq_search2_batch_workspace_size": (_SZ, [_I64, _I32, _I32, _I32]),
    "vrq_search2_batch": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32,
                                    _P, _P, _P, _P, _P, _P, _SZ, _P, _I32]),
    # the *_batch prototypes followed by (int32 nsets, int64 set_words, const int32* query_set)
    "vrq_scan_perquery": (C.c_int, [_P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P, _SZ, _P, _I32, _I32, _I64, _P]),
    "vrq_hamming_topk_perquery": (C.c_int, [_P, _I64, _I32, _I64, _P, _I32, _I32, _P, _P, _P, _P, _SZ, _P, _I32,
                                            _I32, _I64, _P]),
    "vrq_search3_perquery": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32, _P,
                                       _P, _P, _P, _P, _P, _P, _SZ, _P, _I32, _I32, _I64, _P]),
    "vrq_search2_perquery": (C.c_int, [_I32, _P, _P, _P, _D, _P, _I64, _I32, _I64, _P, _P, _I32, _I32, _I32, _I32,
                                       _P, _P, _P, _P, _P, _P, _SZ, _P, _I32, _I32, _I64, _P]),
    "vrq_gemm_topk_workspace_size": (_SZ, [_I32, _I64, _I32, _I32, _I32]),
    "vrq_gemm_topk_pieces": (C.c_int, []),
    "vrq_gemm_topk_plan": (C.c_int, [_I32, _I64, _I32, _I32, _I32, _P]),
    "vrq_gemm_topk_layout": (C.c_int, [_I32, _I64, _I32, _I32, _I32, _P]),
    "vrq_gemm_topk_prep_layout": (C.c_int, [_I32, _I64, _I32, _I32, _I32, _P]),
    "vrq_gemm_topk": (C.c_int, [_I32, _P, _P, _P, _I64, _I32, _I64, _P, _I32, _I32, _I32, _P, _P, _P, _P, _SZ,
                                _P]),
    "vrq_gemm_topk_dim_workspace_size": (_SZ, [_I32, _I64, _I32, _I32, _I32]),
    "vrq_gemm_topk_dim_plan": (C.c_int, [_I32, _I64, _I32, _I32, _I32, _P]),
    "vrq_gemm_topk_dim": (C.c_int, [_I32, _P, _P, _P, _I64, _I32, _I64, _P, _I32, _I32, _I32, _P, _P, _P, _P, _SZ,
                                    _P]),
    "vrq_flat_ip_topk_dim": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _I32, _I32, _I32, _P, _P, _P, _P, _SZ,
                                       _P]),
    "vrq_flat_ip_prepare": (C.c_int, [_P, _I64, _I32, _P, _P, _P, _P]),
    "vrq_flat_ip_topk": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _I64, _P, _I32, _I32, _I32, _P, _P, _P, _P, _SZ,
                                   _P]),
}


class VrqNativeError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


_override = None


def use_library(path: str) -> None:
    """Load ``path`` instead of the in-tree libvrq.so in this process (tools/ sweeps of probe variants
    and tests only; call before the first load()).  The product never reads the environment for it."""
    global _override, _lib
    if _lib is not None:
        raise VrqNativeError("use_library() after the library was loaded")
    _override = path


def lib_path() -> str:
    return _override or _build.LIB


def _open(path: str, default: str, probe: bool = False):
    if not os.path.exists(path) or (path == default and not _build.up_to_date(default)):
        try:
            _build.build(probe=probe)
        except Exception as e:  # no hipcc on this host and no prebuilt library
            if not os.path.exists(path):
                raise VrqNativeError(f"{os.path.basename(path)} missing and cannot be built: {e}") from e
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise VrqNativeError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.vrq_abi_version() != 1:
        raise VrqNativeError("libvrq ABI version mismatch")
    return lib


def load():
    """Load (building first if needed and possible) libvrq.so; raise on failure."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            _lib = _open(lib_path(), _build.LIB)
        return _lib


_probe = None


def load_probe():
    """The probe build libvrq_probe.so: the same kernels, but its planners read the VRQ_* tuning
    overrides (VRQ_SAMPLE_DIV, VRQ_MFMA_MB, VRQ_MFMA_ROWS, VRQ_GEMM_SAMPLE_DIV, VRQ_GEMM_CHUNK_MULT)
    from the environment.  For sweeps and tests only; the product path always uses load()."""
    global _probe
    with _lock:
        if _probe is None:
            _probe = _open(_build.PROBE_LIB, _build.PROBE_LIB, probe=True)
        return _probe


def gemm_topk_dim_workspace(lib, mode: int, n: int, dim: int, nq: int, k: int, flags: int = 0) -> int:
    """Workspace bytes of a vrq_gemm_topk_dim / vrq_flat_ip_topk_dim call (0: unsupported shape).  At
    dim 1024 with VRQ_GEMM_SCAN_EXACT: the maximum of the forwarded path's size and the exact scan's."""
    need = lib.vrq_gemm_topk_dim_workspace_size(mode, n, dim, nq, k)
    if dim == 1024 and flags & VRQ_GEMM_SCAN_EXACT:
        info = (C.c_int64 * 6)()
        if lib.vrq_gemm_topk_dim_plan(mode, n, dim, nq, k, info) != VRQ_OK:
            return 0
        need = max(need, int(info[5]))
    return need


def large_k(K: int, what: str) -> bool:
    """Whether a search with K Phase-I candidates takes the *_large call (K1h, 1024 < K <= VRQ_K_LARGE_MAX);
    raises for a K beyond that."""
    if K > VRQ_K_LARGE_MAX:
        raise VrqNativeError(f"{what}: K = {K} Phase-I candidates (k * binary_oversample) exceed the limit "
                             f"of {VRQ_K_LARGE_MAX}")
    return K > VRQ_K_MAX


def filtered_k(K: int, flags: int, what: str) -> None:
    """A search with a row bitmap takes the *_filtered call (K1h) for every K up to VRQ_K_LARGE_MAX: raises for
    a K beyond that, and for the sharded mode and the scan flags, which the counting scan does not take."""
    large_k(K, what)
    if flags & ~VRQ_SEARCH_PHASE1_ONLY:
        raise VrqNativeError(f"{what}: flags {flags} with a row filter (the filtered calls take no "
                             "VRQ_SEARCH_SHARD and no scan flags)")


VRQ_LARGE_ENGINE_AUTO, VRQ_LARGE_ENGINE_VALU, VRQ_LARGE_ENGINE_MFMA = 0, 1, 2
_ENGINES = {"auto": VRQ_LARGE_ENGINE_AUTO, "valu": VRQ_LARGE_ENGINE_VALU, "mfma": VRQ_LARGE_ENGINE_MFMA}


def batch_engine(engine, K: int, flags: int, what: str):
    """The ``engine=`` argument of the search wrappers: ``None`` (today's route: returns None) or "auto" /
    "valu" / "mfma", the VRQ_LARGE_ENGINE_* value of the *_batch call the search then takes -- the counting
    scan, K1h or K1hm, for every K up to VRQ_K_LARGE_MAX, with or without a row bitmap.  Raises for a K
    beyond that, for an unknown name, and for the sharded mode and the scan flags."""
    if engine is None:
        return None
    if engine not in _ENGINES:
        raise VrqNativeError(f"{what}: engine {engine!r} (None, 'auto', 'mfma' or 'valu')")
    large_k(K, what)
    if flags & ~VRQ_SEARCH_PHASE1_ONLY:
        raise VrqNativeError(f"{what}: flags {flags} with engine={engine!r} (the batch calls take no "
                             "VRQ_SEARCH_SHARD and no scan flags)")
    return _ENGINES[engine]


def batch_call(base: str, engine, K: int, flags: int = 0, allow=None) -> str:
    """The entry point a search wrapper takes for ``base`` ("vrq_search3", "vrq_search2", "vrq_hamming_topk"):
    ``<base>_batch`` with an ``engine``, else ``<base>_filtered`` with a bitmap, ``<base>_large`` for
    K > 1024, ``base``."""
    return SearchCall(base, K, flags, allow, engine).name


def set_words_of(allow) -> int:
    """``set_words`` of a 2-D ``allow`` (int64 [S, words], unit stride along a row): the words from one bitmap to
    the next.  A size-1 dimension may carry any stride, so a single set is as wide as its row."""
    return int(allow.stride(0)) if allow.shape[0] > 1 else int(allow.shape[1])


class SearchCall:
    """The route of a search wrapper to its entry point, and the one place that sizes its workspace and makes
    the call.  ``name`` is ``<base>_batch`` with an ``engine``, else ``<base>_filtered`` with a bitmap ``allow``,
    ``<base>_large`` for K > 1024, else ``plain`` (default ``base``); ``engine`` is the resolved
    VRQ_LARGE_ENGINE_* value (None outside the batch calls).  ``what`` names the caller in the errors
    ``batch_engine`` / ``filtered_k`` / ``large_k`` raise (default ``base``).

    With ``query_set`` (one set id per query; ``allow`` then holds a bitmap per set, ``filters.row_bitmaps``)
    the route is ``<base>_perquery``: a batch call with the filter's shape after the engine.  It has no earlier
    route to preserve, so ``engine=None`` means "auto" there; its workspace is the batch call's."""

    def __init__(self, base: str, K: int, flags: int = 0, allow=None, engine=None, what: str = None,
                 plain: str = None, query_set=None):
        what = what or base
        self.perquery = query_set is not None
        if self.perquery:
            if allow is None:
                raise VrqNativeError(f"{what}: query_set without allow (a bitmap per set, filters.row_bitmaps)")
            engine = "auto" if engine is None else engine
        elif allow is not None and getattr(allow, "ndim", 1) != 1:
            raise VrqNativeError(f"{what}: a {allow.ndim}-D allow needs query_set (one set id per query)")
        self.engine = batch_engine(engine, K, flags, what)
        self.sized_by = None  # the call whose *_workspace_size serves this one (default: its own)
        if self.perquery:
            self.name = base + "_perquery"
            self.sized_by = base + "_batch"
        elif self.engine is not None:
            self.name = base + "_batch"
        elif allow is not None:
            filtered_k(K, flags, what)
            self.name = base + "_filtered"
        else:
            self.name = base + "_large" if large_k(K, what) else plain or base
        self.bitmap = self.engine is not None or allow is not None  # the call has a bitmap argument

    def workspace_bytes(self, lib, n: int, width: int, nq: int, K: int) -> int:
        """``<name>_workspace_size`` (``width``: dim, or code bytes for vrq_hamming_topk*); 0 for an empty shape."""
        return getattr(lib, (self.sized_by or self.name) + "_workspace_size")(n, width, nq, K) if n and nq and K else 0

    def workspace(self, lib, n: int, width: int, nq: int, K: int, device, have=None):
        """``have`` where it is large enough, else a new uint8 tensor of max(8, workspace_bytes) bytes."""
        import torch
        need = self.workspace_bytes(lib, n, width, nq, K)
        if have is not None and have.numel() >= need:
            return have
        return torch.empty((max(8, need),), dtype=torch.uint8, device=device)

    def __call__(self, lib, head: tuple, tail: tuple, allow, ws, device, label: str = None, query_set=None) -> None:
        """``name(*head, [allow,] *tail, ws, bytes, stream[, engine[, nsets, set_words, query_set]])``: the
        bitmap's pointer goes between the inputs and the outputs of a *_filtered / *_batch / *_perquery call, the
        engine ends a *_batch call, the filter's shape (from the 2-D ``allow``) a *_perquery call.  Raises unless
        VRQ_OK."""
        args = head + ((ptr(allow),) if self.bitmap else ()) + tail + (ptr(ws), ws.numel(), stream_handle(device))
        end = () if self.engine is None else (self.engine,)
        if self.perquery:
            end += (int(allow.shape[0]), set_words_of(allow), ptr(query_set)) if allow is not None else (1, 0, 0)
        check(getattr(lib, self.name)(*args, *end), label or self.name)


def check(rc: int, what: str) -> None:
    if rc != VRQ_OK:
        msg = load().vrq_strerror(rc).decode()
        raise VrqNativeError(f"{what} failed: {msg} ({rc})")


def ptr(t) -> int:
    """Raw device pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else int(t.data_ptr())


def stream_handle(device=None) -> int:
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)
