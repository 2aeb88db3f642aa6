"""ctypes binding of libbbq.so (include/bbq.h).  Plumbing only: every numeric operation happens in the
C++/HIP library.  There is no CPU fallback - device entry points raise BBQError(BBQ_ERR_NO_DEVICE) without a GPU."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))            # better-binary-quantization_amd/
LIB_PATH = os.environ.get("BBQ_LIB") or os.path.join(PKG_ROOT, "lib", "libbbq.so")  # BBQ_LIB: experiments with alternative builds

OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5
ERR_DIM_MISMATCH, ERR_NEGATIVE_K, ERR_NAN_INPUT, ERR_INF_INPUT, ERR_EMPTY = 6, 7, 8, 9, 10
EUCLIDEAN, COSINE, MAXIMUM_INNER_PRODUCT = 0, 1, 2
SIMS = {"EUCLIDEAN": 0, "COSINE": 1, "MAXIMUM_INNER_PRODUCT": 2}

# every symbol include/bbq.h declares (tests/test_capi_symbols.py checks the library exports all of them)
SYMBOLS = [
    "bbq_last_error", "bbq_abi_version", "bbq_device_count", "bbq_index_create", "bbq_index_create_shard", "bbq_index_create_multi", "bbq_index_shards", "bbq_index_build", "bbq_index_build_bits",
    "bbq_index_destroy", "bbq_index_size", "bbq_index_dimension", "bbq_index_bytes_per_row", "bbq_index_bits", "bbq_search",
    "bbq_search_batch", "bbq_score_rows", "bbq_shard_scan", "bbq_shard_list_cap", "bbq_replay", "bbq_replay_batch",
    "bbq_quantize_vectors", "bbq_quantize_query", "bbq_quantize_query_vector", "bbq_centroid_dp", "bbq_get_stats",
    "bbq_reset_stats", "bbq_set_option", "bbq_vectors_create", "bbq_vectors_destroy", "bbq_vectors_size",
    "bbq_vectors_dimension", "bbq_rerank_scores", "bbq_search_rerank_batch", "bbq_index_save", "bbq_index_file_info",
    "bbq_index_load", "bbq_index_export", "bbq_quantize_queries",
    "bbq_index_create_shard_opts", "bbq_index_create_multi_opts", "bbq_index_build_opts",
    "bbq_shard_scan_begin", "bbq_shard_scan_wait", "bbq_merge_answers", "bbq_key_of_score", "bbq_index_load_multi", "bbq_index_file_shards",
    "bbq_search_raw_batch",
    "bbq_filter_create", "bbq_filter_create_rows", "bbq_filter_destroy", "bbq_filter_count", "bbq_search_filtered_batch", "bbq_filter_plan",
    "bbq_index_append_rows", "bbq_index_append", "bbq_index_reserve", "bbq_index_capacity", "bbq_vectors_append", "bbq_quantize_rows",
    "bbq_index_compact", "bbq_index_remove_rows", "bbq_vectors_compact", "bbq_filter_kept_rows",
    "bbq_index_update_rows", "bbq_index_update", "bbq_vectors_update", "bbq_update_winners",
    "bbq_score_ords", "bbq_score_ords_batch", "bbq_search_ords_batch",
    "bbq_range_key", "bbq_count_range_batch", "bbq_search_range_batch",
    "bbq_search_spans_batch", "bbq_search_spans_filtered_batch",
    "bbq_groups_create", "bbq_groups_destroy", "bbq_groups_count", "bbq_groups_live", "bbq_groups_plan", "bbq_search_grouped_batch",
    "bbq_search_maxsim_batch", "bbq_maxsim_reduce", "bbq_maxsim_token_block",
    "bbq_score_maxsim_groups_batch", "bbq_search_maxsim_groups_batch",
    "bbq_maxsim_reduce_true", "bbq_rerank_maxsim_groups_batch", "bbq_search_maxsim_rerank_batch",
    "bbq_true_topk", "bbq_vectors_search_batch", "bbq_vectors_set_option",
]


class BBQError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


class IndexOptions(C.Structure):
    """bbq_index_options (include/bbq.h)"""
    _fields_ = [("size", C.c_int32), ("corrections", C.c_int32)]


CORRECTIONS_DEFAULT, CORRECTIONS_INLINE, CORRECTIONS_COMPACT = -1, 0, 1


def _opts(corrections):
    """corrections: None (library default) | "inline" | "compact" | a BBQ_CORRECTIONS_* ordinal"""
    if corrections is None:
        return None
    v = {"inline": CORRECTIONS_INLINE, "compact": CORRECTIONS_COMPACT, "default": CORRECTIONS_DEFAULT}.get(corrections, corrections)
    return C.byref(IndexOptions(C.sizeof(IndexOptions), int(v)))


class Stats(C.Structure):
    _fields_ = [("last_scan_ms", C.c_double), ("last_scan_rows", C.c_int64), ("last_scan_bytes", C.c_int64),
                ("candidates", C.c_int64), ("dense_fallbacks", C.c_int64), ("total_scan_ms", C.c_double),
                ("total_scan_bytes", C.c_int64), ("total_scan_launches", C.c_int64), ("host_replays", C.c_int64), ("resident_bytes", C.c_int64)]


_lib = None


def lib():
    """loads libbbq.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()').
    Note: PyTorch-ROCm wheels bundle their own libamdhip64 with the system's soname; a process that uses both must
    import torch BEFORE the first call into libbbq so that one HIP runtime serves both."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BBQError(ERR_NO_DEVICE, "libbbq.so is not built (%s): run __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.bbq_last_error.restype = C.c_char_p
    L.bbq_abi_version.restype = C.c_int
    L.bbq_device_count.restype = C.c_int
    L.bbq_index_create.argtypes = [vp, vp, i64, i32, i32, dbl, i32, C.POINTER(vp)]
    L.bbq_index_create_shard.argtypes = [vp, vp, i64, i32, i32, dbl, i64, vp, vp, i64, i32, C.POINTER(vp)]
    L.bbq_index_create_multi.argtypes = [vp, vp, i64, i32, i32, dbl, i32, vp, i64, C.POINTER(vp)]
    L.bbq_index_create_shard_opts.argtypes = [vp, vp, i64, i32, i32, dbl, i64, vp, vp, i64, i32, vp, C.POINTER(vp)]
    L.bbq_index_create_multi_opts.argtypes = [vp, vp, i64, i32, i32, dbl, i32, vp, i64, vp, C.POINTER(vp)]
    L.bbq_index_build_opts.argtypes = [vp, i64, i32, i32, i32, dbl, i32, i32, vp, C.POINTER(vp), vp, vp, vp, vp, vp]
    L.bbq_index_shards.argtypes = [vp]
    L.bbq_index_shards.restype = i32
    L.bbq_index_build.argtypes = [vp, i64, i32, i32, dbl, i32, i32, C.POINTER(vp), vp, vp, vp, vp, vp]
    L.bbq_index_build_bits.argtypes = [vp, i64, i32, i32, i32, dbl, i32, i32, C.POINTER(vp), vp, vp, vp, vp, vp]
    L.bbq_index_destroy.argtypes = [vp]
    L.bbq_index_destroy.restype = None
    L.bbq_index_size.argtypes = [vp]
    L.bbq_index_size.restype = i64
    L.bbq_index_dimension.argtypes = [vp]
    L.bbq_index_dimension.restype = i32
    L.bbq_index_bytes_per_row.argtypes = [vp]
    L.bbq_index_bytes_per_row.restype = i32
    L.bbq_index_bits.argtypes = [vp]
    L.bbq_index_bits.restype = i32
    L.bbq_search.argtypes = [vp, vp, vp, i32, i32, i64, vp, vp, vp]
    L.bbq_search_batch.argtypes = [vp, i32, vp, vp, i32, i32, i64, vp, vp, vp]
    L.bbq_search_raw_batch.argtypes = [vp, i32, vp, vp, i32, i32, dbl, i32, i32, i64, vp, vp, vp, vp, vp, C.POINTER(i32)]
    L.bbq_score_rows.argtypes = [vp, vp, vp, i32, i32, i64, i64, vp, vp, vp]
    L.bbq_score_ords.argtypes = [vp, vp, vp, i32, i32, vp, i64, vp, vp, vp]
    L.bbq_score_ords_batch.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.bbq_search_ords_batch.argtypes = [vp, i32, vp, vp, i32, i32, i64, vp, vp, vp, vp, vp]
    L.bbq_range_key.argtypes = [C.c_float, C.POINTER(C.c_uint32)]
    L.bbq_count_range_batch.argtypes = [vp, vp, i32, vp, vp, i32, i32, vp, vp]
    L.bbq_search_range_batch.argtypes = [vp, vp, i32, vp, vp, i32, i32, vp, i64, vp, vp, vp]
    L.bbq_search_spans_batch.argtypes = [vp, i32, vp, vp, i32, i32, i64, vp, vp, vp, vp, vp, vp]
    L.bbq_search_spans_filtered_batch.argtypes = [vp, vp, i32, vp, vp, i32, i32, i64, vp, vp, vp, vp, vp, vp]
    L.bbq_groups_create.argtypes = [vp, vp, i64, vp, C.POINTER(vp)]
    L.bbq_groups_destroy.argtypes = [vp]
    L.bbq_groups_destroy.restype = None
    L.bbq_groups_count.argtypes = [vp]
    L.bbq_groups_count.restype = i64
    L.bbq_groups_live.argtypes = [vp]
    L.bbq_groups_live.restype = i64
    L.bbq_groups_plan.argtypes = [vp, i64, i64, vp, vp, C.POINTER(i64)]
    L.bbq_search_grouped_batch.argtypes = [vp, vp, i32, vp, vp, i32, i32, i64, vp, vp, vp, vp, vp]
    L.bbq_search_maxsim_batch.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i64, vp, vp, vp, vp]
    L.bbq_maxsim_reduce.argtypes = [vp, i64, i64, vp]
    L.bbq_score_maxsim_groups_batch.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
    L.bbq_search_maxsim_groups_batch.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i64, vp, vp, vp, vp, vp]
    L.bbq_maxsim_reduce_true.argtypes = [vp, i64, i64, vp]
    L.bbq_rerank_maxsim_groups_batch.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.bbq_search_maxsim_rerank_batch.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i64, i32, i32, i32, vp, vp, vp, vp]
    L.bbq_true_topk.argtypes = [vp, i64, vp, i64, vp, vp, C.POINTER(i64)]
    L.bbq_vectors_search_batch.argtypes = [vp, vp, i32, vp, i32, i64, vp, vp, vp]
    L.bbq_vectors_set_option.argtypes = [vp, C.c_char_p, i64]
    L.bbq_maxsim_token_block.argtypes = []
    L.bbq_maxsim_token_block.restype = i32
    L.bbq_filter_create.argtypes = [vp, vp, i64, C.POINTER(vp)]
    L.bbq_filter_create_rows.argtypes = [vp, vp, i64, C.POINTER(vp)]
    L.bbq_filter_destroy.argtypes = [vp]
    L.bbq_filter_destroy.restype = None
    L.bbq_filter_count.argtypes = [vp]
    L.bbq_filter_count.restype = i64
    L.bbq_filter_plan.argtypes = [vp, i64, i64, i64, i32, i32, vp, C.POINTER(i32)]
    L.bbq_search_filtered_batch.argtypes = [vp, vp, i32, vp, vp, i32, i32, i64, vp, vp, vp]
    L.bbq_shard_scan.argtypes = [vp, i32, vp, vp, i32, i32, i64, vp, i64, vp, vp, C.POINTER(i64)]
    L.bbq_shard_scan_begin.argtypes = [vp, i32, vp, vp, i32, i32, i64, vp, i64, vp, vp, vp, i64]
    L.bbq_shard_scan_wait.argtypes = [vp, C.POINTER(i64)]
    L.bbq_merge_answers.argtypes = [i32, vp, vp, i32, i64, i64, i32, vp, vp, vp, vp]
    L.bbq_key_of_score.argtypes = [C.c_float]
    L.bbq_key_of_score.restype = C.c_uint32
    L.bbq_shard_list_cap.argtypes = [vp, i64]
    L.bbq_shard_list_cap.restype = i64
    L.bbq_replay.argtypes = [i32, vp, vp, i64, i64, vp, vp, vp]
    L.bbq_replay_batch.argtypes = [i32, vp, vp, i32, i64, i64, i32, vp, vp, vp]
    L.bbq_quantize_vectors.argtypes = [vp, i64, i32, i32, i32, dbl, i32, i32, vp, vp, vp, vp, vp]
    L.bbq_quantize_query.argtypes = [vp, i32, vp, i32, i32, dbl, i32, vp, vp]
    L.bbq_quantize_query_vector.argtypes = [vp, i32, vp, i32, i32, dbl, i32, vp, vp]
    L.bbq_quantize_queries.argtypes = [vp, i32, i32, vp, i32, i32, dbl, i32, i32, vp, vp, C.POINTER(i32)]
    L.bbq_centroid_dp.argtypes = [vp, i32]
    L.bbq_centroid_dp.restype = dbl
    L.bbq_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.bbq_reset_stats.argtypes = [vp]
    L.bbq_set_option.argtypes = [vp, C.c_char_p, i64]
    L.bbq_vectors_create.argtypes = [vp, i64, i32, i32, C.POINTER(vp)]
    L.bbq_vectors_destroy.argtypes = [vp]
    L.bbq_vectors_destroy.restype = None
    L.bbq_vectors_size.argtypes = [vp]
    L.bbq_vectors_size.restype = i64
    L.bbq_vectors_dimension.argtypes = [vp]
    L.bbq_vectors_dimension.restype = i32
    L.bbq_rerank_scores.argtypes = [vp, i32, vp, vp, vp, i32, vp]
    L.bbq_search_rerank_batch.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i64, i32, i32, i32, vp, vp, vp, vp]
    L.bbq_index_save.argtypes = [vp, C.c_char_p, vp, i32]
    L.bbq_index_file_info.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), C.POINTER(dbl), C.POINTER(i64)]
    L.bbq_index_load.argtypes = [C.c_char_p, i32, C.POINTER(vp), vp]
    L.bbq_index_load_multi.argtypes = [C.c_char_p, i32, vp, C.POINTER(vp), vp]
    L.bbq_index_file_shards.argtypes = [C.c_char_p]
    L.bbq_index_file_shards.restype = i32
    L.bbq_index_export.argtypes = [vp, vp, vp]
    L.bbq_index_append_rows.argtypes = [vp, vp, vp, i64]
    L.bbq_index_append.argtypes = [vp, vp, i64, vp, i32, dbl, i32, vp, vp, C.POINTER(i64), C.POINTER(i32)]
    L.bbq_index_reserve.argtypes = [vp, i64]
    L.bbq_index_capacity.argtypes = [vp]
    L.bbq_index_capacity.restype = i64
    L.bbq_vectors_append.argtypes = [vp, vp, i64]
    L.bbq_index_compact.argtypes = [vp, vp]
    L.bbq_index_remove_rows.argtypes = [vp, vp, i64]
    L.bbq_vectors_compact.argtypes = [vp, vp]
    L.bbq_filter_kept_rows.argtypes = [vp, i64, vp, i64, C.POINTER(i64)]
    L.bbq_index_update_rows.argtypes = [vp, vp, vp, vp, i64]
    L.bbq_index_update.argtypes = [vp, vp, vp, i64, vp, i32, dbl, i32, vp, vp, C.POINTER(i64), C.POINTER(i32)]
    L.bbq_vectors_update.argtypes = [vp, vp, vp, i64]
    L.bbq_update_winners.argtypes = [vp, i64, i64, vp, i64, C.POINTER(i64)]
    L.bbq_quantize_rows.argtypes = [vp, i64, i32, vp, i32, i32, dbl, i32, i32, vp, vp, C.POINTER(i64), C.POINTER(i32)]
    _lib = L
    return L


def _chk(rc):
    if rc != OK:
        raise BBQError(rc, lib().bbq_last_error().decode("utf-8", "replace"))


def _chk_pos(call):
    """_chk for the entry points that report where a NaN / Infinity sits: the BBQError carries .bad_row / .bad_col"""
    br, bc = C.c_int64(-1), C.c_int32(-1)
    rc = call(C.byref(br), C.byref(bc))
    if rc != OK:
        e = BBQError(rc, lib().bbq_last_error().decode("utf-8", "replace"))
        e.bad_row, e.bad_col = br.value, bc.value
        raise e


def _ptr(a):
    return None if a is None else a.ctypes.data


def device_count():
    return lib().bbq_device_count()


# ------------------------------------------------------------------------------------------------ host quantizer

def quantize_vectors(vectors, sim, index_bits=1, lam=0.1, iters=5, n_threads=0):
    v = np.ascontiguousarray(vectors, np.float32)
    if v.ndim != 2:
        raise BBQError(ERR_INVALID_ARG, "vectors must be [n, dim]")
    n, dim = v.shape
    if n == 0:
        raise BBQError(ERR_EMPTY, "向量集合不能为空")
    pb = (dim + 7) // 8 if index_bits == 1 else dim
    codes = np.zeros((n, pb), np.uint8)
    corr = np.zeros((n, 4), np.float64)
    cen = np.zeros(dim, np.float32)
    _chk(lib().bbq_quantize_vectors(_ptr(v), n, dim, sim, index_bits, lam, iters, n_threads, _ptr(codes), _ptr(corr), _ptr(cen),
                                   None, None))
    return codes, corr, cen


def quantize_rows(vectors, centroid, sim, index_bits=1, lam=0.1, iters=5, n_threads=0):
    """quantizeVectors' per-row part against a GIVEN centroid (bbq_quantize_rows; host only): (codes, corr) - what Index.append
    computes on the device.  A NaN / Infinity raises BBQError with .bad_row / .bad_col set."""
    v = np.ascontiguousarray(vectors, np.float32)
    cen = np.ascontiguousarray(centroid, np.float32)
    if v.ndim != 2 or cen.shape != (v.shape[1],):
        raise BBQError(ERR_DIM_MISMATCH, "向量维度不匹配")
    n, dim = v.shape
    codes = np.zeros((n, (dim + 7) // 8 if index_bits == 1 else dim), np.uint8)
    corr = np.zeros((n, 4), np.float64)
    _chk_pos(lambda br, bc: lib().bbq_quantize_rows(_ptr(v), n, dim, _ptr(cen), sim, index_bits, lam, iters, n_threads, _ptr(codes), _ptr(corr), br, bc))
    return codes, corr


def quantize_query(query, centroid, sim, query_bits=4, lam=0.1, iters=5, search_path=True):
    q = np.ascontiguousarray(query, np.float32)
    cen = np.ascontiguousarray(centroid, np.float32)
    dim = q.shape[0]
    qq = np.zeros(dim, np.uint8)
    qc = np.zeros(4, np.float64)
    fn = lib().bbq_quantize_query if search_path else lib().bbq_quantize_query_vector
    _chk(fn(_ptr(q), dim, _ptr(cen), sim, query_bits, lam, iters, _ptr(qq), _ptr(qc)))
    return qq, qc


def quantize_queries(queries, centroid, sim, query_bits=4, lam=0.1, iters=5, n_threads=0):
    """searchNearestNeighbors' query preparation for a batch, on host threads: (qquant [n, dim], qcorr [n, 4])"""
    q = np.ascontiguousarray(queries, np.float32)
    cen = np.ascontiguousarray(centroid, np.float32)
    if q.ndim != 2 or q.shape[1] != cen.shape[0]:
        raise BBQError(ERR_DIM_MISMATCH, "查询向量维度与目标向量维度不匹配")
    n, dim = q.shape
    qq = np.zeros((n, dim), np.uint8)
    qc = np.zeros((n, 4), np.float64)
    bad = C.c_int32(-1)
    _chk(lib().bbq_quantize_queries(_ptr(q), n, dim, _ptr(cen), sim, query_bits, lam, iters, n_threads, _ptr(qq), _ptr(qc), C.byref(bad)))
    return qq, qc


def centroid_dp(centroid):
    cen = np.ascontiguousarray(centroid, np.float32)
    return lib().bbq_centroid_dp(_ptr(cen), cen.shape[0])


# ------------------------------------------------------------------------------------------------ device index

class Index:
    """a device-resident index shard (bbq_index)"""

    def __init__(self, codes, corr, dim, cdp, device=0, index_bits=1, row_base=0, pilot_codes=None, pilot_corr=None, corrections=None):
        codes = np.ascontiguousarray(codes, np.uint8)
        corr = np.ascontiguousarray(corr, np.float64)
        n = codes.shape[0]
        h = C.c_void_p()
        if pilot_codes is not None:
            pilot_codes = np.ascontiguousarray(pilot_codes, np.uint8)
            pilot_corr = np.ascontiguousarray(pilot_corr, np.float64)
            npilot = pilot_codes.shape[0]
        else:
            npilot = 0
        _chk(lib().bbq_index_create_shard_opts(_ptr(codes), _ptr(corr), n, dim, index_bits, cdp, row_base, _ptr(pilot_codes),
                                              _ptr(pilot_corr), npilot, device, _opts(corrections), C.byref(h)))
        self._h = h
        self.dim = dim
        self.n = n
        self.index_bits = index_bits

    @classmethod
    def create_multi(cls, codes, corr, dim, cdp, devices, index_bits=1, pilot_rows=32768, corrections=None):
        """one index row-sharded over `devices` (a list of HIP ordinals, one shard each; repeats allowed) behind one handle"""
        codes = np.ascontiguousarray(codes, np.uint8)
        corr = np.ascontiguousarray(corr, np.float64)
        dev = np.ascontiguousarray(devices, np.int32)
        h = C.c_void_p()
        _chk(lib().bbq_index_create_multi_opts(_ptr(codes), _ptr(corr), codes.shape[0], dim, index_bits, cdp, len(dev), _ptr(dev), pilot_rows,
                                              _opts(corrections), C.byref(h)))
        self = cls.__new__(cls)
        self._h, self.dim, self.n, self.index_bits = h, dim, codes.shape[0], index_bits
        return self

    @property
    def shards(self):
        return lib().bbq_index_shards(self._h)

    @classmethod
    def build(cls, vectors, sim, lam=0.1, iters=5, device=0, want_host_copy=True, index_bits=1, corrections=None):
        """quantizeVectors on the device (bbq_index_build_bits): returns (index, codes, corr, centroid); codes/corr are None
        unless want_host_copy"""
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim != 2:
            raise BBQError(ERR_INVALID_ARG, "vectors must be [n, dim]")
        n, dim = v.shape
        cen = np.zeros(dim, np.float32)
        codes = np.zeros((n, (dim + 7) // 8 if index_bits == 1 else dim), np.uint8) if want_host_copy else None
        corr = np.zeros((n, 4), np.float64) if want_host_copy else None
        h = C.c_void_p()
        _chk(lib().bbq_index_build_opts(_ptr(v), n, dim, sim, index_bits, lam, iters, device, _opts(corrections), C.byref(h), _ptr(cen), _ptr(codes),
                                       _ptr(corr), None, None))
        self = cls.__new__(cls)
        self._h, self.dim, self.n, self.index_bits = h, dim, n, index_bits
        return self, codes, corr, cen

    def save(self, path_prefix, centroid, sim):
        """<prefix>.veb (the device tiles, byte for byte) + <prefix>.vemb (MetadataFormat + geometry + centroid)"""
        cen = np.ascontiguousarray(centroid, np.float32)
        if cen.shape != (self.dim,):
            raise BBQError(ERR_DIM_MISMATCH, "centroid must be [dim]")
        _chk(lib().bbq_index_save(self._h, os.fsencode(path_prefix), _ptr(cen), sim))

    @classmethod
    def load(cls, path_prefix, device=0):
        """returns (index, centroid, info): a straight file -> HBM copy, no re-tiling"""
        info = file_info(path_prefix)
        cen = np.zeros(info["dim"], np.float32)
        h = C.c_void_p()
        _chk(lib().bbq_index_load(os.fsencode(path_prefix), device, C.byref(h), _ptr(cen)))
        self = cls.__new__(cls)
        self._h, self.dim, self.n = h, info["dim"], info["n_rows"]
        self.index_bits = lib().bbq_index_bits(h)
        return self, cen, info

    @classmethod
    def load_multi(cls, path_prefix, devices=None):
        """a saved multi-device index back over `devices` (None: shard s on device s modulo the visible ones): (index, centroid, info)"""
        info = file_info(path_prefix)
        cen = np.zeros(info["dim"], np.float32)
        dev = None if devices is None else np.ascontiguousarray(devices, np.int32)
        h = C.c_void_p()
        _chk(lib().bbq_index_load_multi(os.fsencode(path_prefix), 0 if dev is None else len(dev), _ptr(dev), C.byref(h), _ptr(cen)))
        self = cls.__new__(cls)
        self._h, self.dim, self.n = h, info["dim"], info["n_rows"]
        self.index_bits = lib().bbq_index_bits(h)
        return self, cen, info

    def export(self):
        """(codes [n, ceil(dim/8)], corr [n, 4]) as vectorValue / getCorrectiveTerms would return them"""
        codes = np.zeros((self.n, (self.dim + 7) // 8 if self.index_bits == 1 else self.dim), np.uint8)
        corr = np.zeros((self.n, 4), np.float64)
        _chk(lib().bbq_index_export(self._h, _ptr(codes), _ptr(corr)))
        return codes, corr

    def append_rows(self, codes, corr):
        """bbq_index_append_rows: rows already quantized, in the shape the constructor takes them, get the next ords"""
        codes = np.ascontiguousarray(codes, np.uint8)
        corr = np.ascontiguousarray(corr, np.float64)
        width = (self.dim + 7) // 8 if self.index_bits == 1 else self.dim
        if codes.ndim != 2 or codes.shape[1] != width or corr.shape != (codes.shape[0], 4):
            raise BBQError(ERR_DIM_MISMATCH, "codes must be [n, %d] and corr [n, 4]" % width)
        _chk(lib().bbq_index_append_rows(self._h, _ptr(codes), _ptr(corr), codes.shape[0]))
        self.n = int(lib().bbq_index_size(self._h))

    def append(self, vectors, centroid, sim, lam=0.1, iters=5, want_host_copy=True):
        """bbq_index_append: raw fp32 rows quantized on the device against `centroid` (the one the index was built with).
        Returns (codes, corr) of the new rows, or (None, None) unless want_host_copy.  A NaN / Infinity raises BBQError with
        .bad_row / .bad_col (position inside `vectors`) and leaves the index as it was."""
        v = np.ascontiguousarray(vectors, np.float32)
        cen = np.ascontiguousarray(centroid, np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim or cen.shape != (self.dim,):
            raise BBQError(ERR_DIM_MISMATCH, "向量维度不匹配")
        n = v.shape[0]
        codes = np.zeros((n, (self.dim + 7) // 8 if self.index_bits == 1 else self.dim), np.uint8) if want_host_copy else None
        corr = np.zeros((n, 4), np.float64) if want_host_copy else None
        _chk_pos(lambda br, bc: lib().bbq_index_append(self._h, _ptr(v), n, _ptr(cen), int(sim), lam, iters, _ptr(codes), _ptr(corr), br, bc))
        self.n = int(lib().bbq_index_size(self._h))
        return codes, corr

    def update_rows(self, ords, codes, corr):
        """bbq_index_update_rows: rows already quantized, in the shape the constructor takes them, replace the rows `ords` names in
        place (the last of equal ords wins).  The size, and with it every filter, stays."""
        o = _ords(ords)
        codes = np.ascontiguousarray(codes, np.uint8)
        corr = np.ascontiguousarray(corr, np.float64)
        width = (self.dim + 7) // 8 if self.index_bits == 1 else self.dim
        if codes.ndim != 2 or codes.shape[1] != width or corr.shape != (codes.shape[0], 4) or o.shape[0] != codes.shape[0]:
            raise BBQError(ERR_DIM_MISMATCH, "ords must be [n], codes [n, %d] and corr [n, 4]" % width)
        _chk(lib().bbq_index_update_rows(self._h, _ptr(o), _ptr(codes), _ptr(corr), o.shape[0]))

    def update(self, ords, vectors, centroid, sim, lam=0.1, iters=5, want_host_copy=True):
        """bbq_index_update: raw fp32 rows quantized on the device against `centroid` (the one the index was built with) replace
        the rows `ords` names in place.  Returns (codes, corr) of ALL rows of the block, or (None, None) unless want_host_copy.  A
        NaN / Infinity raises BBQError with .bad_row / .bad_col (position inside `vectors`) and leaves the index as it was."""
        o = _ords(ords)
        v = np.ascontiguousarray(vectors, np.float32)
        cen = np.ascontiguousarray(centroid, np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim or cen.shape != (self.dim,) or o.shape[0] != v.shape[0]:
            raise BBQError(ERR_DIM_MISMATCH, "向量维度不匹配")
        n = v.shape[0]
        codes = np.zeros((n, (self.dim + 7) // 8 if self.index_bits == 1 else self.dim), np.uint8) if want_host_copy else None
        corr = np.zeros((n, 4), np.float64) if want_host_copy else None
        _chk_pos(lambda br, bc: lib().bbq_index_update(self._h, _ptr(o), _ptr(v), n, _ptr(cen), int(sim), lam, iters, _ptr(codes), _ptr(corr), br, bc))
        return codes, corr

    def compact(self, flt):
        """bbq_index_compact: the index becomes the index over the rows `flt` (a Filter of this index) accepts, in order, on the
        device.  The filter - and any made earlier - no longer fits afterwards; kept_rows(mask) tells the old ord of every new row."""
        _chk(lib().bbq_index_compact(self._h, flt._h if flt is not None else None))
        self.n = int(lib().bbq_index_size(self._h))

    def remove_rows(self, rows):
        """bbq_index_remove_rows: drop these ords (any order, duplicates allowed)"""
        r = np.ascontiguousarray(np.asarray(rows, np.int64).ravel().clip(-2**31, 2**31 - 1), np.int32)
        _chk(lib().bbq_index_remove_rows(self._h, _ptr(r), r.shape[0]))
        self.n = int(lib().bbq_index_size(self._h))

    def reserve(self, rows):
        """room for `rows` rows in total without another reallocation (bbq_index_reserve)"""
        _chk(lib().bbq_index_reserve(self._h, int(rows)))

    @property
    def capacity(self):
        """rows the current allocations hold (>= n)"""
        return int(lib().bbq_index_capacity(self._h))

    def close(self):
        if self._h:
            lib().bbq_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def bytes_per_row(self):
        return lib().bbq_index_bytes_per_row(self._h)

    def set_option(self, name, value):
        _chk(lib().bbq_set_option(self._h, name.encode(), int(value)))

    def stats(self):
        s = Stats()
        _chk(lib().bbq_get_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in Stats._fields_}

    def reset_stats(self):
        _chk(lib().bbq_reset_stats(self._h))

    def search(self, qquant, qcorr, query_bits, sim, k):
        idx, sc, n = self.search_batch(np.asarray(qquant)[None, :], np.asarray(qcorr)[None, :], query_bits, sim, k)
        return idx[0, :n[0]], sc[0, :n[0]]

    def search_batch(self, qquant, qcorr, query_bits, sim, k):
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        nq = qq.shape[0]
        if nq and qq.shape[1] != self.dim:
            raise BBQError(ERR_DIM_MISMATCH, "查询向量维度与目标向量维度不匹配")
        kk = max(int(k), 0)
        idx = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        _chk(lib().bbq_search_batch(self._h, nq, _ptr(qq), _ptr(qc), query_bits, sim, k, _ptr(idx), _ptr(sc), _ptr(cnt)))
        return idx, sc, cnt

    def search_filtered(self, qquant, qcorr, query_bits, sim, k, flt):
        """bbq_search restricted to the rows `flt` (a Filter of this index) accepts"""
        idx, sc, n = self.search_filtered_batch(np.asarray(qquant)[None, :], np.asarray(qcorr)[None, :], query_bits, sim, k, flt)
        return idx[0, :n[0]], sc[0, :n[0]]

    def search_filtered_batch(self, qquant, qcorr, query_bits, sim, k, flt):
        """bbq_search_filtered_batch: search_batch over the accepted rows only; one filter serves every query of the call"""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        nq = qq.shape[0]
        if nq and qq.shape[1] != self.dim:
            raise BBQError(ERR_DIM_MISMATCH, "查询向量维度与目标向量维度不匹配")
        kk = max(int(k), 0)
        idx = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        _chk(lib().bbq_search_filtered_batch(self._h, flt._h if flt is not None else None, nq, _ptr(qq), _ptr(qc), query_bits, sim, k,
                                            _ptr(idx), _ptr(sc), _ptr(cnt)))
        return idx, sc, cnt

    def search_raw_batch(self, queries, centroid, sim, query_bits, k, lam=0.1, iters=5, n_threads=0, want_quantized=False):
        """searchNearestNeighbors from raw fp32 queries [nq, dim]: quantization on host threads pipelined with the sweeps
        (bbq_search_raw_batch).  Returns (idx, score, count[, qquant, qcorr])."""
        q = np.ascontiguousarray(queries, np.float32)
        cen = np.ascontiguousarray(centroid, np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim or cen.shape != (self.dim,):
            raise BBQError(ERR_DIM_MISMATCH, "查询向量维度与目标向量维度不匹配")
        nq = q.shape[0]
        kk = max(int(k), 0)
        idx = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        qq = np.zeros((nq, self.dim), np.uint8) if want_quantized else None
        qc = np.zeros((nq, 4), np.float64) if want_quantized else None
        bad = C.c_int32(-1)
        _chk(lib().bbq_search_raw_batch(self._h, nq, _ptr(q), _ptr(cen), sim, query_bits, lam, iters, n_threads, k, _ptr(idx), _ptr(sc), _ptr(cnt),
                                       _ptr(qq), _ptr(qc), C.byref(bad)))
        return (idx, sc, cnt, qq, qc) if want_quantized else (idx, sc, cnt)

    def score_rows(self, qquant, qcorr, query_bits, sim, row_begin=0, row_count=None):
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        if row_count is None:
            row_count = self.n - row_begin
        d = np.zeros(row_count, np.int32)
        s64 = np.zeros(row_count, np.float64)
        s32 = np.zeros(row_count, np.float32)
        _chk(lib().bbq_score_rows(self._h, _ptr(qq), _ptr(qc), query_bits, sim, row_begin, row_count, _ptr(d), _ptr(s64), _ptr(s32)))
        return d, s64, s32

    def score_ords(self, qquant, qcorr, query_bits, sim, ords, want=(True, True, True)):
        """bbq_score_ords: (qcdist, score64, score32) of the rows `ords` names, in the order given (any order, duplicates allowed);
        want = which of the three the library is asked for (the others come back None)"""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        o = _ords(ords)
        n = o.shape[0]
        d = np.zeros(n, np.int32) if want[0] else None
        s64 = np.zeros(n, np.float64) if want[1] else None
        s32 = np.zeros(n, np.float32) if want[2] else None
        _chk(lib().bbq_score_ords(self._h, _ptr(qq), _ptr(qc), query_bits, sim, _ptr(o), n, _ptr(d), _ptr(s64), _ptr(s32)))
        return d, s64, s32

    def score_ords_batch(self, qquant, qcorr, query_bits, sim, lists):
        """bbq_score_ords_batch: query q against its own list.  `lists` is a list of ord arrays, one per query, or (offsets, ords).
        Returns (qcdist, score64, score32), each indexed like the concatenated ords (list q at offsets[q] .. offsets[q+1]), and offsets."""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        off, o = _lists(lists, qq.shape[0])
        n = o.shape[0]
        d, s64, s32 = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.float32)
        _chk(lib().bbq_score_ords_batch(self._h, qq.shape[0], _ptr(qq), _ptr(qc), query_bits, sim, _ptr(off), _ptr(o), _ptr(d), _ptr(s64), _ptr(s32)))
        return d, s64, s32, off

    def search_ords_batch(self, qquant, qcorr, query_bits, sim, k, lists):
        """bbq_search_ords_batch: exact top-k of every query over its own list, visited in the order given.  `lists` as
        score_ords_batch takes them.  Returns a list of (idx, score) per query."""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        nq = qq.shape[0]
        off, o = _lists(lists, nq)
        kk = max(int(k), 0)
        idx = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        _chk(lib().bbq_search_ords_batch(self._h, nq, _ptr(qq), _ptr(qc), query_bits, sim, k, _ptr(off), _ptr(o), _ptr(idx), _ptr(sc), _ptr(cnt)))
        return [(idx[q, :cnt[q]], sc[q, :cnt[q]]) for q in range(nq)]

    def search_spans_batch(self, qquant, qcorr, query_bits, sim, k, spans):
        """bbq_search_spans_batch: exact top-k of every query over its own contiguous spans of rows [begin, end), ascending and
        disjoint.  `spans` is a list of (m, 2) arrays, one per query, or (offsets, spans).  Returns a list of (idx, score) per query
        and the status array (0: the device selected the answer, 1: the host replayed the heap over the device's scores)."""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        nq = qq.shape[0]
        off, sp = _spans(spans, nq)
        kk = max(int(k), 0)
        idx = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        status = np.zeros(nq, np.uint8)
        _chk(lib().bbq_search_spans_batch(self._h, nq, _ptr(qq), _ptr(qc), query_bits, sim, k, _ptr(off), _ptr(sp), _ptr(idx), _ptr(sc), _ptr(cnt),
                                         _ptr(status)))
        return [(idx[q, :cnt[q]], sc[q, :cnt[q]]) for q in range(nq)], status

    def search_spans_filtered_batch(self, qquant, qcorr, query_bits, sim, k, spans, flt):
        """bbq_search_spans_filtered_batch: search_spans_batch over the rows of the spans that `flt` (a Filter of this index) accepts;
        one filter serves every query of the call, flt=None accepts every row.  Returns what search_spans_batch returns; the status
        rule counts accepted rows."""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        nq = qq.shape[0]
        off, sp = _spans(spans, nq)
        kk = max(int(k), 0)
        idx = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        status = np.zeros(nq, np.uint8)
        _chk(lib().bbq_search_spans_filtered_batch(self._h, flt._h if flt is not None else None, nq, _ptr(qq), _ptr(qc), query_bits, sim, k,
                                                  _ptr(off), _ptr(sp), _ptr(idx), _ptr(sc), _ptr(cnt), _ptr(status)))
        return [(idx[q, :cnt[q]], sc[q, :cnt[q]]) for q in range(nq)], status

    def search_grouped_batch(self, qquant, qcorr, query_bits, sim, k, groups):
        """bbq_search_grouped_batch: the k best groups of `groups` (a Groups of this index) for every query, each through its best
        accepted row.  Returns a list of (idx, score, group) per query and the status array (0: the device selected the answer, 1: the
        host replayed the heap over the device's representatives)."""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        nq = qq.shape[0]
        kk = max(int(k), 0)
        idx = np.zeros((nq, kk), np.int32)
        grp = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        status = np.zeros(nq, np.uint8)
        _chk(lib().bbq_search_grouped_batch(self._h, groups._h if groups is not None else None, nq, _ptr(qq), _ptr(qc), query_bits, sim, k,
                                           _ptr(idx), _ptr(grp), _ptr(sc), _ptr(cnt), _ptr(status)))
        return [(idx[q, :cnt[q]], sc[q, :cnt[q]], grp[q, :cnt[q]]) for q in range(nq)], status

    def search_maxsim_batch(self, token_lists, query_bits, sim, k, groups):
        """bbq_search_maxsim_batch: the k best groups of `groups` (a Groups of this index) for every query, a query being a bag of token
        vectors and a group scoring the ordered f64 sum of its representatives' scores.  token_lists: per query a pair (qquant uint8
        [T, dim], qcorr float64 [T, 4]), T >= 1.  Returns a list of (group, score) per query and the status array (0: the device selected
        the answer, 1: the host replayed the heap over the device's sums)."""
        nq = len(token_lists)
        off, qq, qc = self._maxsim_tokens(token_lists)
        kk = max(int(k), 0)
        grp = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        status = np.zeros(nq, np.uint8)
        _chk(lib().bbq_search_maxsim_batch(self._h, groups._h if groups is not None else None, nq, _ptr(off), _ptr(qq), _ptr(qc), query_bits, sim, k,
                                          _ptr(grp), _ptr(sc), _ptr(cnt), _ptr(status)))
        return [(grp[q, :cnt[q]], sc[q, :cnt[q]]) for q in range(nq)], status

    def _maxsim_tokens(self, token_lists):
        """(vec_offsets int64 [nq + 1], qquant uint8 [vectors, dim], qcorr float64 [vectors, 4]) of per-query (qquant, qcorr) pairs"""
        nq = len(token_lists)
        off = np.zeros(nq + 1, np.int64)
        for q, (tq, _) in enumerate(token_lists):
            off[q + 1] = off[q] + np.asarray(tq).reshape(-1, self.dim).shape[0]
        qq = np.ascontiguousarray(np.concatenate([np.asarray(t[0], np.uint8).reshape(-1, self.dim) for t in token_lists]) if nq else np.zeros((0, self.dim), np.uint8))
        qc = np.ascontiguousarray(np.concatenate([np.asarray(t[1], np.float64).reshape(-1, 4) for t in token_lists]) if nq else np.zeros((0, 4), np.float64))
        if qc.shape[0] != qq.shape[0]:
            raise BBQError(ERR_INVALID_ARG, "one correction row per token vector")
        return off, qq, qc

    def score_maxsim_groups_batch(self, token_lists, query_bits, sim, groups, cand_lists):
        """bbq_score_maxsim_groups_batch: the MaxSim score of every candidate group of every query.  token_lists as search_maxsim_batch
        takes them; cand_lists: per query an int array of group numbers of `groups`, in any order, duplicates allowed (or (offsets,
        groups) as score_ords_batch takes its lists).  Returns (scores float32 [total], offsets int64 [nq + 1])."""
        nq = len(token_lists)
        off, qq, qc = self._maxsim_tokens(token_lists)
        coff, cg = _lists(cand_lists, nq)
        out = np.zeros(cg.shape[0], np.float32)
        _chk(lib().bbq_score_maxsim_groups_batch(self._h, groups._h if groups is not None else None, nq, _ptr(off), _ptr(qq), _ptr(qc), query_bits, sim,
                                                _ptr(coff), _ptr(cg), _ptr(out)))
        return out, coff

    def search_maxsim_groups_batch(self, token_lists, query_bits, sim, k, groups, cand_lists):
        """bbq_search_maxsim_groups_batch: the k best of every query's own candidate groups by their MaxSim score, visited in the order
        given.  Arguments as score_maxsim_groups_batch takes them.  Returns a list of (group, score) per query."""
        nq = len(token_lists)
        off, qq, qc = self._maxsim_tokens(token_lists)
        coff, cg = _lists(cand_lists, nq)
        kk = max(int(k), 0)
        grp = np.zeros((nq, kk), np.int32)
        sc = np.zeros((nq, kk), np.float32)
        cnt = np.zeros(nq, np.int64)
        _chk(lib().bbq_search_maxsim_groups_batch(self._h, groups._h if groups is not None else None, nq, _ptr(off), _ptr(qq), _ptr(qc), query_bits, sim, k,
                                                 _ptr(coff), _ptr(cg), _ptr(grp), _ptr(sc), _ptr(cnt)))
        return [(grp[q, :cnt[q]], sc[q, :cnt[q]]) for q in range(nq)]

    def _range_args(self, qquant, qcorr, thresholds):
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        th = np.ascontiguousarray(thresholds, np.float32).ravel()
        if qq.ndim != 2 or (qq.shape[0] and qq.shape[1] != self.dim):
            raise BBQError(ERR_DIM_MISMATCH, "查询向量维度与目标向量维度不匹配")
        if th.shape[0] != qq.shape[0]:
            raise BBQError(ERR_INVALID_ARG, "one threshold per query")
        return qq, qc, th

    def count_range_batch(self, qquant, qcorr, query_bits, sim, thresholds, row_filter=None):
        """bbq_count_range_batch: per query, the number of rows (of `row_filter`, a Filter of this index, if given) whose f32 score
        is >= its threshold"""
        qq, qc, th = self._range_args(qquant, qcorr, thresholds)
        cnt = np.zeros(qq.shape[0], np.int64)
        _chk(lib().bbq_count_range_batch(self._h, row_filter._h if row_filter is not None else None, qq.shape[0], _ptr(qq), _ptr(qc), query_bits, sim,
                                        _ptr(th), _ptr(cnt)))
        return cnt

    def search_range_batch(self, qquant, qcorr, query_bits, sim, thresholds, row_filter=None):
        """bbq_search_range_batch: (idx, score, offsets) - query q's answer, ascending by ord, is idx / score [offsets[q], offsets[q+1]).
        Counts first, allocates exactly, then fills."""
        qq, qc, th = self._range_args(qquant, qcorr, thresholds)
        nq = qq.shape[0]
        total = int(self.count_range_batch(qq, qc, query_bits, sim, th, row_filter).sum())
        off = np.zeros(nq + 1, np.int64)
        idx, sc = np.zeros(total, np.int32), np.zeros(total, np.float32)
        _chk(lib().bbq_search_range_batch(self._h, row_filter._h if row_filter is not None else None, nq, _ptr(qq), _ptr(qc), query_bits, sim,
                                         _ptr(th), total, _ptr(off), _ptr(idx), _ptr(sc)))
        return idx, sc, off

    def shard_scan_begin(self, qquant, qcorr, query_bits, sim, k, dev_packed_ptr, packed_cap, dev_offsets_ptr, dev_flags_ptr,
                         dev_answers_ptr=None, answers_stride=0):
        """enqueue the sweep of one batch (and its packing) and return; shard_scan_wait() later.  Two batches may be in flight."""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        _chk(lib().bbq_shard_scan_begin(self._h, qq.shape[0], _ptr(qq), _ptr(qc), query_bits, sim, k, dev_packed_ptr, packed_cap,
                                       dev_offsets_ptr, dev_flags_ptr, dev_answers_ptr, answers_stride))

    def shard_scan_wait(self):
        total = C.c_int64(0)
        _chk(lib().bbq_shard_scan_wait(self._h, C.byref(total)))
        return total.value

    def shard_list_cap(self, k):
        return lib().bbq_shard_list_cap(self._h, k)

    def shard_scan(self, qquant, qcorr, query_bits, sim, k, dev_packed_ptr, packed_cap, dev_offsets_ptr, dev_flags_ptr):
        """device pointers in (e.g. torch tensors' data_ptr()); returns the number of packed entries"""
        qq = np.ascontiguousarray(qquant, np.uint8)
        qc = np.ascontiguousarray(qcorr, np.float64)
        total = C.c_int64(0)
        _chk(lib().bbq_shard_scan(self._h, qq.shape[0], _ptr(qq), _ptr(qc), query_bits, sim, k, dev_packed_ptr, packed_cap,
                                 dev_offsets_ptr, dev_flags_ptr, C.byref(total)))
        return total.value


def merge_answers(blocks, n_queries, n_total, k, n_threads=1):
    """blocks[s]: uint64 array [>= n_queries, stride_s] of source s (bbq_shard_scan_begin's answers, in host memory).  Host only.
    Returns (idx [nq,k], score [nq,k], count [nq], status [nq]: 0 answered / 1 replay the lists / 2 dense path)."""
    bl = [np.ascontiguousarray(b, np.uint64) for b in blocks]
    n = len(bl)
    pp = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bl])
    strides = np.array([b.shape[1] for b in bl], np.int64)
    kk = max(int(k), 0)
    idx = np.zeros((n_queries, kk), np.int32)
    sc = np.zeros((n_queries, kk), np.float32)
    cnt = np.zeros(n_queries, np.int64)
    status = np.zeros(n_queries, np.uint8)
    _chk(lib().bbq_merge_answers(n, pp, _ptr(strides), n_queries, n_total, k, n_threads, _ptr(idx), _ptr(sc), _ptr(cnt), _ptr(status)))
    return idx, sc, cnt, status


def key_of_score(score):
    return int(lib().bbq_key_of_score(float(score)))


def range_key(threshold):
    """the key K with key_of_score(s) > K <=> s >= threshold for every non-NaN s (bbq_range_key; host only).  NaN raises."""
    k = C.c_uint32(0)
    _chk(lib().bbq_range_key(float(threshold), C.byref(k)))
    return int(k.value)


def file_shards(path_prefix):
    return int(lib().bbq_index_file_shards(os.fsencode(path_prefix)))


def file_info(path_prefix):
    n, dim, sim, cdp, rb = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_double(0), C.c_int64(0)
    _chk(lib().bbq_index_file_info(os.fsencode(path_prefix), C.byref(n), C.byref(dim), C.byref(sim), C.byref(cdp), C.byref(rb)))
    return {"n_rows": n.value, "dim": dim.value, "sim": sim.value, "centroid_dp": cdp.value, "row_base": rb.value}


def pack_mask(mask):
    """a bool mask over the rows -> the accept words of bbq_filter_create: row r is bit r & 63 of word r >> 6"""
    m = np.ascontiguousarray(mask, np.bool_).ravel()
    padded = np.zeros((m.shape[0] + 63) // 64 * 64, np.bool_)
    padded[:m.shape[0]] = m
    return np.ascontiguousarray(np.packbits(padded, bitorder="little")).view("<u8")


def filter_plan(mask, k_dev, first_segment_rows=4096, growth=8):
    """the segments a filtered call sweeps for this mask (bbq_filter_plan; host only): [(first chunk, chunks, slots per chunk)]"""
    words = pack_mask(mask)
    segs = np.zeros((64, 3), np.int64)
    n = C.c_int32(0)
    _chk(lib().bbq_filter_plan(_ptr(words), len(mask), k_dev, first_segment_rows, growth, 64, _ptr(segs), C.byref(n)))
    return [tuple(int(v) for v in row) for row in segs[:n.value]]


def _ords(ords):
    """ords as the C ABI takes them: int32, values beyond its range clipped to its ends (out of range for every index either way)"""
    return np.ascontiguousarray(np.asarray(ords, np.int64).ravel().clip(-2**31, 2**31 - 1), np.int32)


def _lists(lists, n_queries):
    """one ord list per query as the C ABI takes them: (offsets int64 [n_queries + 1], ords int32).  A TUPLE is the pair
    (offsets, ords), handed over as it is so that the library's own checks speak; any other sequence holds one array per query"""
    if isinstance(lists, tuple):
        if len(lists) != 2 or len(lists[0]) != n_queries + 1:
            raise BBQError(ERR_INVALID_ARG, "(offsets, ords) with one offset per query and one more")
        return np.ascontiguousarray(lists[0], np.int64), _ords(lists[1])
    if len(lists) != n_queries:
        raise BBQError(ERR_INVALID_ARG, "one ord list per query")
    arrs = [_ords(a) for a in lists]
    off = np.zeros(n_queries + 1, np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    return off, (np.concatenate(arrs) if arrs else np.zeros(0, np.int32))


def _spans(spans, n_queries):
    """one span list per query as the C ABI takes them: (offsets int64 [n_queries + 1], spans int64 [total, 2]).  A TUPLE is the pair
    (offsets, spans), handed over as it is so that the library's own checks speak; any other sequence holds one (m, 2) array per query"""
    if isinstance(spans, tuple):
        if len(spans) != 2 or len(spans[0]) != n_queries + 1:
            raise BBQError(ERR_INVALID_ARG, "(offsets, spans) with one offset per query and one more")
        return np.ascontiguousarray(spans[0], np.int64), np.ascontiguousarray(np.asarray(spans[1], np.int64).reshape(-1, 2))
    if len(spans) != n_queries:
        raise BBQError(ERR_INVALID_ARG, "one span list per query")
    arrs = [np.asarray(a, np.int64).reshape(-1, 2) for a in spans]
    off = np.zeros(n_queries + 1, np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    return off, np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 2), np.int64))


def update_winners(ords, n_rows):
    """the entries of an update block that take effect: positions into `ords`, ascending by ord, one per distinct ord - its last
    occurrence (bbq_update_winners; host only)"""
    o = _ords(ords)
    out = np.zeros(o.shape[0], np.int64)
    n = C.c_int64(0)
    _chk(lib().bbq_update_winners(_ptr(o), o.shape[0], int(n_rows), _ptr(out), out.shape[0], C.byref(n)))
    return out[:n.value]


def kept_rows(mask):
    """the old ord of every row a compaction by `mask` keeps, ascending (bbq_filter_kept_rows; host only)"""
    m = np.ascontiguousarray(mask, np.bool_).ravel()
    words = pack_mask(m)
    out = np.zeros(m.shape[0], np.int32)
    n = C.c_int64(0)
    _chk(lib().bbq_filter_kept_rows(_ptr(words), m.shape[0], _ptr(out), out.shape[0], C.byref(n)))
    return out[:n.value]


class Filter:
    """an accept set of one Index, resident on its device (bbq_filter_*): `mask_or_rows` is a bool mask of length index.n or
    an integer array of row ids (any order, duplicates allowed).  Read-only after creation; any number of searches may share it."""

    def __init__(self, index, mask_or_rows):
        a = np.asarray(mask_or_rows)
        h = C.c_void_p()
        if a.dtype == np.bool_:
            if a.ndim != 1 or a.shape[0] != index.n:
                raise BBQError(ERR_INVALID_ARG, "a filter mask has one entry per row of the index")
            words = pack_mask(a)
            _chk(lib().bbq_filter_create(index._h, _ptr(words), words.shape[0], C.byref(h)))
        else:
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise BBQError(ERR_INVALID_ARG, "a filter is a bool mask or an array of row ids")
            wide = np.asarray(a, np.int64).ravel()
            if wide.size and (wide.min() < -2**31 or wide.max() >= 2**31):
                raise BBQError(ERR_INVALID_ARG, "向量索引 %d 不存在" % int(wide.max() if wide.max() >= 2**31 else wide.min()))
            rows = np.ascontiguousarray(wide, np.int32)
            _chk(lib().bbq_filter_create_rows(index._h, _ptr(rows), rows.shape[0], C.byref(h)))
        self._h = h

    @property
    def count(self):
        """|A|: the rows the filter accepts"""
        return int(lib().bbq_filter_count(self._h)) if self._h else 0

    def close(self):
        if getattr(self, "_h", None):
            lib().bbq_filter_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def groups_plan(offsets, n_rows, mask=None):
    """which groups of `offsets` are live under `mask` (a bool mask over the rows, or None: every row) and where they rank among the
    live ones (bbq_groups_plan; host only): (slot int32 [n_groups], -1 for a group without an accepted row; L)"""
    off = np.ascontiguousarray(offsets, np.int64).ravel()
    n_groups = off.shape[0] - 1
    words = pack_mask(mask) if mask is not None else None
    if words is not None and len(mask) != n_rows:
        raise BBQError(ERR_INVALID_ARG, "a mask has one entry per row")
    slot = np.zeros(max(n_groups, 0), np.int32)
    live = C.c_int64(0)
    _chk(lib().bbq_groups_plan(_ptr(off) if off.shape[0] else None, n_groups, int(n_rows), _ptr(words), _ptr(slot), C.byref(live)))
    return slot, int(live.value)


def maxsim_reduce(rep_scores):
    """bbq_maxsim_reduce (host only): rep_scores float32 [n_vectors, n_groups], the representatives' scores of every token vector ->
    float32 [n_groups], each group's ordered f64 sum rounded once"""
    r = np.ascontiguousarray(rep_scores, np.float32)
    if r.ndim != 2:
        raise BBQError(ERR_INVALID_ARG, "rep_scores is [n_vectors, n_groups]")
    out = np.zeros(r.shape[1], np.float32)
    _chk(lib().bbq_maxsim_reduce(_ptr(r), r.shape[0], r.shape[1], _ptr(out)))
    return out


def maxsim_reduce_true(rep_true):
    """bbq_maxsim_reduce_true (host only): rep_true float64 [n_vectors, n_groups], every token vector's greatest true score of every
    group -> float64 [n_groups], each group's ordered f64 sum, a NaN sum as the one quiet NaN 0x7ff8000000000000"""
    r = np.ascontiguousarray(rep_true, np.float64)
    if r.ndim != 2:
        raise BBQError(ERR_INVALID_ARG, "rep_true is [n_vectors, n_groups]")
    out = np.zeros(r.shape[1], np.float64)
    _chk(lib().bbq_maxsim_reduce_true(_ptr(r), r.shape[0], r.shape[1], _ptr(out)))
    return out


def true_topk(scores, k, accept=None):
    """bbq_true_topk (host only): the exact search's ranking over one row of f64 scores - by true_key descending, equal keys by
    ascending row, a NaN below every number and written as 0x7ff8000000000000 - `accept` a bool mask over the rows or None: every row.
    Returns (rows int32 [m], scores float64 [m]), m = min(k, accepted rows)"""
    s = np.ascontiguousarray(scores, np.float64).ravel()
    words = None
    if accept is not None:
        m = np.ascontiguousarray(accept, np.bool_).ravel()
        if m.shape[0] != s.shape[0]:
            raise BBQError(ERR_INVALID_ARG, "a mask has one entry per row")
        words = pack_mask(m)
    cap = max(min(int(k), s.shape[0]), 0)
    idx = np.zeros(cap, np.int32)
    out = np.zeros(cap, np.float64)
    n = C.c_int64(0)
    _chk(lib().bbq_true_topk(_ptr(s), s.shape[0], _ptr(words), int(k), _ptr(idx), _ptr(out), C.byref(n)))
    return idx[:n.value], out[:n.value]


def _raw_tokens(token_lists, dim):
    """(vec_offsets int64 [nq + 1], queries float32 [vectors, dim]) of per-query raw fp32 token arrays [T, dim]"""
    arrs = [np.asarray(t, np.float32).reshape(-1, dim) for t in token_lists]
    off = np.zeros(len(arrs) + 1, np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    return off, np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, dim), np.float32))


def maxsim_token_block():
    """bbq_maxsim_token_block: the tokens of a query a MaxSim search works through at a time"""
    return int(lib().bbq_maxsim_token_block())


class Groups:
    """the groups of one Index, resident on its device (bbq_groups_*): group g is the rows [offsets[g], offsets[g + 1]); `row_filter` (a
    Filter of the index, or None) says which rows exist for a grouped search.  Read-only after creation; any number of searches may
    share it, and the filter may be closed before it."""

    def __init__(self, index, offsets, row_filter=None):
        off = np.ascontiguousarray(offsets, np.int64).ravel()
        h = C.c_void_p()
        _chk(lib().bbq_groups_create(index._h, _ptr(off) if off.shape[0] else None, off.shape[0] - 1, row_filter._h if row_filter is not None else None,
                                    C.byref(h)))
        self._h = h

    @property
    def count(self):
        """the number of groups, empty ones included"""
        return int(lib().bbq_groups_count(self._h)) if self._h else 0

    @property
    def live(self):
        """L: the groups with at least one accepted row"""
        return int(lib().bbq_groups_live(self._h)) if self._h else 0

    def close(self):
        if getattr(self, "_h", None):
            lib().bbq_groups_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Vectors:
    """the original fp32 vectors resident on one GPU (bbq_vectors_*): the `vectors` argument of the reference's
    oversample selectors (src/topKSelector.ts:29-115)"""

    def __init__(self, vectors, device=0):
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim != 2:
            raise BBQError(ERR_INVALID_ARG, "vectors must be [n, dim]")
        self.n, self.dim = int(v.shape[0]), int(v.shape[1])
        h = C.c_void_p()
        _chk(lib().bbq_vectors_create(_ptr(v), self.n, self.dim, device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().bbq_vectors_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, vectors):
        """bbq_vectors_append: the fp32 rows of an appended block get the next ords"""
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise BBQError(ERR_DIM_MISMATCH, "向量维度不匹配")
        _chk(lib().bbq_vectors_append(self._h, _ptr(v), v.shape[0]))
        self.n = int(lib().bbq_vectors_size(self._h))

    def compact(self, flt):
        """bbq_vectors_compact: the fp32 rows follow a compaction of the index by the same filter"""
        _chk(lib().bbq_vectors_compact(self._h, flt._h if flt is not None else None))
        self.n = int(lib().bbq_vectors_size(self._h))

    def update(self, ords, vectors):
        """bbq_vectors_update: the fp32 rows follow an update of the index - `vectors` become the rows `ords` (the last of equal ords wins)"""
        o = _ords(ords)
        v = np.ascontiguousarray(vectors, np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim or o.shape[0] != v.shape[0]:
            raise BBQError(ERR_DIM_MISMATCH, "向量维度不匹配")
        _chk(lib().bbq_vectors_update(self._h, _ptr(o), _ptr(v), v.shape[0]))

    def rerank_scores(self, queries, rows_per_query, true_sim=1):
        """computeSimilarity(queries[q], vectors[r]) for r in rows_per_query[q]; returns a list of f64 arrays"""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise BBQError(ERR_DIM_MISMATCH, "向量维度不匹配")
        lists = [np.ascontiguousarray(r, np.int32) for r in rows_per_query]
        if len(lists) != q.shape[0]:
            raise BBQError(ERR_INVALID_ARG, "one candidate list per query")
        off = np.zeros(len(lists) + 1, np.int64)
        off[1:] = np.cumsum([a.shape[0] for a in lists])
        rows = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        rows = np.ascontiguousarray(rows, np.int32)
        out = np.zeros(int(off[-1]), np.float64)
        _chk(lib().bbq_rerank_scores(self._h, q.shape[0], _ptr(q), _ptr(off), _ptr(rows), true_sim, _ptr(out)))
        return [out[off[i]:off[i + 1]] for i in range(len(lists))]

    def set_option(self, name, value):
        """bbq_vectors_set_option: "exact_slab_rows", the rows search_batch scores between two select passes (0: automatic)"""
        _chk(lib().bbq_vectors_set_option(self._h, name.encode(), int(value)))

    def search_batch(self, queries, k, true_sim=1, row_filter=None):
        """bbq_vectors_search_batch: the exact top-k of every raw fp32 query over the rows (those `row_filter` accepts), the
        reference's getTrueTopK on the device.  Returns (rows int32 [nq, m], true scores float64 [nq, m], counts int64 [nq]), m = min(k,
        rows of the handle) - a k beyond the rows asks for the same answer; row q holds counts[q] = min(k, accepted rows) answers,
        best first"""
        q = np.ascontiguousarray(queries, np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise BBQError(ERR_DIM_MISMATCH, "向量维度不匹配")
        k = min(int(k), self.n)
        nq, kk = q.shape[0], max(k, 0)
        idx = np.full((nq, kk), -1, np.int32)
        out = np.zeros((nq, kk), np.float64)
        cnt = np.zeros(max(nq, 1), np.int64)
        _chk(lib().bbq_vectors_search_batch(self._h, row_filter._h if row_filter is not None else None, nq, _ptr(q), int(true_sim), int(k), _ptr(idx), _ptr(out),
                                            _ptr(cnt)))
        return idx, out, cnt[:nq]

    def rerank_maxsim_groups_batch(self, token_lists, groups, cand_lists, true_sim=1):
        """bbq_rerank_maxsim_groups_batch: the exact MaxSim score of every candidate group of every query.  token_lists: per query its
        raw fp32 token vectors [T, dim], T >= 1; cand_lists: per query an int array of group numbers of `groups`, in any order,
        duplicates allowed (or (offsets, groups) as score_ords_batch takes its lists).  Returns (true scores float64 [total], offsets
        int64 [nq + 1])."""
        nq = len(token_lists)
        off, q = _raw_tokens(token_lists, self.dim)
        coff, cg = _lists(cand_lists, nq)
        out = np.zeros(cg.shape[0], np.float64)
        _chk(lib().bbq_rerank_maxsim_groups_batch(self._h, groups._h if groups is not None else None, nq, _ptr(off), _ptr(q), true_sim, _ptr(coff), _ptr(cg),
                                                 _ptr(out)))
        return out, coff


def search_maxsim_rerank_batch(index, vectors, groups, raw_token_lists, token_lists, query_bits, sim, k, factor, selector=0, true_sim=1):
    """bbq_search_maxsim_rerank_batch: the MaxSim search with k * factor on `index`, the exact MaxSim scores of the returned groups on
    `vectors`, the reference's selector (0 heap, 1 sort).  raw_token_lists: per query its raw fp32 token vectors [T, dim]; token_lists:
    the same tokens quantized, as Index.search_maxsim_batch takes them.  Returns a list of (group int32, quantized f32, true f64) per query."""
    nq = len(token_lists)
    if len(raw_token_lists) != nq:
        raise BBQError(ERR_INVALID_ARG, "one raw token array per query")
    off, qq, qc = index._maxsim_tokens(token_lists)
    roff, q = _raw_tokens(raw_token_lists, index.dim)
    if roff.tolist() != off.tolist():
        raise BBQError(ERR_INVALID_ARG, "as many raw token vectors as quantized ones, query by query")
    kk = max(int(k), 0)
    grp = np.zeros((nq, kk), np.int32)
    qs = np.zeros((nq, kk), np.float32)
    ts = np.zeros((nq, kk), np.float64)
    cnt = np.zeros(nq, np.int64)
    _chk(lib().bbq_search_maxsim_rerank_batch(index._h, vectors._h if vectors is not None else None, groups._h if groups is not None else None, nq, _ptr(off),
                                             _ptr(q), _ptr(qq), _ptr(qc), query_bits, sim, k, factor, selector, true_sim, _ptr(grp), _ptr(qs), _ptr(ts), _ptr(cnt)))
    return [(grp[i, :cnt[i]], qs[i, :cnt[i]], ts[i, :cnt[i]]) for i in range(nq)]


def search_rerank_batch(index, vectors, queries, qquant, qcorr, query_bits, sim, k, factor, selector=0, true_sim=1):
    """oversample k*factor on `index`, exact true scores on `vectors`, the reference's selector (0 heap, 1 sort).
    Returns (idx [nq,k], quantized f32 [nq,k], true f64 [nq,k], counts)."""
    q = np.ascontiguousarray(queries, np.float32)
    qq = np.ascontiguousarray(qquant, np.uint8)
    qc = np.ascontiguousarray(qcorr, np.float64)
    nq = qq.shape[0]
    if nq and (qq.shape[1] != index.dim or q.shape[1] != index.dim):
        raise BBQError(ERR_DIM_MISMATCH, "查询向量维度与目标向量维度不匹配")
    kk = max(int(k), 0)
    idx = np.zeros((nq, kk), np.int32)
    qs = np.zeros((nq, kk), np.float32)
    ts = np.zeros((nq, kk), np.float64)
    cnt = np.zeros(nq, np.int64)
    _chk(lib().bbq_search_rerank_batch(index._h, vectors._h, nq, _ptr(q), _ptr(qq), _ptr(qc), query_bits, sim, k, factor,
                                       selector, true_sim, _ptr(idx), _ptr(qs), _ptr(ts), _ptr(cnt)))
    return idx, qs, ts, cnt


def replay(lists, n_total, k):
    """lists: sequence of uint64 numpy arrays (ascending shard order).  Host only - needs no device."""
    arrs = [np.ascontiguousarray(a, np.uint64) for a in lists]
    n = len(arrs)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
    counts = np.array([a.shape[0] for a in arrs], np.int64)
    kk = max(int(k), 0)
    idx = np.zeros(kk, np.int32)
    sc = np.zeros(kk, np.float32)
    cnt = C.c_int64(0)
    _chk(lib().bbq_replay(n, ptrs, _ptr(counts), n_total, k, _ptr(idx), _ptr(sc), C.byref(cnt)))
    return idx[:cnt.value], sc[:cnt.value]


def replay_batch(packed, offsets, n_queries, n_total, k, n_threads=1):
    """packed[s]: uint64 array of source s (ascending shard order), offsets[s]: int64 [n_queries+1].  Host only."""
    pk = [np.ascontiguousarray(a, np.uint64) for a in packed]
    of = [np.ascontiguousarray(a, np.int64) for a in offsets]
    n = len(pk)
    pp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in pk])
    po = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in of])
    kk = max(int(k), 0)
    idx = np.zeros((n_queries, kk), np.int32)
    sc = np.zeros((n_queries, kk), np.float32)
    cnt = np.zeros(n_queries, np.int64)
    _chk(lib().bbq_replay_batch(n, pp, po, n_queries, n_total, k, n_threads, _ptr(idx), _ptr(sc), _ptr(cnt)))
    return idx, sc, cnt
