"""ctypes binding of libcubitgpu.so (include/cubit_gpu.h) and libcubit_datagen.so.

The HIP library is the product: nothing here falls back to a CPU implementation. If the
shared object is missing the import raises, so a GPU run can never silently pass on
something other than the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_ROOT = Path(__file__).resolve().parent.parent          # duckdb-cubit_amd/
LIB_DIR = PKG_ROOT / "lib"
GPU_LIB = LIB_DIR / "libcubitgpu.so"
GEN_LIB = LIB_DIR / "libcubit_datagen.so"
SCAN_LIB = LIB_DIR / "libcubit_scan.so"

# status codes / constants (include/cubit_gpu.h)
OK = 0
ERR_INVALID, ERR_HIP, ERR_OOM, ERR_UNSUPPORTED, ERR_CAPACITY, ERR_DEVICE = 1, 2, 3, 4, 5, 6
TYPE_INT32, TYPE_INT64 = 0, 1
# the T of BITPACKING segments (cubit_table_add_bitpacked_column): numpy dtype → CUBIT_TYPE_*
TYPE_INT8, TYPE_INT16, TYPE_UINT8, TYPE_UINT16, TYPE_UINT32, TYPE_UINT64 = 2, 3, 4, 5, 6, 7
SEGMENT_TYPES = {"int8": TYPE_INT8, "int16": TYPE_INT16, "int32": TYPE_INT32, "int64": TYPE_INT64,
                 "uint8": TYPE_UINT8, "uint16": TYPE_UINT16, "uint32": TYPE_UINT32, "uint64": TYPE_UINT64,
                 "bool": TYPE_INT8}
# FLOAT / DOUBLE columns hold IEEE bit patterns; constants, keys, update values and probed values
# cross the ABI as those patterns in an int64 (FLOAT: the 32-bit pattern, zero-extended)
TYPE_FLOAT, TYPE_DOUBLE = 8, 9
# VARCHAR columns hold int32 codes of an order-preserving dictionary (cubit_dict); their filter
# constants and index keys are addresses of cubit_string structs (filters.string_ref)
TYPE_VARCHAR = 10
# HUGEINT / UHUGEINT columns are dictionary columns over the values' 16-byte order keys
# (cubit_key128 / filters.key128): the type codes name the key encoding
TYPE_INT128, TYPE_UINT128 = 11, 12
# per-segment codecs of cubit_table_add_segment_column
CODEC_UNCOMPRESSED, CODEC_CONSTANT, CODEC_RLE, CODEC_BITPACKING = 0, 1, 2, 3
COLUMN_TYPES = dict(SEGMENT_TYPES, float32=TYPE_FLOAT, float64=TYPE_DOUBLE)


def fp_bits(values, type_: int):
    """Values of a FLOAT / DOUBLE column as the int64 bit patterns the ABI carries; other types'
    values as int64."""
    import numpy as _np
    if type_ == TYPE_FLOAT:
        return _np.ascontiguousarray(_np.asarray(values, dtype=_np.float32)).view(_np.uint32).astype(_np.int64)
    if type_ == TYPE_DOUBLE:
        return _np.ascontiguousarray(_np.asarray(values, dtype=_np.float64)).view(_np.int64)
    return _np.ascontiguousarray(_np.asarray(values, dtype=_np.int64))
CMP_EQ, CMP_NE, CMP_LT, CMP_LE, CMP_GT, CMP_GE = range(6)
FILTER_CONSTANT, FILTER_IS_NULL, FILTER_IS_NOT_NULL, FILTER_OR, FILTER_AND = range(5)
INDEX_RANGE, INDEX_EQUALITY, INDEX_BINS, INDEX_SLICED = 0, 1, 2, 3
SUM_GATHER_B = 1
SUM_NO_ZONEMAP = 2
SUM_PACKED_A = 4
SUM_PLAIN_A = 8
SUM_FROM_SLICES, SUM_FROM_COLUMN = 16, 32
AGG_SUM, AGG_MIN, AGG_MAX = 1, 2, 4
AGG_ALL = AGG_SUM | AGG_MIN | AGG_MAX
AGG_FROM_SLICES, AGG_FROM_COLUMN, AGG_NO_ZONEMAP = 16, 32, 64
AGG_MAX_GROUP_COLS, AGG_MAX_GROUPS = 2, 256
SELECT_RANK, SELECT_RANK_DESC, SELECT_QUANTILE = 0, 1, 2
SELECT_DESC_ROWS = 1
SELECT_FROM_SLICES, SELECT_FROM_COLUMN, SELECT_NO_ZONEMAP = 16, 32, 64
OP_AND, OP_OR, OP_ANDNOT = -1, -2, -3
SCAN_COUNT_ONLY = 1
SCAN_ORDERED = 2
SCAN_CHECK_CAPACITY = 4  # synchronise; ERR_CAPACITY when the count exceeds the buffer
SCAN_NO_ZONEMAP = 8  # evaluate every zone (the zonemap skip off; results are identical)
DECODE_AUTO, DECODE_PAIRS, DECODE_RUNS, DECODE_LOOKBACK = 0, 1, 2, 3
DECODE_PREFIXED = 4  # reported only (cubit_ctx_last_decode_kernel): one index bitvector, offsets from its zone counts
FORM_POSTFIX, FORM_CONJ, FORM_DNF, FORM_CNF = range(4)  # cubit_table_last_form: the kernel template the last program ran in


class FilterNode(C.Structure):
    """cubit_filter_node — one prefix-order node of a TableFilter tree."""

    _fields_ = [
        ("kind", C.c_int32),
        ("cmp", C.c_int32),
        ("column", C.c_int32),
        ("n_children", C.c_int32),
        ("constant", C.c_int64),
    ]


class Txn(C.Structure):
    """cubit_txn — DuckDB TransactionData{start_time, transaction_id}."""

    _fields_ = [("start_time", C.c_uint64), ("transaction_id", C.c_uint64)]


class CubitError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"cubit error {code}: {msg}")
        self.code = code


_P = C.c_void_p
_U64 = C.c_uint64
_I64 = C.c_int64
_I32 = C.c_int32
_U32 = C.c_uint32

# name -> (restype, argtypes)
GPU_SIGNATURES = {
    "cubit_abi_version": (C.c_int, []),
    "cubit_vector_size": (C.c_int, []),
    "cubit_row_group_size": (C.c_int, []),
    "cubit_padded_words": (_U64, [_U64]),
    "cubit_last_error": (C.c_char_p, []),
    "cubit_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "cubit_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "cubit_ctx_destroy": (C.c_int, [_P]),
    "cubit_ctx_set_stream": (C.c_int, [_P, _P]),
    "cubit_ctx_enable_timing": (C.c_int, [_P, C.c_int]),
    "cubit_last_kernel_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "cubit_ctx_timing_reset": (C.c_int, [_P]),
    "cubit_ctx_kernel_times": (C.c_int, [_P, C.POINTER(C.c_float), _U32, C.POINTER(_U32)]),
    "cubit_ctx_set_repeat": (C.c_int, [_P, _U32]),
    "cubit_ctx_repeat_time": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(_U32)]),
    "cubit_ctx_check": (C.c_int, [_P]),
    "cubit_ctx_last_tiles": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_U32), C.POINTER(_U64)]),
    "cubit_dev_alloc": (C.c_int, [_P, _U64, C.POINTER(_P)]),
    "cubit_dev_free": (C.c_int, [_P, _P]),
    "cubit_memcpy_h2d": (C.c_int, [_P, _P, _P, _U64]),
    "cubit_memcpy_d2h": (C.c_int, [_P, _P, _P, _U64]),
    "cubit_memset_d": (C.c_int, [_P, _P, C.c_int, _U64]),
    "cubit_memcpy_d2d": (C.c_int, [_P, _P, _P, _U64]),
    "cubit_sync": (C.c_int, [_P]),
    "cubit_copy_stream_create": (C.c_int, [_P, C.POINTER(_P)]),
    "cubit_copy_stream_destroy": (C.c_int, [_P, _P]),
    "cubit_memcpy_d2h_stream": (C.c_int, [_P, _P, _P, _P, _U64]),
    "cubit_memcpy_d2h_async": (C.c_int, [_P, _P, _P, _P, _U64]),
    "cubit_copy_stream_sync": (C.c_int, [_P, _P]),
    "cubit_copy_event_record": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "cubit_copy_event_sync": (C.c_int, [_P, _P]),
    "cubit_copy_stream_wait_event": (C.c_int, [_P, _P, _P]),
    "cubit_copy_event_destroy": (C.c_int, [_P, _P]),
    "cubit_build_bitvector": (C.c_int, [_P, _P, C.c_int, _P, _U64, C.c_int, _I64, _P]),
    "cubit_bitslice_build": (C.c_int, [_P, _P, C.c_int, _P, _U64, _I64, _U32, _P]),
    "cubit_bitslice_compare": (C.c_int, [_P, _P, _U32, _P, _U64, _U64, _U64, C.c_int, _P]),
    "cubit_dict_create": (C.c_int, [_P, _P, _U64, C.POINTER(_P)]),
    "cubit_dict_destroy": (C.c_int, [_P]),
    "cubit_dict_size": (C.c_int, [_P, C.POINTER(_U64)]),
    "cubit_dict_entry": (C.c_int, [_P, _U64, C.POINTER(_P), C.POINTER(_U64)]),
    "cubit_dict_encode": (C.c_int, [_P, _P, _P, _U64, _P, _P]),
    "cubit_dict_lookup": (C.c_int, [_P, _P, _U64, C.POINTER(_U64), C.POINTER(C.c_int)]),
    "cubit_dict_encode_device": (C.c_int, [_P, _P, _P, _P, _U64, _P, _P]),
    "cubit_table_add_dict_column": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "cubit_bitvector_eval": (
        C.c_int,
        [_P, C.POINTER(_P), _U32, _U32, C.POINTER(_I32), _U32, _U64, _I64, _P, _U64, _P, _P, _U32],
    ),
    "cubit_gather": (C.c_int, [_P, _P, C.c_int, _P, _P, _U64, _I64, _P]),
    "cubit_narrow_i32": (C.c_int, [_P, _P, _P, _U64, C.c_int64, _P]),
    "cubit_narrow_i32_checked": (C.c_int, [_P, _P, _P, _U64, C.c_int64, _P, _P]),
    "cubit_narrow_checked": (C.c_int, [_P, _P, _P, _U64, C.c_int64, C.c_int, _P, _P]),
    "cubit_gather_sum_product": (C.c_int, [_P, _P, _P, _P, _P, _U64, _I64, _P]),
    "cubit_table_create": (C.c_int, [_P, _U64, _I64, C.POINTER(_P)]),
    "cubit_table_destroy": (C.c_int, [_P]),
    "cubit_table_info": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(_I64), C.POINTER(_P)]),
    "cubit_table_add_column": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int]),
    "cubit_table_add_bitpacked_column": (C.c_int, [_P, C.c_int, C.c_int, _P, _U64, _P, _P, _U32, _P]),
    "cubit_table_add_rle_column": (C.c_int, [_P, C.c_int, C.c_int, _P, _U64, _P, _P, _U32, _P]),
    "cubit_table_add_segment_column": (C.c_int, [_P, C.c_int, C.c_int, _P, _U64, _P, _P, _P, _P, _U32, _P]),
    "cubit_table_build_index": (C.c_int, [_P, C.c_int, C.c_int, _P, _U32]),
    "cubit_table_build_index_quantiles": (C.c_int, [_P, C.c_int, C.c_int, _U32, _P, _U32, C.POINTER(_U32)]),
    "cubit_table_index_info": (C.c_int, [_P, C.c_int, C.POINTER(_U32), C.POINTER(_U64)]),
    "cubit_table_set_deletes": (C.c_int, [_P, _P, _P, _U64]),
    "cubit_table_set_updates": (C.c_int, [_P, C.c_int, _P, _P, _P, _U64]),
    "cubit_table_set_updates_nullable": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _U64]),
    "cubit_table_scan": (
        C.c_int,
        [_P, C.POINTER(FilterNode), _U32, C.POINTER(Txn), _P, _U64, _P, _U32],
    ),
    "cubit_table_scan_tiles": (
        C.c_int,
        [_P, C.POINTER(FilterNode), _U32, C.POINTER(Txn), _P, _U64, _P, _U32, _P, _U32, C.POINTER(_U32),
         C.POINTER(_U64)],
    ),
    "cubit_table_probe": (C.c_int, [_P, C.c_int, C.POINTER(Txn), _P, _P, _U64, _P]),
    "cubit_table_probe_validity": (C.c_int, [_P, C.c_int, C.POINTER(Txn), _P, _P, _U64, _P, _P]),
    "cubit_table_last_plan": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(_U32)]),
    "cubit_table_last_form": (C.c_int, [_P, C.POINTER(_U32)]),
    "cubit_table_set_derived_budget": (C.c_int, [_P, _U64]),
    "cubit_table_derived_stats": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(_U64), C.POINTER(_U64)]),
    "cubit_table_set_derived_chain_cost": (C.c_int, [_P, _U64]),
    "cubit_table_set_derived_chain_cost_pooled": (C.c_int, [_P, _U64]),
    "cubit_table_derived_chain_stats": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(_U64)]),
    "cubit_table_derived_pool_stats": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(_U64)]),
    "cubit_table_use_row_lists": (C.c_int, [_P, C.c_int]),
    "cubit_table_row_list_stats": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(_U64), C.POINTER(_U64)]),
    "cubit_table_estimate_rows": (C.c_int, [_P, C.POINTER(FilterNode), _U32, C.POINTER(_U64)]),
    "cubit_table_last_zones": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(_U32)]),
    "cubit_table_use_packed_filter": (C.c_int, [_P, C.c_int]),
    "cubit_table_last_packed": (C.c_int, [_P, C.POINTER(_U32)]),
    "cubit_table_use_sliced": (C.c_int, [_P, C.c_int]),
    "cubit_table_last_sliced": (C.c_int, [_P, C.POINTER(_U32)]),
    "cubit_table_use_narrowing": (C.c_int, [_P, C.c_int]),
    "cubit_table_last_narrowed": (C.c_int, [_P, C.POINTER(_U32)]),
    "cubit_table_last_k0_order": (C.c_int, [_P, C.POINTER(C.c_int32), _U32, C.POINTER(_U32)]),
    "cubit_table_column_changed": (C.c_int, [_P, C.c_int]),
    "cubit_table_column_statistics": (C.c_int, [_P, C.c_int, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(C.c_int),
                                                C.POINTER(C.c_int)]),
    "cubit_table_sum_product": (C.c_int, [_P, _P, _U32, _P, C.c_int, C.c_int, _P, _P, _U32]),
    "cubit_table_last_sum_product": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(_U32)]),
    "cubit_table_sum_product_grouped": (C.c_int, [_P, _P, _U32, _P, C.c_int, C.c_int, _P, _U32, _U32, _P, _U32]),
    "cubit_bitslice_sum_product": (C.c_int, [_P, _P, _U32, _P, _I64, _P, _U32, _P, _I64, _P, _U64, _P]),
    "cubit_table_last_sum_decode": (C.c_int, [_P, C.POINTER(_U32)]),
    "cubit_table_last_sum_packed": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "cubit_table_aggregate": (C.c_int, [_P, _P, _U32, _P, C.c_int, _U32, _P]),
    "cubit_table_last_aggregate": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "cubit_table_aggregate_groups": (C.c_int, [_P, _P, _U32, _P, _P, _U32, C.POINTER(_U32)]),
    "cubit_table_aggregate_grouped": (C.c_int, [_P, _P, _U32, _P, C.c_int, _P, _U32, _U32, _P, _U32]),
    "cubit_table_last_grouped": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(_U32), C.POINTER(_U32)]),
    "cubit_bitslice_aggregate": (C.c_int, [_P, _P, _U32, _P, _P, _U64, C.c_int, _I64, _U32, _P]),
    "cubit_table_select": (C.c_int, [_P, _P, _U32, _P, C.c_int, C.c_int, _U64, C.c_double, _U32, _P]),
    "cubit_table_last_select": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(_U32)]),
    "cubit_bitslice_select": (C.c_int, [_P, _P, _U32, _P, _P, _U64, C.c_int, _I64, C.c_int, _U64, C.c_double, _P]),
    "cubit_table_select_grouped": (C.c_int, [_P, _P, _U32, _P, C.c_int, _P, _U32, C.c_int, _U64, C.c_double, _U32, _P,
                                             _U32]),
    "cubit_table_last_select_grouped": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(_U32), C.POINTER(_U32),
                                                  C.POINTER(_U32)]),
    "cubit_bitslice_select_grouped": (C.c_int, [_P, _P, _U32, _P, _P, _P, _U32, _U64, C.c_int, _I64, C.c_int, _U64,
                                                C.c_double, _P]),
    "cubit_table_top_n": (C.c_int, [_P, _P, _U32, _P, C.c_int, _U64, _U32, _P, _U64, _P, _P]),
    "cubit_table_column_data": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int)]),
    "cubit_table_set_inserts": (C.c_int, [_P, _P, _P, _P, _U64]),
    "cubit_table_append": (C.c_int, [_P, _U64, _P, _P, _P, C.c_uint32, _U64]),
    "cubit_ctx_set_decode_kernel": (C.c_int, [_P, C.c_int]),
    "cubit_ctx_set_lookback_spins": (C.c_int, [_P, C.c_uint32]),
    "cubit_ctx_set_compute_units": (C.c_int, [_P, C.c_int]),
    "cubit_ctx_compute_units": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cubit_ctx_last_grid": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(_U32)]),
    "cubit_host_alloc": (C.c_int, [_P, _U64, C.POINTER(_P)]),
    "cubit_host_free": (C.c_int, [_P, _P]),
    "cubit_ctx_last_decode_kernel": (C.c_int, [_P, _P]),
    "cubit_ctx_last_decode_from_list": (C.c_int, [_P, _P]),
    "cubit_table_merge_updates": (C.c_int, [_P, C.c_int, _U64, _P]),
    "cubit_table_sync_column": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, _U64, C.POINTER(_U64), C.POINTER(C.c_int)]),
    "cubit_table_save_index": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p]),
    "cubit_table_load_index": (C.c_int, [_P, C.c_int, C.c_char_p]),
}

GEN_SIGNATURES = {
    "cubit_tpch_orders": (_I64, [C.c_double]),
    "cubit_tpch_lineitem_rows": (_I64, [C.c_double, _I64, _I64, C.c_int]),
    "cubit_tpch_lineitem_gen": (_I64, [C.c_double, _I64, _I64, _P, _P, _P, _P, C.c_int]),
    "cubit_splitmix64": (_U64, [_U64, _U64]),
    "cubit_synth_uniform_i32": (C.c_int, [_U64, _U64, _U64, _U32, _P, C.c_int]),
    "cubit_bitpack_for": (_U32, [_P, C.c_int, _U64, _U64, _P, _U64, _P, _P, _U32, C.POINTER(_U64), C.c_int]),
}

SCAN_SIGNATURES = {
    "cubit_scan_last_error": (C.c_char_p, []),
    "cubit_scan_init_global": (C.c_int, [_P, C.POINTER(_U64), _U32, C.POINTER(_U64), _U32, C.POINTER(FilterNode),
                                         _U32, C.POINTER(Txn), C.POINTER(_P)]),
    "cubit_scan_init_global_multi": (C.c_int, [C.POINTER(_P), _U32, C.POINTER(_U64), _U32, C.POINTER(_U64), _U32,
                                               C.POINTER(FilterNode), _U32, C.POINTER(Txn), C.POINTER(_P)]),
    "cubit_scan_cardinality_multi": (C.c_int, [C.POINTER(_P), _U32, C.POINTER(_U64), C.POINTER(_U64)]),
    "cubit_scan_statistics_multi": (C.c_int, [C.POINTER(_P), _U32, _U64, C.POINTER(_I64), C.POINTER(_I64),
                                              C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cubit_scan_max_threads": (C.c_int, [_P, C.POINTER(_U64)]),
    "cubit_scan_init_local": (C.c_int, [_P, C.POINTER(_P)]),
    "cubit_scan_function": (C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(_U64)]),
    "cubit_scan_function_validity": (C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_U64)]),
    "cubit_scan_batch_index": (C.c_int, [_P, _P, C.POINTER(_U64)]),
    "cubit_scan_progress": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "cubit_scan_decodes": (C.c_int, [_P, C.POINTER(_U32)]),
    "cubit_scan_cardinality": (C.c_int, [_P, C.POINTER(_U64), C.POINTER(_U64)]),
    "cubit_scan_statistics": (C.c_int, [_P, _U64, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    "cubit_scan_release_cached": (C.c_int, [C.POINTER(_U64), C.POINTER(_U64)]),
    "cubit_scan_local_destroy": (C.c_int, [_P]),
    "cubit_scan_destroy": (C.c_int, [_P]),
}

_gpu = None
_gen = None
_scan = None


def _bind(lib, sigs):
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def gpu_lib():
    """The HIP library. Raises if it was not built (run __graft_entry__.build())."""
    global _gpu
    if _gpu is None:
        if not GPU_LIB.exists():
            raise RuntimeError(f"{GPU_LIB} is missing: build it with `make -C {PKG_ROOT}` "
                               "(or __graft_entry__.build()); there is no CPU fallback")
        _gpu = _bind(C.CDLL(str(GPU_LIB)), GPU_SIGNATURES)
    return _gpu


def gen_lib():
    global _gen
    if _gen is None:
        if not GEN_LIB.exists():
            raise RuntimeError(f"{GEN_LIB} is missing: build it with `make -C {PKG_ROOT}`")
        _gen = _bind(C.CDLL(str(GEN_LIB)), GEN_SIGNATURES)
    return _gen


def scan_lib():
    """libcubit_scan.so: the TableFunction mirror (loads libcubitgpu.so first)."""
    global _scan
    if _scan is None:
        gpu_lib()
        if not SCAN_LIB.exists():
            raise RuntimeError(f"{SCAN_LIB} is missing: build it with `make -C {PKG_ROOT}`")
        _scan = _bind(C.CDLL(str(SCAN_LIB)), SCAN_SIGNATURES)
    return _scan


def check_scan(rc: int) -> None:
    if rc != OK:
        msg = scan_lib().cubit_scan_last_error()
        raise CubitError(rc, msg.decode() if msg else "")


def check(rc: int) -> None:
    if rc != OK:
        msg = gpu_lib().cubit_last_error()
        raise CubitError(rc, msg.decode() if msg else "")


def exported_symbols(path: os.PathLike) -> set[str]:
    """Dynamic symbols a shared object exports (for the ABI-completeness test)."""
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True)
    return {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
