"""ctypes binding of ``libfcp_hip.so`` (C ABI: ``include/fcp_hip.h``).

The library is built in-tree by ``__graft_entry__.build()`` (``hipcc
--offload-arch=gfx950``).  There is NO fallback: if the shared object is
missing or cannot be loaded, importing the product path fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

from .plan import (FLAG_OUT_BF16, FLAG_OUT_F16, FLAG_TABLES_BF16, FLAG_TABLES_F16, FLAG_TABLES_PER_INPUT, FLAG_TABLES_Q8,  # noqa: F401
                   OUT_FORMATS, TABLE_FORMATS)

_HERE = os.path.dirname(os.path.abspath(__file__))
# FCP_LIB_DIR: loads the library from another build directory (`make -C recom_amd/csrc OUT=<dir>`, e.g. of another commit)
LIB_PATH = os.path.join(os.environ.get("FCP_LIB_DIR", _HERE), "libfcp_hip.so")

FCP_ABI_VERSION = 2
FCP_OK = 0
FCP_ERR_INVALID_ARGUMENT = 1
FCP_ERR_SHAPE_MISMATCH = 2
FCP_ERR_ALLOC = 3
FCP_ERR_HIP = 4
FCP_ERR_UNSUPPORTED = 5
FCP_ERR_NO_DEVICE = 6
FLAG_HOST_ONLY = 1 << 31  # plan without device resources (layout queries only)
# the storage formats (plan.OUT_FORMATS / plan.TABLE_FORMATS) as the library numbers them: FCP_OUT_* / FCP_TAB_* -> name, name -> flag bit
OUT_DTYPES = dict(enumerate(OUT_FORMATS))                                 # fcp_plan_out_dtype
OUT_DTYPE_FLAGS = {name: f.flag for name, f in OUT_FORMATS.items()}
ALL_TABLE_DTYPES = dict(enumerate(TABLE_FORMATS))                         # fcp_plan_table_kinds
ALL_TABLE_DTYPE_FLAGS = {name: f.flag for name, f in TABLE_FORMATS.items()}
TAB_Q8 = 3                 # FCP_TAB_Q8
TABLE_DTYPES = {k: n for k, n in ALL_TABLE_DTYPES.items() if k != TAB_Q8}   # the 16-bit feature's two dicts: without "q8"
TABLE_DTYPE_FLAGS = {n: ALL_TABLE_DTYPE_FLAGS[n] for n in TABLE_DTYPES.values()}
TAB_MIXED = 255            # FCP_TAB_MIXED: fcp_plan_table_dtype of a plan whose tables have more than one format; no row format
PLAN_TABLE_DTYPES = {**ALL_TABLE_DTYPES, TAB_MIXED: "mixed"}   # what fcp_plan_table_dtype may answer
TABLE_KINDS = {name: kind for kind, name in ALL_TABLE_DTYPES.items()}   # name -> FCP_TAB_* (fcp_table_convert)
# fcp_launch_info_t (fcp_plan_last_launch): names of the kernel, store-policy and segment-offset codes
LAUNCH_KERNELS = {0: "none", 1: "dense", 2: "ragged", 3: "hybrid", 4: "ragged_weighted",
                  5: "dense_narrow", 6: "ragged_narrow", 7: "hybrid_narrow",
                  8: "dense_tab16", 9: "ragged_tab16", 10: "hybrid_tab16",
                  11: "dense_tabq8", 12: "ragged_tabq8", 13: "hybrid_tabq8",
                  14: "dense_tabmix", 15: "ragged_tabmix", 16: "hybrid_tabmix"}
DENSE_FRONTS = {0: "none", 1: "generic", 2: "plain"}   # fcp_plan_last_dense_front
LAUNCH_STORES = {0: "nt", 1: "sc1_nt", 4: "plain", 8: "sc1"}
LAUNCH_SEGMENT_OFFSETS = {0: "none", 1: "prepass", 2: "search"}
# fcp_aux_launch_counts: the kernels outside the fused matrix, one counter per instantiation (FCP_AUX_* order)
AUX_KERNELS = ("segment_offsets", "shard_finalize_v4", "shard_finalize_v2", "shard_finalize_v1",
               "concat_v4", "concat_v2", "concat_v1", "upload", "h2d_copy")


class FcpError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = "") -> None:
        self.status = status
        super().__init__(f"{what}: status {status}" + (f" ({detail})" if detail else ""))


class ColumnDesc(C.Structure):
    _fields_ = [
        ("form", C.c_int32), ("combiner", C.c_int32), ("dim", C.c_int32), ("id_source", C.c_int32),
        ("vocab", C.c_int64),
        ("table_input", C.c_int32), ("ids_input", C.c_int32), ("seg_input", C.c_int32),
        ("seg_kind", C.c_int32), ("seg_stride", C.c_int32),
        ("rows_source", C.c_int32), ("rows_arg", C.c_int32),
        ("n_boundaries", C.c_int32),
        ("boundaries", C.POINTER(C.c_float)),
        ("concat_group", C.c_int32), ("concat_slot", C.c_int32),
        ("xform_mode", C.c_int32), ("xform_n", C.c_int32),
        ("xform_lo", C.POINTER(C.c_int64)), ("xform_hi", C.POINTER(C.c_int64)),
        ("xform_substitute", C.c_int64), ("hash_buckets", C.c_int64),
    ]


class ColumnExt(C.Structure):
    """fcp_column_ext_t: per-column extensions (segment-id maps, per-id weights, the table's format under
    FLAG_TABLES_PER_INPUT: ``table_kind1`` = 1 + FCP_TAB_*, 0 = float32)"""
    _fields_ = [
        ("seg_map_n", C.c_int32), ("seg_map_sym", C.c_int32), ("seg_map_sym_slot", C.c_int32), ("weights_input1", C.c_int32),
        ("seg_map_mul", C.c_int64 * 4), ("seg_map_div", C.c_int64),
        ("table_kind1", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int64 * 1),
    ]


class PlanDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_columns", C.c_int32),
        ("columns", C.POINTER(ColumnDesc)),
        ("n_host_inputs", C.c_int32),
        ("host_input_ranks", C.POINTER(C.c_int32)),
        ("host_input_elem_sizes", C.POINTER(C.c_int32)),
        ("n_device_inputs", C.c_int32), ("n_groups", C.c_int32), ("n_symbols", C.c_int32),
        ("layout", C.c_int32), ("device", C.c_int32),
        ("shard_rank", C.c_int32), ("shard_world", C.c_int32),
        ("flags", C.c_uint32),
    ]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class ProcessArgs(C.Structure):
    _fields_ = [
        ("concated_inputs", C.c_void_p), ("concated_bytes", C.c_int64),
        ("concated_offsets", C.POINTER(C.c_int32)), ("concated_shapes", C.POINTER(C.c_int32)),
        ("input_ptrs", C.POINTER(C.c_void_p)), ("input_shapes", C.POINTER(C.c_int32)),
        ("symbols", C.POINTER(C.c_int32)),
        ("stream", C.c_void_p),
        ("malloc_temp", ALLOC_FN), ("malloc_temp_ctx", C.c_void_p),
        ("malloc_buff", ALLOC_FN), ("malloc_buff_ctx", C.c_void_p),
    ]


class ProcessResult(C.Structure):
    _fields_ = [
        ("output_ptrs", C.POINTER(C.c_void_p)), ("output_shapes", C.POINTER(C.c_int32)),
        ("output_row_strides", C.POINTER(C.c_int64)),
        ("group_ptrs", C.POINTER(C.c_void_p)), ("group_shapes", C.POINTER(C.c_int32)),
        ("buffer", C.c_void_p), ("buffer_bytes", C.c_int64),
    ]


class Placement(C.Structure):
    _fields_ = [("mode", C.c_int32), ("min_world", C.c_int32), ("bytes_per_gpu", C.c_int64)]


class TableAuditKind(C.Structure):
    """fcp_table_audit_kind_t"""
    _fields_ = [("rows_bad", C.c_int64), ("first_bad_row", C.c_int64), ("sum_sq_err", C.c_double), ("max_abs_err", C.c_float),
                ("reserved", C.c_int32)]


class TableAudit(C.Structure):
    """fcp_table_audit_t"""
    _fields_ = [("rows", C.c_int64), ("rows_nonfinite", C.c_int64), ("first_nonfinite_row", C.c_int64), ("sum_sq", C.c_double),
                ("kind", TableAuditKind * 4)]


class TableDigest(C.Structure):
    """fcp_table_digest_t"""
    _fields_ = [("sum", C.c_uint64), ("rows", C.c_int64), ("skipped", C.c_int64), ("reserved", C.c_int64)]


class TableDeltaReport(C.Structure):
    """fcp_table_delta_report_t"""
    _fields_ = [("n", C.c_int64), ("distinct", C.c_int64), ("duplicates", C.c_int64), ("skipped", C.c_int64)]


class TableDiffReport(C.Structure):
    """fcp_table_diff_report_t"""
    _fields_ = [("rows", C.c_int64), ("changed", C.c_int64), ("first_changed", C.c_int64), ("last_changed", C.c_int64)]


class OutputError(C.Structure):
    """fcp_output_error_t"""
    _fields_ = [("elems", C.c_int64), ("differ", C.c_int64), ("nonfinite", C.c_int64), ("first_differ_row", C.c_int64),
                ("sum_sq_ref", C.c_double), ("sum_sq_err", C.c_double), ("max_abs_err", C.c_float), ("max_abs_ref", C.c_float),
                ("reserved", C.c_int64)]


class TableRows(C.Structure):
    """fcp_table_rows_t: one entry of fcp_tables_update_rows / fcp_tables_read_rows"""
    _fields_ = [("table", C.c_void_p), ("row_ids", C.c_void_p), ("rows", C.c_void_p), ("table_rows", C.c_int64), ("n", C.c_int64),
                ("kind", C.c_int32), ("dim", C.c_int32), ("reserved", C.c_int64 * 2)]


class TableDigestEntry(C.Structure):
    """fcp_table_digest_entry_t: one entry of fcp_tables_digest"""
    _fields_ = [("table", C.c_void_p), ("row_ids", C.c_void_p), ("rows", C.c_int64), ("n", C.c_int64), ("row0", C.c_int64),
                ("row_step", C.c_int64), ("kind", C.c_int32), ("dim", C.c_int32), ("reserved", C.c_int64)]


class TableDeltaEntry(C.Structure):
    """fcp_table_delta_entry_t: one entry of fcp_tables_delta_distinct"""
    _fields_ = [("row_ids", C.c_void_p), ("rows", C.c_void_p), ("ids_out", C.c_void_p), ("rows_out", C.c_void_p), ("pos_out", C.c_void_p),
                ("table_rows", C.c_int64), ("n", C.c_int64), ("id_bytes", C.c_int32), ("dim", C.c_int32)]


class PrivateStreamsStats(C.Structure):
    """fcp_private_streams_stats_t"""
    _fields_ = [("supervised_stream", C.c_void_p), ("requests", C.c_int64), ("lane_requests", C.c_int64), ("evaluations", C.c_int64),
                ("stream_order_us_per_mib", C.c_double), ("last_ratio", C.c_double), ("worst_ratio", C.c_double),
                ("keep_ratio", C.c_double), ("demoted", C.c_int32), ("evaluation_in_progress", C.c_int32)]


class LaunchInfo(C.Structure):
    """fcp_launch_info_t"""
    _fields_ = [("kernel", C.c_int32), ("vec", C.c_int32), ("rows_per_wave", C.c_int32), ("store_policy", C.c_int32),
                ("wide_rows", C.c_int32), ("shard_world", C.c_int32), ("dense_blocks", C.c_int32), ("ragged_blocks", C.c_int32),
                ("segment_offsets", C.c_int32)]


class StagerStats(C.Structure):
    """fcp_stager_stats_t"""
    _fields_ = [("calls", C.c_int64), ("copy_calls", C.c_int64), ("copy_calls_over_1ms", C.c_int64), ("fallback_switches", C.c_int64),
                ("requests_with_blocked_copy", C.c_int64), ("max_copy_call_us", C.c_double)]


class HostTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("elem_size", C.c_int32), ("rank", C.c_int32),
                ("dims", C.POINTER(C.c_int64))]


# every symbol include/fcp_hip.h declares
EXPORTS = [
    "fcp_abi_version", "fcp_status_string", "fcp_last_error",
    "fcp_concat_inputs_sizes", "fcp_concat_inputs",
    "fcp_plan_create", "fcp_plan_create_ex", "fcp_plan_create_from_file", "fcp_plan_counts", "fcp_plan_destroy", "fcp_plan_group_width",
    "fcp_plan_column_offset",
    "fcp_plan_arena_bytes", "fcp_plan_read_bad_ids", "fcp_plan_output_columns", "fcp_plan_table_bytes",
    "fcp_placement_decide", "fcp_plan_release_captures",
    "fcp_process_feature_columns", "fcp_concat_outputs", "fcp_concat_outputs_scatter", "fcp_concat_outputs_host",
    "fcp_shard_finalize", "fcp_comm_unique_id", "fcp_comm_create", "fcp_comm_destroy", "fcp_comm_rank",
    "fcp_shard_batch_slice", "fcp_shard_exchange", "fcp_shard_exchange_columns",
    "fcp_shard_step_create", "fcp_shard_step_run", "fcp_shard_step_destroy",
    "fcp_stager_create", "fcp_stager_create_ex", "fcp_stager_stage", "fcp_stager_stage_ex", "fcp_stager_stage_narrow", "fcp_stager_destroy", "fcp_stager_stats",
    "fcp_concat_inputs_ex_sizes", "fcp_concat_inputs_ex", "fcp_plan_file_stage_info",
    "fcp_pack_pool_create", "fcp_pack_pool_destroy", "fcp_concat_inputs_ex_pool",
    "fcp_graph_build", "fcp_graph_free", "fcp_placement_assign", "fcp_concat_outputs_scatter_strided",
    "fcp_plan_set_private_streams", "fcp_result_wait", "fcp_result_synchronize", "fcp_plan_set_request_order",
    "fcp_plan_probe_private_streams", "fcp_plan_private_streams_verdict", "fcp_plan_verify_private_streams",
    "fcp_plan_private_streams_stats", "fcp_plan_last_launch", "fcp_plan_last_csr", "fcp_aux_launch_counts",
    "fcp_plan_out_dtype", "fcp_plan_last_dense_front", "fcp_plan_table_dtype",
    "fcp_table_row_bytes", "fcp_table_convert", "fcp_table_update_rows", "fcp_table_read_rows",
    "fcp_plan_table_kinds",
    "fcp_table_audit_workspace_bytes", "fcp_table_audit", "fcp_table_formats_choose",
    "fcp_table_audit_weighted", "fcp_table_count_ids",
    "fcp_plan_table_rows", "fcp_plan_traffic_bind", "fcp_plan_traffic_count",
    "fcp_table_digest_workspace_bytes", "fcp_table_digest", "fcp_table_digest_rows", "fcp_table_digest_host",
    "fcp_table_delta_workspace_bytes", "fcp_table_delta_distinct",
    "fcp_table_diff_workspace_bytes", "fcp_table_diff",
    "fcp_outputs_compare_workspace_bytes", "fcp_outputs_compare",
    "fcp_tables_rows_workspace_bytes", "fcp_tables_rows_launches", "fcp_tables_update_rows", "fcp_tables_read_rows",
    "fcp_tables_digest_workspace_bytes", "fcp_tables_digest_launches", "fcp_tables_digest",
    "fcp_tables_delta_workspace_bytes", "fcp_tables_delta_launches", "fcp_tables_delta_deal_blocks", "fcp_tables_delta_grid",
    "fcp_tables_delta_distinct",
]

_lib = None


def _build_in_tree() -> None:
    """`make -C recom_amd/csrc` (hipcc --offload-arch=gfx950) when the shared objects are missing,
    e.g. in a fresh checkout.  Silent no-op when there is no hipcc: load() then fails loudly."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")) or not shutil.which("make"):
        return
    # several ranks of one node may get here at once (torch.distributed.run): one builds, the others wait
    import fcntl
    try:
        with open(os.path.join(_HERE, "csrc", ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(LIB_PATH):
                subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc")], stdout=subprocess.DEVNULL)
    except (subprocess.CalledProcessError, OSError):
        pass


def load() -> C.CDLL:
    """Load libfcp_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch (device memory / stream plumbing of the Python host side) bundles its
    # own HIP runtime.  Load it first so the process ends up with ONE runtime: if
    # libfcp_hip.so pulled in /opt/rocm's copy before torch initialised its own, the
    # second runtime to start would not see the GPU.
    try:
        import torch  # noqa: F401
    except ImportError:  # the C ABI itself does not need torch
        pass
    if not os.path.exists(LIB_PATH) and "FCP_LIB_DIR" not in os.environ:
        _build_in_tree()                     # fresh checkout on a box with hipcc: build, never fall back
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    L = C.CDLL(LIB_PATH)
    L.fcp_abi_version.restype = C.c_int
    L.fcp_status_string.restype = C.c_char_p
    L.fcp_status_string.argtypes = [C.c_int]
    L.fcp_last_error.restype = C.c_char_p
    L.fcp_concat_inputs_sizes.argtypes = [C.POINTER(HostTensor), C.c_int32, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int32)]
    L.fcp_concat_inputs.argtypes = [C.POINTER(HostTensor), C.c_int32, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p]
    L.fcp_plan_create.argtypes = [C.POINTER(PlanDesc), C.POINTER(C.c_void_p)]
    if hasattr(L, "fcp_plan_create_ex"):
        L.fcp_plan_create_ex.argtypes = [C.POINTER(PlanDesc), C.POINTER(ColumnExt), C.POINTER(C.c_void_p)]
    L.fcp_plan_create_from_file.argtypes = [C.c_char_p, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.fcp_plan_counts.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 5
    L.fcp_plan_destroy.argtypes = [C.c_void_p]
    L.fcp_plan_group_width.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.fcp_plan_column_offset.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.fcp_plan_arena_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.fcp_plan_read_bad_ids.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.fcp_process_feature_columns.argtypes = [C.c_void_p, C.POINTER(ProcessArgs), C.POINTER(ProcessResult)]
    L.fcp_concat_outputs.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                     C.c_void_p]
    L.fcp_plan_output_columns.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int32]
    L.fcp_plan_table_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.fcp_plan_out_dtype.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.fcp_plan_table_dtype.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.fcp_plan_table_kinds.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
    L.fcp_plan_release_captures.argtypes = [C.c_void_p]
    L.fcp_placement_decide.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                       C.POINTER(Placement)]
    L.fcp_concat_outputs_scatter.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                             C.c_int32, C.c_void_p, C.c_void_p]
    L.fcp_concat_outputs_host.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                          C.c_int32, C.c_void_p, ALLOC_FN, C.c_void_p, C.c_int32, C.c_void_p]
    L.fcp_shard_finalize.argtypes = [C.c_void_p, C.POINTER(ProcessArgs), C.c_int32, C.c_void_p, C.c_int32,
                                     C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.fcp_comm_unique_id.argtypes = [C.c_void_p]
    L.fcp_comm_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.fcp_comm_destroy.argtypes = [C.c_void_p]
    L.fcp_comm_rank.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.fcp_shard_batch_slice.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.fcp_shard_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.c_void_p]
    L.fcp_shard_exchange_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
    L.fcp_shard_step_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                        C.POINTER(C.c_void_p)]
    L.fcp_shard_step_run.argtypes = [C.c_void_p, C.POINTER(ProcessArgs), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64)]
    L.fcp_shard_step_destroy.argtypes = [C.c_void_p]
    L.fcp_stager_stage_ex.argtypes = [C.c_void_p, C.POINTER(HostTensor), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.POINTER(C.c_int32)),
                                      C.POINTER(C.POINTER(C.c_int32))]
    L.fcp_stager_create_ex.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                       C.POINTER(C.c_void_p)]
    L.fcp_stager_create.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(C.c_void_p)]
    L.fcp_stager_stage.argtypes = [C.c_void_p, C.POINTER(HostTensor), C.c_int32, C.c_void_p, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_int64), C.POINTER(C.POINTER(C.c_int32)),
                                   C.POINTER(C.POINTER(C.c_int32))]
    L.fcp_stager_stage_narrow.argtypes = [C.c_void_p, C.POINTER(HostTensor), C.c_int32, C.POINTER(C.c_uint8),
                                          C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                          C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32))]
    L.fcp_stager_destroy.argtypes = [C.c_void_p]
    if hasattr(L, "fcp_stager_stats"):
        L.fcp_stager_stats.argtypes = [C.c_void_p, C.POINTER(StagerStats)]
    if hasattr(L, "fcp_pack_pool_create"):
        L.fcp_pack_pool_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        L.fcp_pack_pool_destroy.argtypes = [C.c_void_p]
        L.fcp_concat_inputs_ex_pool.argtypes = [C.c_void_p, C.POINTER(HostTensor), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int64, C.c_void_p, C.c_void_p]
    if "FCP_LIB_DIR" not in os.environ or hasattr(L, "fcp_concat_inputs_ex"):  # (an older A/B build may predate these)
        L.fcp_concat_inputs_ex_sizes.argtypes = [C.POINTER(HostTensor), C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int32)]
        L.fcp_concat_inputs_ex.argtypes = [C.POINTER(HostTensor), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_void_p]
        L.fcp_plan_file_stage_info.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int32,
                                               C.POINTER(C.c_int32)]
        L.fcp_graph_build.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_char_p)]
        L.fcp_graph_free.argtypes = [C.c_void_p]
        L.fcp_graph_free.restype = None
        L.fcp_placement_assign.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                           C.POINTER(Placement)]
        L.fcp_concat_outputs_scatter_strided.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                         C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    if hasattr(L, "fcp_plan_set_private_streams"):                              # (an older A/B build may predate these)
        L.fcp_plan_set_private_streams.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
        L.fcp_result_wait.argtypes = [C.c_void_p, C.c_void_p]
        L.fcp_result_synchronize.argtypes = [C.c_void_p]
    if hasattr(L, "fcp_plan_probe_private_streams"):
        L.fcp_plan_probe_private_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.fcp_plan_private_streams_verdict.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    if hasattr(L, "fcp_plan_verify_private_streams"):
        L.fcp_plan_verify_private_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.fcp_plan_private_streams_stats.argtypes = [C.c_void_p, C.POINTER(PrivateStreamsStats)]
    if hasattr(L, "fcp_plan_set_request_order"):
        L.fcp_plan_set_request_order.argtypes = [C.c_void_p, C.c_int32]
    if hasattr(L, "fcp_plan_last_launch"):
        L.fcp_plan_last_launch.argtypes = [C.c_void_p, C.POINTER(LaunchInfo)]
    if hasattr(L, "fcp_aux_launch_counts"):
        L.fcp_plan_last_csr.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int32]
        L.fcp_aux_launch_counts.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    if hasattr(L, "fcp_plan_last_dense_front"):
        L.fcp_plan_last_dense_front.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    if hasattr(L, "fcp_table_convert"):
        L.fcp_table_row_bytes.restype = C.c_int64
        L.fcp_table_row_bytes.argtypes = [C.c_int32, C.c_int32]
        L.fcp_table_convert.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_void_p]
    if hasattr(L, "fcp_table_update_rows"):
        L.fcp_table_update_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_int32, C.c_void_p]
        L.fcp_table_read_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                          C.c_int32, C.c_void_p]
    if hasattr(L, "fcp_table_audit"):
        L.fcp_table_audit_workspace_bytes.restype = C.c_int64
        L.fcp_table_audit_workspace_bytes.argtypes = []
        L.fcp_table_audit.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.fcp_table_formats_choose.argtypes = [C.POINTER(TableAudit), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.c_int64,
                                               C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                               C.POINTER(C.c_double)]
    if hasattr(L, "fcp_table_count_ids"):
        L.fcp_table_audit_weighted.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.fcp_table_count_ids.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(L, "fcp_plan_traffic_count"):
        L.fcp_plan_table_rows.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)]
        L.fcp_plan_traffic_bind.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p]
        L.fcp_plan_traffic_count.argtypes = [C.c_void_p, C.POINTER(ProcessArgs)]
    if hasattr(L, "fcp_table_digest"):
        L.fcp_table_digest_workspace_bytes.restype = C.c_int64
        L.fcp_table_digest_workspace_bytes.argtypes = []
        L.fcp_table_digest.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_void_p]
        L.fcp_table_digest_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.fcp_table_digest_host.restype = C.c_uint64
        L.fcp_table_digest_host.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int64]
    if hasattr(L, "fcp_table_delta_distinct"):
        L.fcp_table_delta_workspace_bytes.restype = C.c_int64
        L.fcp_table_delta_workspace_bytes.argtypes = [C.c_int64]
        L.fcp_table_delta_distinct.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(L, "fcp_table_diff"):
        L.fcp_table_diff_workspace_bytes.restype = C.c_int64
        L.fcp_table_diff_workspace_bytes.argtypes = [C.c_int64]
        L.fcp_table_diff.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(L, "fcp_outputs_compare"):
        L.fcp_outputs_compare_workspace_bytes.restype = C.c_int64
        L.fcp_outputs_compare_workspace_bytes.argtypes = [C.c_int32]
        L.fcp_outputs_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(L, "fcp_tables_update_rows"):
        L.fcp_tables_rows_workspace_bytes.restype = C.c_int64
        L.fcp_tables_rows_workspace_bytes.argtypes = [C.c_int32]
        L.fcp_tables_rows_launches.restype = C.c_int32
        L.fcp_tables_rows_launches.argtypes = [C.POINTER(TableRows), C.c_int32]
        L.fcp_tables_update_rows.argtypes = [C.POINTER(TableRows), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.fcp_tables_read_rows.argtypes = [C.POINTER(TableRows), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(L, "fcp_tables_delta_distinct"):
        L.fcp_tables_delta_workspace_bytes.restype = C.c_int64
        L.fcp_tables_delta_workspace_bytes.argtypes = [C.POINTER(C.c_int64), C.c_int32]
        L.fcp_tables_delta_launches.restype = C.c_int32
        L.fcp_tables_delta_launches.argtypes = [C.POINTER(TableDeltaEntry), C.c_int32]
        L.fcp_tables_delta_deal_blocks.restype = C.c_int32
        L.fcp_tables_delta_deal_blocks.argtypes = []
        L.fcp_tables_delta_grid.restype = C.c_int32
        L.fcp_tables_delta_grid.argtypes = [C.POINTER(TableDeltaEntry), C.c_int32, C.POINTER(C.c_int32)]
        L.fcp_tables_delta_distinct.argtypes = [C.POINTER(TableDeltaEntry), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(L, "fcp_tables_digest"):
        L.fcp_tables_digest_workspace_bytes.restype = C.c_int64
        L.fcp_tables_digest_workspace_bytes.argtypes = [C.c_int32]
        L.fcp_tables_digest_launches.restype = C.c_int32
        L.fcp_tables_digest_launches.argtypes = [C.POINTER(TableDigestEntry), C.c_int32, C.POINTER(C.c_int32)]
        L.fcp_tables_digest.argtypes = [C.POINTER(TableDigestEntry), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if L.fcp_abi_version() != FCP_ABI_VERSION:
        raise ImportError("libfcp_hip.so ABI version mismatch; rebuild")
    _lib = L
    return L


def aux_launch_counts(reset: bool = False) -> dict:
    """``fcp_aux_launch_counts``: process-wide launches of each kernel outside the fused matrix, by ``AUX_KERNELS`` name;
    ``reset`` zeroes the counters after reading them."""
    L = load()
    counts = (C.c_int64 * len(AUX_KERNELS))()
    n = L.fcp_aux_launch_counts(counts, len(AUX_KERNELS), 1 if reset else 0)
    if n != len(AUX_KERNELS):
        raise FcpError(-n if n < 0 else FCP_ERR_UNSUPPORTED, "fcp_aux_launch_counts", f"{n} counters")
    return dict(zip(AUX_KERNELS, counts[:]))


def check(status: int, what: str) -> None:
    if status != FCP_OK:
        L = load()
        detail = L.fcp_last_error().decode(errors="replace") or L.fcp_status_string(status).decode()
        raise FcpError(status, what, detail)
