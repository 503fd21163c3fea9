"""Host-side mirror of the reference's three custom ops, above the C ABI.

Same names, argument meaning and error behaviour as the TensorFlow ops of the
reference (TensorFlow itself is not available here, so tensors are NumPy on the
host and ``torch`` tensors on the device — torch is plumbing for device memory
and streams only):

* :func:`concat_inputs`           — ``Addons>ConcatInputs``
  (``custom_ops/concat_inputs/concat_inputs_ops.cc:42-88``)
* :class:`FeatureColumnProcess`   — ``Addons>FeatureColumnProcess[WithSymbols]``
  (``custom_ops/feature_column_process/feature_column_process_op_gpu.cu.cc:33-175``)
* :func:`concat_outputs`          — ``Addons>ConcatOutputs[NoHost]``
  (``custom_ops/concat_outputs/concat_outputs_op_gpu.cu.cc:180-288``)

All compute goes through ``libfcp_hip.so``; there is no Python/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import lib as _lib
from .plan import (FORM_BATCH_COL_REDUCTION, FORM_GATHER, FORM_GATHER_SCATTER, FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE,
                   IDS_F32_BUCKETIZE, LAYOUT_CONCAT, PlanSpec)


# ----------------------------------------------------------------------------
# Addons>ConcatInputs (CPU op)
# ----------------------------------------------------------------------------
def _host_tensors(inputs):
    arrs = [np.require(np.asarray(a), requirements="C") for a in inputs]  # keeps rank-0
    dims_keep = [np.asarray(a.shape, np.int64) for a in arrs]
    tens = (_lib.HostTensor * max(len(arrs), 1))()
    for i, a in enumerate(arrs):
        tens[i] = _lib.HostTensor(a.ctypes.data, a.dtype.itemsize, a.ndim,
                                  dims_keep[i].ctypes.data_as(C.POINTER(C.c_int64)))
    return arrs, dims_keep, tens


class PackPool:
    """Worker pool for ``Addons>ConcatInputs`` (``fcp_pack_pool_create``): the reference's op packs on one thread
    (``concat_inputs_ops.cc:42-77``); with a pool one call's inputs are split over sleeping worker threads."""

    def __init__(self, n_threads: int) -> None:
        self._L = _lib.load()
        self.handle = C.c_void_p()
        _lib.check(self._L.fcp_pack_pool_create(int(n_threads), C.byref(self.handle)), "fcp_pack_pool_create")

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._L.fcp_pack_pool_destroy(self.handle)
            self.handle = None

    __del__ = close


def concat_inputs(inputs: Sequence[np.ndarray], stage=None, pool: Optional[PackPool] = None):
    """Pack N host tensors into ``(output:int8[sum bytes], offsets:int32[N],
    shapes:int32[sum rank])`` — bit-exact with ``ConcatInputsOp::Compute``.  ``pool``: pack on a worker pool.

    ``stage`` (a :class:`recom_amd.plan.StageInfo`, the stage section of the plan file): the staged form —
    int64 ids packed as int32, the sorted row ids / SparseTensor indices of pooled columns as int32 row offsets
    (``fcp_concat_inputs_ex``); the consuming plan is the staged plan."""
    L = _lib.load()
    arrs, dims_keep, tens = _host_tensors(inputs)
    n = len(arrs)
    nbytes = C.c_int64(0)
    rank_sum = C.c_int32(0)
    if stage is None:
        _lib.check(L.fcp_concat_inputs_sizes(tens, n, C.byref(nbytes), C.byref(rank_sum)), "ConcatInputs")
    else:
        if len(stage.modes) != n:
            raise ValueError(f"ConcatInputs: the plan's stage section lists {len(stage.modes)} inputs, the op got {n}")
        modes = np.asarray(stage.modes, np.uint8)
        args = np.asarray(stage.mode_args(arrs), np.int64)
        _lib.check(L.fcp_concat_inputs_ex_sizes(tens, n, modes.ctypes.data, args.ctypes.data, C.byref(nbytes),
                                                C.byref(rank_sum)), "ConcatInputs")
    blob = np.empty(nbytes.value, np.int8)
    offsets = np.empty(n, np.int32)
    shapes = np.empty(rank_sum.value, np.int32)
    if pool is not None:
        m, a = (None, None) if stage is None else (modes.ctypes.data, args.ctypes.data)
        _lib.check(L.fcp_concat_inputs_ex_pool(pool.handle, tens, n, m, a, blob.ctypes.data, blob.nbytes, offsets.ctypes.data,
                                               shapes.ctypes.data), "ConcatInputs")
    elif stage is None:
        _lib.check(L.fcp_concat_inputs(tens, n, blob.ctypes.data, blob.nbytes, offsets.ctypes.data,
                                       shapes.ctypes.data), "ConcatInputs")
    else:
        _lib.check(L.fcp_concat_inputs_ex(tens, n, modes.ctypes.data, args.ctypes.data, blob.ctypes.data, blob.nbytes,
                                          offsets.ctypes.data, shapes.ctypes.data), "ConcatInputs")
    return blob, offsets, shapes


def pack_as_staged(inputs: Sequence[np.ndarray], modes: Sequence[int]):
    """ALREADY CONVERTED tensors (``synth.staged_model``: int32 ids, int32 row offsets) laid out as the staged
    ``Addons>ConcatInputs`` lays out its blob (``stage_layout``, ``csrc/fcp_stager.hip``): copied / narrowed inputs back to back
    in input order from offset 0, the inputs that were converted to row offsets (mode 2) behind all of them, in input order, from
    a 4-byte boundary — one [columns, rows + 1] matrix.  For harnesses that keep staged requests resident (the op itself
    converts while it packs: ``concat_inputs(raw, stage)``; tests hold the two to each other, ``conftest.assert_staged_blob``).
    Returns ``(blob, offsets, shapes)``."""
    _, _, shapes = concat_inputs(inputs)
    raws = [np.ascontiguousarray(a).view(np.int8).reshape(-1) if np.asarray(a).size else np.zeros(0, np.int8) for a in inputs]
    order = [i for i, m in enumerate(modes) if m != 2] + [i for i, m in enumerate(modes) if m == 2]
    n_first = sum(1 for m in modes if m != 2)
    offsets = np.zeros(len(inputs), np.int32)
    size = 0
    for pos, i in enumerate(order):
        if pos == n_first:
            size = (size + 3) & ~3
        offsets[i] = size
        size += raws[i].size
    blob = np.zeros(size, np.int8)
    for i in order:
        blob[offsets[i]:offsets[i] + raws[i].size] = raws[i]
    return blob, offsets, shapes


class ConcatInputs:
    """``Addons>ConcatInputs`` as the shim builds it from a node of the rewritten graph: attrs ``T`` / ``ranks``
    (``concat_inputs_ops.cc:33-40``) and, when the graph was rewritten for a staged plan, the node's ``_fcp_plan``
    attr — the plan file whose stage section says how to pack (``tf_shim/fcp_tf_ops.cc``)."""

    def __init__(self, ranks: Sequence[int], plan_path: Optional[str] = None, threads: Optional[int] = None) -> None:
        self.ranks = [int(r) for r in ranks]
        self.stage = None
        # FCP_CONCAT_INPUTS_THREADS (what the shim reads): pack on that many threads; default 1 = the reference's op
        threads = int(os.environ.get("FCP_CONCAT_INPUTS_THREADS", "1")) if threads is None else int(threads)
        self.pool = PackPool(threads) if threads > 1 else None
        if plan_path:
            from .plan_io import load_stage
            self.stage = load_stage(plan_path)
            if self.stage is not None and len(self.stage.modes) != len(self.ranks):
                raise ValueError("ConcatInputs: the plan's stage section does not match the op's inputs")

    def __call__(self, inputs: Sequence[np.ndarray]):
        if [np.asarray(a).ndim for a in inputs] != self.ranks:
            raise ValueError("ConcatInputs: input ranks differ from attr `ranks`")
        return concat_inputs(inputs, self.stage, self.pool)


# ----------------------------------------------------------------------------
# plan handle
# ----------------------------------------------------------------------------
class Plan:
    """Owns an ``fcp_plan_t`` (replaces code generation + ``CreateConstBuffers``,
    ``cuda_emitter.cc:2260-2301``; freed like the op destructor frees
    ``const_buff``, ``feature_column_process_ops.h:47``)."""

    def __init__(self, spec: PlanSpec, device: int = 0, host_only: bool = False) -> None:
        spec.validate()
        self.spec = spec
        self.device = device
        self._L = _lib.load()
        self._keep: List[np.ndarray] = []
        cols = (_lib.ColumnDesc * spec.n_columns)()
        for k, c in enumerate(spec.columns):
            b = None
            if c.boundaries is not None and c.id_source == IDS_F32_BUCKETIZE and \
                    c.form not in (FORM_PASSTHROUGH, FORM_BATCH_COL_REDUCTION):
                b = np.ascontiguousarray(c.boundaries, np.float32)
                self._keep.append(b)
            xlo = np.ascontiguousarray(c.xform_lo, np.int64)
            xhi = np.ascontiguousarray(c.xform_hi, np.int64)
            self._keep += [xlo, xhi]
            cols[k] = _lib.ColumnDesc(
                c.form, c.combiner, c.dim, c.id_source, c.vocab, c.table_input, c.ids_input, c.seg_input,
                c.seg_kind, c.seg_stride, c.rows_source, c.rows_arg, 0 if b is None else len(b),
                None if b is None else b.ctypes.data_as(C.POINTER(C.c_float)), c.concat_group, c.concat_slot,
                c.xform_mode, len(xlo), xlo.ctypes.data_as(C.POINTER(C.c_int64)) if len(xlo) else None,
                xhi.ctypes.data_as(C.POINTER(C.c_int64)) if len(xhi) else None, int(c.xform_substitute),
                int(c.hash_buckets))
        ranks = np.asarray(spec.host_input_ranks, np.int32)
        esz = np.asarray(spec.host_input_elem_sizes, np.int32)
        self._keep += [ranks, esz]
        flags = spec.plan_flags() | (_lib.FLAG_HOST_ONLY if host_only else 0)
        desc = _lib.PlanDesc(
            _lib.FCP_ABI_VERSION, spec.n_columns, cols, len(ranks),
            ranks.ctypes.data_as(C.POINTER(C.c_int32)), esz.ctypes.data_as(C.POINTER(C.c_int32)),
            spec.n_device_inputs, spec.n_groups, spec.n_symbols, spec.layout, device,
            spec.shard_rank, spec.shard_world, flags)
        handle = C.c_void_p()
        # per-column extensions: segment-id maps, weights, per-input table formats
        if any(len(c.seg_mul) or c.weights_input != -1 for c in spec.columns) or spec.table_dtypes is not None:
            ext = (_lib.ColumnExt * spec.n_columns)()
            for k, c in enumerate(spec.columns):
                ext[k].weights_input1 = int(c.weights_input) + 1          # 0 = unweighted
                if spec.table_dtypes is not None and c.form in (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER):
                    ext[k].table_kind1 = 1 + _lib.TABLE_KINDS[spec.table_dtypes[c.table_input]]   # 0 = float32 / no table
                if len(c.seg_mul):
                    ext[k].seg_map_n, ext[k].seg_map_sym, ext[k].seg_map_sym_slot = len(c.seg_mul), c.seg_sym, c.seg_sym_slot
                    for j, v in enumerate(list(c.seg_mul)[:4]):
                        ext[k].seg_map_mul[j] = int(v)
                    ext[k].seg_map_div = int(c.seg_div)
            _lib.check(self._L.fcp_plan_create_ex(C.byref(desc), ext, C.byref(handle)), "fcp_plan_create_ex")
        else:
            _lib.check(self._L.fcp_plan_create(C.byref(desc), C.byref(handle)), "fcp_plan_create")
        self.handle = handle

    @classmethod
    def from_file(cls, path: str, device: int = 0, host_only: bool = False, out_dtype: Optional[str] = None,
                  table_dtype: Optional[str] = None) -> "Plan":
        """The plan a column-plan file describes, parsed by the library itself
        (``fcp_plan_create_from_file`` — what the TF shim calls with the op's ``dlpath``).  ``out_dtype``: "bf16" / "f16"
        select narrow output for a file that does not name a dtype (the flag bits of the call); a file that names
        another one is refused.  ``table_dtype``: the same for 16-bit ("bf16" / "f16") and 8-bit row-quantised ("q8") tables."""
        import dataclasses
        from .plan_io import load_plan
        self = cls.__new__(cls)
        self.device = device
        self._L = _lib.load()
        self._keep = []
        self.handle = None
        handle = C.c_void_p()
        flags = (_lib.FLAG_HOST_ONLY if host_only else 0) | _lib.OUT_DTYPE_FLAGS[out_dtype or "f32"] | \
            _lib.ALL_TABLE_DTYPE_FLAGS[table_dtype or "f32"]
        _lib.check(self._L.fcp_plan_create_from_file(path.encode(), device, flags, C.byref(handle)), "fcp_plan_create_from_file")
        self.handle = handle
        self.spec = load_plan(path)          # Python-side bookkeeping only
        if self.out_dtype() != self.spec.out_dtype:
            self.spec = dataclasses.replace(self.spec, out_dtype=self.out_dtype())
        if self.table_dtype() not in (self.spec.table_dtype, "mixed"):   # (mixed: the file's table_dtypes line, which load_plan read)
            self.spec = dataclasses.replace(self.spec, table_dtype=self.table_dtype())
        return self

    def out_dtype(self) -> str:
        """``fcp_plan_out_dtype``: "f32", "bf16" or "f16" — the element type of the plan's outputs."""
        v = C.c_int32()
        _lib.check(self._L.fcp_plan_out_dtype(self.handle, C.byref(v)), "fcp_plan_out_dtype")
        return _lib.OUT_DTYPES[v.value]

    def table_dtype(self) -> str:
        """``fcp_plan_table_dtype``: "f32", "bf16", "f16" or "q8" — the element type of every embedding table the plan reads;
        "mixed" for a plan whose tables have more than one format (``table_dtypes`` names them)."""
        v = C.c_int32()
        _lib.check(self._L.fcp_plan_table_dtype(self.handle, C.byref(v)), "fcp_plan_table_dtype")
        return _lib.PLAN_TABLE_DTYPES[v.value]

    def table_dtypes(self) -> tuple:
        """``fcp_plan_table_kinds``: one of "f32" / "bf16" / "f16" / "q8" per device input, "-" for an input no lookup column
        reads — of any plan (a plan-wide format names every read input alike)."""
        n = C.c_int32()
        _lib.check(self._L.fcp_plan_table_kinds(self.handle, None, 0, C.byref(n)), "fcp_plan_table_kinds")
        kinds = (C.c_int32 * max(1, n.value))()
        _lib.check(self._L.fcp_plan_table_kinds(self.handle, kinds, n.value, None), "fcp_plan_table_kinds")
        return tuple("-" if kinds[t] < 0 else _lib.ALL_TABLE_DTYPES[kinds[t]] for t in range(n.value))

    def table_rows(self) -> tuple:
        """``fcp_plan_table_rows``: per device input the rows of the unsharded table (the largest ``vocab`` of the lookup
        columns that read it), -1 for an input no lookup column reads — of any plan, host-only ones too."""
        n = C.c_int32()
        _lib.check(self._L.fcp_plan_table_rows(self.handle, None, 0, C.byref(n)), "fcp_plan_table_rows")
        rows = (C.c_int64 * max(1, n.value))()
        _lib.check(self._L.fcp_plan_table_rows(self.handle, rows, n.value, None), "fcp_plan_table_rows")
        return tuple(int(rows[t]) for t in range(n.value))

    def traffic_bind(self, counts, skipped=None) -> None:
        """``fcp_plan_traffic_bind``: ``counts`` names, per device input, the count tensor (``tables.new_plan_counts``: one
        cell per row of the unsharded table, on the plan's device) that ``traffic_count`` adds the table's reads to, or
        ``None`` for a table that is not counted; ``skipped``: an int64 device tensor of one element that receives the ids
        outside their column's vocab (the caller zeroes it), or ``None``.  ``counts=None``, or all entries ``None``,
        unbinds.  The plan keeps the tensors alive until the next bind.  Copies to the device and may synchronise it."""
        import torch
        from . import tables as _tables
        if counts is None:
            _lib.check(self._L.fcp_plan_traffic_bind(self.handle, None, 0, None), "fcp_plan_traffic_bind")
            self._traffic_keep = None
            return
        rows = self.table_rows()
        if len(counts) != len(rows):
            raise ValueError(f"counts names {len(counts)} inputs, the plan has {len(rows)} device inputs")
        for t, c in enumerate(counts):
            if c is None:
                continue
            if _tables._check_counts(torch, c, f"counts[{t}]") != rows[t]:
                raise ValueError(f"counts[{t}] has {c.shape[0]} cells, the plan's table {t} has {rows[t]} rows (Plan.table_rows)")
        for t, c in enumerate(counts):          # (behind what can be seen of the tensors wherever they live)
            if c is None:
                continue
            if not c.is_cuda or (c.device.index or 0) != self.device:
                raise ValueError(f"counts[{t}] is on {c.device}, the plan on cuda:{self.device}")
        if skipped is not None:
            if skipped.dtype != torch.int64 or skipped.numel() != 1 or not skipped.is_cuda or (skipped.device.index or 0) != self.device:
                raise ValueError("skipped is an int64 tensor of one element on the plan's device")
        ptrs = (C.c_void_p * max(1, len(counts)))(*[None if c is None else c.data_ptr() for c in counts])
        _lib.check(self._L.fcp_plan_traffic_bind(self.handle, ptrs, len(counts), None if skipped is None else C.c_void_p(skipped.data_ptr())),
                   "fcp_plan_traffic_bind")
        self._traffic_keep = (list(counts), skipped)

    def traffic_count(self, concated_inputs, concated_offsets, concated_shapes, symbols=None, stream: Optional[int] = None) -> None:
        """``fcp_plan_traffic_count``: add the table rows this request reads — the request as ``FeatureColumnProcess`` takes
        it: the device blob, its host offsets and shapes, the symbols — to the bound count tensors, through the plan's own id
        path (bucketize, hash, select / filter, the vocab check), in one launch.  No tables, no arena.  Asynchronous on
        ``stream`` (torch's current stream of the plan's device by default)."""
        import torch
        offs = np.ascontiguousarray(concated_offsets, np.int32)
        shps = np.ascontiguousarray(concated_shapes, np.int32)
        sym = None if symbols is None else np.ascontiguousarray(symbols, np.int32)
        if stream is None:
            stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        a = _lib.ProcessArgs(
            concated_inputs.data_ptr() if concated_inputs is not None and concated_inputs.numel() else None,
            0 if concated_inputs is None else concated_inputs.numel() * concated_inputs.element_size(),
            offs.ctypes.data_as(C.POINTER(C.c_int32)), shps.ctypes.data_as(C.POINTER(C.c_int32)), None, None,
            None if sym is None else sym.ctypes.data_as(C.POINTER(C.c_int32)), stream)
        _lib.check(self._L.fcp_plan_traffic_count(self.handle, C.byref(a)), "fcp_plan_traffic_count")

    def table_bytes(self):
        """``fcp_plan_table_bytes``: (bytes of tables this plan reads on its device, largest table unsharded)."""
        a, b = C.c_int64(), C.c_int64()
        _lib.check(self._L.fcp_plan_table_bytes(self.handle, C.byref(a), C.byref(b)), "fcp_plan_table_bytes")
        return a.value, b.value

    def counts(self) -> dict:
        v = [C.c_int32() for _ in range(5)]
        _lib.check(self._L.fcp_plan_counts(self.handle, *[C.byref(x) for x in v]), "fcp_plan_counts")
        return dict(zip(("columns", "groups", "host_inputs", "device_inputs", "symbols"), (x.value for x in v)))

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._L.fcp_plan_destroy(self.handle)
            self.handle = None

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def group_width(self, group: int) -> int:
        w = C.c_int32()
        _lib.check(self._L.fcp_plan_group_width(self.handle, group, C.byref(w)), "fcp_plan_group_width")
        return w.value

    def column_offset(self, column: int) -> int:
        o = C.c_int32()
        _lib.check(self._L.fcp_plan_column_offset(self.handle, column, C.byref(o)), "fcp_plan_column_offset")
        return o.value

    def arena_bytes(self, shapes, symbols=None) -> int:
        shapes = np.ascontiguousarray(shapes, np.int32)
        sym = None if symbols is None else np.ascontiguousarray(symbols, np.int32)
        out = C.c_int64()
        _lib.check(self._L.fcp_plan_arena_bytes(self.handle, shapes.ctypes.data,
                                                None if sym is None else sym.ctypes.data, C.byref(out)),
                   "fcp_plan_arena_bytes")
        return out.value

    def set_private_streams(self, n_streams: int, no_caller_wait: bool = False, always: bool = False, verify: bool = True) -> None:
        """``fcp_plan_set_private_streams``: requests of one caller stream run on ``n_streams`` plan-owned streams
        (0 = off; the library creates at most three); readers of a result order themselves behind it with
        ``fcp_result_wait``.  ``always``: also requests whose work is below the library's threshold (48 MiB gathered +
        written), which otherwise stay on the caller's stream.  ``verify`` (default): the first such request of every caller
        stream probes whether the streams really overlap behind it in this process and otherwise looks for a mapping that
        does, or keeps that caller's requests on its own stream (``FCP_PRIVATE_NO_VERIFY`` when False)."""
        _lib.check(self._L.fcp_plan_set_private_streams(self.handle, int(n_streams),
                                                        (1 if no_caller_wait else 0) | (2 if always else 0) | (0 if verify else 4)),
                   "fcp_plan_set_private_streams")
        self.private_streams = int(n_streams)

    def probe_private_streams(self, stream: int, requests: int = 24, spin_us: int = 20, grid_blocks: int = 2048):
        """``fcp_plan_probe_private_streams``: (serial_us, lanes_us) of the synthetic request pattern behind ``stream``."""
        a, b = C.c_double(), C.c_double()
        _lib.check(self._L.fcp_plan_probe_private_streams(self.handle, C.c_void_p(stream), requests, spin_us, grid_blocks,
                                                         C.byref(a), C.byref(b)), "fcp_plan_probe_private_streams")
        return a.value, b.value

    def private_streams_verdict(self, stream: int) -> int:
        """``fcp_plan_private_streams_verdict``: 1 = requests of ``stream`` take the private streams, 0 = they stay on it
        (verified: nothing overlapped), -1 = not verified yet / mode off."""
        v = C.c_int32(-1)
        _lib.check(self._L.fcp_plan_private_streams_verdict(self.handle, C.c_void_p(stream), C.byref(v)), "fcp_plan_private_streams_verdict")
        return int(v.value)

    def verify_private_streams(self, stream: int, budget_ms: int = 0) -> int:
        """``fcp_plan_verify_private_streams``: the verification at warm-up (searches a hardware-queue mapping that overlaps
        behind ``stream`` for at most ``budget_ms``; forgets an earlier negative verdict or a demotion).  Returns the verdict."""
        v = C.c_int32(-1)
        _lib.check(self._L.fcp_plan_verify_private_streams(self.handle, C.c_void_p(stream), int(budget_ms), C.byref(v)),
                   "fcp_plan_verify_private_streams")
        return int(v.value)

    def private_streams_stats(self) -> dict:
        """``fcp_plan_private_streams_stats``: what the run-time supervisor of the private streams has seen."""
        st = _lib.PrivateStreamsStats()
        _lib.check(self._L.fcp_plan_private_streams_stats(self.handle, C.byref(st)), "fcp_plan_private_streams_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def set_inputs_ready(self, on: bool = True) -> None:
        """``fcp_plan_set_request_order(FCP_ORDER_INPUTS_READY)``: the caller's promise that blobs are complete and arenas
        unused when a request is issued; consecutive requests of one stream then overlap (any-order kernel launch)."""
        _lib.check(self._L.fcp_plan_set_request_order(self.handle, 1 if on else 0), "fcp_plan_set_request_order")

    def read_bad_ids(self, stream: int = 0) -> int:
        out = C.c_int64()
        _lib.check(self._L.fcp_plan_read_bad_ids(self.handle, stream, C.byref(out)), "fcp_plan_read_bad_ids")
        return out.value

    def last_launch(self) -> dict:
        """``fcp_plan_last_launch``: what the plan's most recent request enqueued — kernel (``none`` / ``dense`` /
        ``ragged`` / ``hybrid`` / ``ragged_weighted`` / ``dense_narrow`` / ``ragged_narrow`` / ``hybrid_narrow`` / ``dense_tab16`` / ``ragged_tab16`` / ``hybrid_tab16`` / ``dense_tabq8`` / ``ragged_tabq8`` / ``hybrid_tabq8``), ``vec``, dense ``rows_per_wave``, ``store`` (``nt`` / ``sc1_nt`` / ``plain``),
        ``wide_rows``, ``shard_world``, ``dense_blocks`` / ``ragged_blocks``, ``segment_offsets`` (``none`` /
        ``prepass`` / ``search``).  Read-only diagnostics: which kernel instantiation a request reached."""
        li = _lib.LaunchInfo()
        _lib.check(self._L.fcp_plan_last_launch(self.handle, C.byref(li)), "fcp_plan_last_launch")
        return dict(kernel=_lib.LAUNCH_KERNELS[li.kernel], vec=li.vec, rows_per_wave=li.rows_per_wave,
                    store=_lib.LAUNCH_STORES[li.store_policy], wide_rows=bool(li.wide_rows), shard_world=li.shard_world,
                    dense_blocks=li.dense_blocks, ragged_blocks=li.ragged_blocks,
                    segment_offsets=_lib.LAUNCH_SEGMENT_OFFSETS[li.segment_offsets])

    def last_dense_front(self) -> str:
        """``fcp_plan_last_dense_front``: ``none`` / ``generic`` / ``plain`` — which front the dense kernel of the plan's
        most recent request had (``plain``: fcp_dense_kernel_plain).  Read-only diagnostics."""
        v = C.c_int32()
        _lib.check(self._L.fcp_plan_last_dense_front(self.handle, C.byref(v)), "fcp_plan_last_dense_front")
        return _lib.DENSE_FRONTS[v.value]

    def last_csr(self):
        """``fcp_plan_last_csr``: (byte offset of the most recent request's segment-offset scratch in its arena, or -1;
        int32[n_columns] index of each column's range in it, -1 for a column without one).  Read-only diagnostics."""
        off = C.c_int64()
        n = self.spec.n_columns
        base = np.empty(max(n, 1), np.int32)
        _lib.check(self._L.fcp_plan_last_csr(self.handle, C.byref(off), base.ctypes.data, n), "fcp_plan_last_csr")
        return off.value, base[:n]


@dataclass
class ProcessOutputs:
    """What ``FeatureColumnProcessOp::Compute`` returns
    (``feature_column_process_op_gpu.cu.cc:72-126``) plus torch views."""
    output_ptrs: np.ndarray      # int64[n_columns]  (reference: device int64 tensor)
    output_shapes: np.ndarray    # int32[2*n_columns] host
    output_row_strides: np.ndarray
    buffer: "object"             # torch.uint8 arena (output 2)
    groups: list                 # [rows, width] views per concat group (CONCAT layout): torch.float32, or torch.bfloat16 /
                                 # torch.float16 for a narrow-output plan
    group_shapes: np.ndarray

    def wait(self, stream: Optional[int] = None) -> None:
        """Plans with private streams, ``defer_wait=True``: make ``stream`` (default: torch's current stream) wait
        on the device for this result — what ``Addons>ConcatOutputs`` does before it reads the arena
        (``fcp_result_wait``).  A no-op when nothing is pending."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.buffer.device).cuda_stream
        _lib.check(_lib.load().fcp_result_wait(self.buffer.data_ptr(), stream), "fcp_result_wait")

    def column(self, k: int):
        """torch view of column k's output ([rows, dim], possibly strided)."""
        import torch
        rows, dim = int(self.output_shapes[2 * k]), int(self.output_shapes[2 * k + 1])
        dtype = self.groups[0].dtype if self.groups else torch.float32
        f = _typed_arena(torch, self.buffer, dtype)
        off = (int(self.output_ptrs[k]) - self.buffer.data_ptr()) // f.element_size()
        return f.as_strided((rows, dim), (int(self.output_row_strides[k]), 1), off)


def _typed_arena(torch, arena, dtype):
    """The uint8 arena as elements of the plan's output type (float32 arenas as ever; a narrow plan's as 2-byte elements)."""
    if dtype == torch.float32:
        return arena.view(torch.float32)
    return arena[:arena.numel() // 2 * 2].view(dtype)


# ----------------------------------------------------------------------------
# fcp_outputs_compare: what two requests' outputs differ by, per column
# ----------------------------------------------------------------------------
OUTPUT_ERROR_DTYPE = np.dtype([("elems", "<i8"), ("differ", "<i8"), ("nonfinite", "<i8"), ("first_differ_row", "<i8"),
                               ("sum_sq_ref", "<f8"), ("sum_sq_err", "<f8"), ("max_abs_err", "<f4"), ("max_abs_ref", "<f4"),
                               ("reserved", "<i8")])   # fcp_output_error_t, 64 bytes

_compare_workspaces: dict = {}   # (device index, stream) -> torch.int64 workspace: calls on one stream run one after the other


@dataclass
class OutputErrors:
    """``fcp_outputs_compare``'s records on the host: ``columns[k]`` is column k's, ``total`` that of all columns together
    (a NumPy record array of ``OUTPUT_ERROR_DTYPE`` and one record of it: fields by name or as attributes)."""
    columns: np.ndarray
    total: np.record

    def rel_rms(self, k: Optional[int] = None) -> float:
        """sqrt(sum_sq_err / sum_sq_ref) of column ``k``, or of all columns together for ``None``; 0.0 where both sums are 0."""
        r = self.total if k is None else self.columns[k]
        if r["sum_sq_ref"] == 0.0:
            return 0.0 if r["sum_sq_err"] == 0.0 else float("inf")
        return float(np.sqrt(r["sum_sq_err"] / r["sum_sq_ref"]))

    @property
    def identical(self) -> bool:
        """Every pair of elements has the same bit pattern."""
        return int(self.total["differ"]) == 0


def _out_kind(torch, outputs: ProcessOutputs) -> int:
    dtype = outputs.groups[0].dtype if outputs.groups else torch.float32
    return {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]   # FCP_OUT_*


def _same_request(a: ProcessOutputs, b: ProcessOutputs) -> np.ndarray:
    """the output_shapes the two results share, or ValueError"""
    sa, sb = np.asarray(a.output_shapes, np.int32), np.asarray(b.output_shapes, np.int32)
    if sa.size != sb.size:
        raise ValueError(f"compare_outputs: {sa.size // 2} columns against {sb.size // 2}")
    if not np.array_equal(sa, sb):
        k = int(np.flatnonzero(sa != sb)[0]) // 2
        raise ValueError(f"compare_outputs: column {k} is [{sa[2 * k]}, {sa[2 * k + 1]}] in a and [{sb[2 * k]}, {sb[2 * k + 1]}] in b: "
                         "the two results are not of the same request")
    return sa


def compare_outputs_async(a: ProcessOutputs, b: ProcessOutputs, stream: Optional[int] = None):
    """``fcp_outputs_compare`` of two results of the SAME request (two plans, two arenas), enqueued on ``stream`` (default:
    torch's current stream of ``a``'s device) behind whatever wrote them there: returns a device tensor ``[n_columns + 1, 8]``
    of int64 words — one 64-byte ``fcp_output_error_t`` per column, then the one of all columns together — that is valid once
    the stream has reached this point (``OutputErrors`` of it: ``compare_outputs``).  Nothing blocks.  Each side's element kind
    is that of its ``groups[0]`` (float32 for a per-column result); layouts, strides and kinds of the two may differ, their
    ``output_shapes`` must be equal (``ValueError`` naming the first column that differs)."""
    import torch
    sa = _same_request(a, b)
    n = sa.size // 2
    device = a.buffer.device
    if b.buffer.device != device:
        raise ValueError(f"compare_outputs: a lies on {device}, b on {b.buffer.device}")
    L = _lib.load()
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    need = int(L.fcp_outputs_compare_workspace_bytes(n))
    key = (device.index or 0, int(stream))
    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device)):
        out = torch.empty((n + 1, OUTPUT_ERROR_DTYPE.itemsize // 8), dtype=torch.int64, device=device)
        workspace = _compare_workspaces.get(key)
        if workspace is None or workspace.numel() * 8 < need:
            workspace = _compare_workspaces[key] = torch.empty((need // 8,), dtype=torch.int64, device=device)
    pa, pb = np.ascontiguousarray(a.output_ptrs, np.int64), np.ascontiguousarray(b.output_ptrs, np.int64)
    ta, tb = np.ascontiguousarray(a.output_row_strides, np.int64), np.ascontiguousarray(b.output_row_strides, np.int64)
    shapes = np.ascontiguousarray(sa)
    status = L.fcp_outputs_compare(pa.ctypes.data, ta.ctypes.data, _out_kind(torch, a), pb.ctypes.data, tb.ctypes.data,
                                   _out_kind(torch, b), shapes.ctypes.data, n, out.data_ptr(), workspace.data_ptr(),
                                   device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_outputs_compare")
    return out


def compare_outputs(a: ProcessOutputs, b: ProcessOutputs, stream: Optional[int] = None) -> OutputErrors:
    """``compare_outputs_async``, then a synchronise of ``stream`` and the records on the host."""
    import torch
    _same_request(a, b)
    if stream is None:
        stream = torch.cuda.current_stream(a.buffer.device).cuda_stream
    out = compare_outputs_async(a, b, stream)
    torch.cuda.ExternalStream(stream, device=a.buffer.device).synchronize()
    records = np.frombuffer(out.cpu().numpy().tobytes(), OUTPUT_ERROR_DTYPE).copy().view(np.recarray)
    return OutputErrors(records[:-1], records[-1])


class FeatureColumnProcess:
    """``Addons>FeatureColumnProcess[WithSymbols]``.

    Inputs of ``__call__`` follow the op: ``concated_inputs`` (device int8 blob),
    ``concated_offsets`` / ``concated_shapes`` (host int32), ``inputs`` (device
    tables), optional ``symbols`` (host int32).  The ``dlpath`` attr of the
    reference is replaced by the plan.  Work is enqueued on ``stream`` (default:
    torch's current stream); nothing blocks.
    """

    def __init__(self, spec: PlanSpec, device: int = 0, plan: Optional[Plan] = None) -> None:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("FeatureColumnProcess needs a GPU (no CPU fallback)")
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.plan = plan if plan is not None else Plan(spec, device)
        self.spec = spec
        self._L = self.plan._L
        # the element type of the outputs as the LIBRARY holds it (a plan file, or flag bits, may have chosen it)
        self.out_dtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[self.plan.out_dtype()]
        # likewise the element type the bound tables must have (a wrong one would be read as garbage, or out of bounds)
        # (q8: torch.uint8 [vocab, dim + 8] — what quantized::embedding_bag_byte_prepack returns)
        # (per-input table formats: every input is held to ITS kind, as the LIBRARY names it — self.table_dtype is then None)
        torch_dtypes = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "q8": torch.uint8}
        self.table_dtype = torch_dtypes.get(self.plan.table_dtype())
        kinds = self.plan.table_dtypes()
        self._input_dtypes = {t: torch_dtypes[k] for t, k in enumerate(kinds) if k != "-"}
        self._q8_shapes = {c.table_input: (int(c.vocab), int(c.dim) + 8) for c in self.plan.spec.columns
                           if c.form in (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER) and kinds[c.table_input] == "q8"}
        self._table_inputs = sorted({c.table_input for c in self.plan.spec.columns
                                     if c.form in (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER)})

    @classmethod
    def from_plan_file(cls, dlpath: str, device: int = 0) -> "FeatureColumnProcess":
        """The op as the shim builds it: ``dlpath`` attr -> ``fcp_plan_create_from_file``."""
        plan = Plan.from_file(dlpath, device)
        return cls(plan.spec, device, plan)

    def _allocators(self, arena=None):
        """Per-call allocator callbacks (malloc_buff = the op's allocate_output(2),
        malloc_temp = allocate_temp): per-call state keeps __call__ re-entrant.  ``arena``: a caller-owned
        torch.uint8 device tensor that malloc_buff hands out instead of a fresh one (it must hold ``nbytes``)."""
        torch, dev = self.torch, self.device
        state = {"arena": None, "temps": [], "error": None}

        def _alloc(_ctx, nbytes):
            if arena is None:
                state["arena"] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
                return state["arena"].data_ptr()
            have = arena.numel() * arena.element_size()
            if have < int(nbytes):       # (raised after the call: an exception cannot cross the C callback)
                state["error"] = ValueError(f"FeatureColumnProcess: caller arena of {have} bytes, the request needs {int(nbytes)} "
                                            "(Plan.arena_bytes)")
                return None
            state["arena"] = arena
            return arena.data_ptr()

        def _alloc_temp(_ctx, nbytes):
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            state["temps"].append(t)
            return t.data_ptr()

        return state, _lib.ALLOC_FN(_alloc), _lib.ALLOC_FN(_alloc_temp)

    def _args(self, concated_inputs, concated_offsets, concated_shapes, inputs, symbols, stream, arena=None):
        torch = self.torch
        if arena is not None and (arena.dtype != torch.uint8 or arena.device != self.device or not arena.is_contiguous()):
            raise ValueError(f"FeatureColumnProcess: arena= must be a contiguous torch.uint8 tensor on {self.device}")
        offs = np.ascontiguousarray(concated_offsets, np.int32)
        shps = np.ascontiguousarray(concated_shapes, np.int32)
        sym = None if symbols is None else np.ascontiguousarray(symbols, np.int32)
        cached = getattr(self, "_tab_cache", None)
        if cached is not None and cached[0] is inputs and len(inputs) == cached[3]:
            tptrs, tshapes = cached[1], cached[2]  # same table list object as last time (hundreds of tables)
        else:
            for i in self._table_inputs:
                if i < len(inputs) and self.table_dtype is not None and inputs[i].dtype != self.table_dtype:
                    raise ValueError(f"FeatureColumnProcess: table {i} is {inputs[i].dtype}, the plan reads {self.table_dtype} tables "
                                     "(PlanSpec.table_dtype)")
                if i < len(inputs) and self.table_dtype is None and inputs[i].dtype != self._input_dtypes[i]:
                    raise ValueError(f"FeatureColumnProcess: table {i} is {inputs[i].dtype}, the plan reads input {i} as a "
                                     f"{self._input_dtypes[i]} table (PlanSpec.table_dtypes)")
                if i < len(inputs) and i in self._q8_shapes and (tuple(inputs[i].shape) != self._q8_shapes[i] or not inputs[i].is_contiguous()):
                    raise ValueError(f"FeatureColumnProcess: table {i} has shape {tuple(inputs[i].shape)}, the plan reads a contiguous "
                                     f"torch.uint8 table of shape {self._q8_shapes[i]}: [vocab, dim + 8] (codes, float32 scale, float32 bias)")
            tptrs = (C.c_void_p * max(1, len(inputs)))(*[t.data_ptr() for t in inputs])
            tshapes = np.asarray([d for t in inputs for d in t.shape], np.int32)
            self._tab_cache = (inputs, tptrs, tshapes, len(inputs))
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        # (without `arena`, the zero-argument form: callers may replace `_allocators` with their own)
        state, alloc_cb, alloc_temp_cb = self._allocators(arena) if arena is not None else self._allocators()
        a = _lib.ProcessArgs(
            concated_inputs.data_ptr() if concated_inputs is not None and concated_inputs.numel() else None,
            0 if concated_inputs is None else concated_inputs.numel() * concated_inputs.element_size(),
            offs.ctypes.data_as(C.POINTER(C.c_int32)), shps.ctypes.data_as(C.POINTER(C.c_int32)),
            tptrs, tshapes.ctypes.data_as(C.POINTER(C.c_int32)) if len(inputs) and all(t.dim() == 2 for t in inputs) else None,
            None if sym is None else sym.ctypes.data_as(C.POINTER(C.c_int32)),
            stream, alloc_temp_cb, None, alloc_cb, None)
        return a, (offs, shps, sym, tptrs, tshapes, state, alloc_cb, alloc_temp_cb)

    def _process(self, a, res, state) -> None:
        rc = self._L.fcp_process_feature_columns(self.plan.handle, C.byref(a), C.byref(res))
        if state.get("error") is not None:
            raise state["error"]
        _lib.check(rc, "FeatureColumnProcess")

    def groups_only(self, concated_inputs, concated_offsets, concated_shapes, inputs, symbols=None,
                    stream: Optional[int] = None, arena=None) -> list:
        """Lean call: returns only the per-group concat matrices (no per-column pointer /
        shape arrays are materialised in Python).  FCP_LAYOUT_CONCAT plans only.  ``arena``: as for ``__call__``."""
        torch = self.torch
        a, keep = self._args(concated_inputs, concated_offsets, concated_shapes, inputs, symbols, stream, arena)
        g = self.spec.n_groups
        _grp_ptrs = (C.c_void_p * g)()
        _grp_shapes = (C.c_int32 * (2 * g))()
        res = _lib.ProcessResult(None, None, None, _grp_ptrs, _grp_shapes, None, 0)
        self._process(a, res, keep[5])
        arena = keep[5]["arena"]
        if getattr(self.plan, "private_streams", 0):
            _lib.check(self._L.fcp_result_wait(arena.data_ptr(), a.stream), "fcp_result_wait")
        f = _typed_arena(torch, arena, self.out_dtype)
        out = []
        for gi in range(g):
            rows, width = _grp_shapes[2 * gi], _grp_shapes[2 * gi + 1]
            off = ((_grp_ptrs[gi] or arena.data_ptr()) - arena.data_ptr()) // f.element_size()
            out.append(f[off:off + rows * width].view(rows, width))
        return out

    def __call__(self, concated_inputs, concated_offsets, concated_shapes, inputs, symbols=None,
                 stream: Optional[int] = None, defer_wait: bool = False, arena=None) -> ProcessOutputs:
        """``defer_wait`` (plans with private streams only): do not order ``stream`` behind the result here; the reader
        calls ``ProcessOutputs.wait`` — the split between FeatureColumnProcess and ConcatOutputs in the rewritten
        graph.  Default: the wait is enqueued at once, so torch code on ``stream`` may read the result as always.
        ``arena``: a caller-owned contiguous torch.uint8 tensor on the op's device that the request writes its outputs
        into instead of a fresh allocation (at least ``Plan.arena_bytes(shapes, symbols)`` bytes, else ValueError) — the
        caller decides whether consecutive requests reuse an arena, which the output store policy depends on."""
        torch = self.torch
        a, keep = self._args(concated_inputs, concated_offsets, concated_shapes, inputs, symbols, stream, arena)
        n, g = self.spec.n_columns, self.spec.n_groups
        _out_ptrs = (C.c_void_p * n)()
        _out_shapes = (C.c_int32 * (2 * n))()
        _out_strides = (C.c_int64 * n)()
        _grp_ptrs = (C.c_void_p * g)()
        _grp_shapes = (C.c_int32 * (2 * g))()
        res = _lib.ProcessResult(_out_ptrs, _out_shapes, _out_strides, _grp_ptrs, _grp_shapes, None, 0)
        self._process(a, res, keep[5])
        arena = keep[5]["arena"]
        if getattr(self.plan, "private_streams", 0) and not defer_wait:
            _lib.check(self._L.fcp_result_wait(arena.data_ptr(), a.stream), "fcp_result_wait")
        out_ptrs = np.array([_out_ptrs[k] or 0 for k in range(n)], np.int64)
        out_shapes = np.array(_out_shapes[:], np.int32)
        strides = np.array(_out_strides[:], np.int64)
        gshapes = np.array(_grp_shapes[:], np.int32)
        groups = []
        if self.spec.layout == LAYOUT_CONCAT:
            f = _typed_arena(torch, arena, self.out_dtype)
            for gi in range(g):
                rows, width = int(gshapes[2 * gi]), int(gshapes[2 * gi + 1])
                off = ((_grp_ptrs[gi] or arena.data_ptr()) - arena.data_ptr()) // f.element_size()
                groups.append(f[off:off + rows * width].view(rows, width))
        return ProcessOutputs(out_ptrs, out_shapes, strides, arena, groups, gshapes)

    def table_rows(self) -> tuple:
        """``Plan.table_rows``."""
        return self.plan.table_rows()

    def traffic_bind(self, counts, skipped=None) -> None:
        """``Plan.traffic_bind``."""
        self.plan.traffic_bind(counts, skipped)

    def traffic_count(self, concated_inputs, concated_offsets, concated_shapes, inputs=None, symbols=None,
                      stream: Optional[int] = None) -> None:
        """``Plan.traffic_count`` with the arguments of ``__call__``: a sampled request is counted with the very arguments it
        is served with.  ``inputs`` (the tables) is accepted and not looked at."""
        self.plan.traffic_count(concated_inputs, concated_offsets, concated_shapes, symbols, stream)

    def shard_finalize(self, concated_inputs, concated_offsets, concated_shapes, inputs, symbols, group: int,
                       partial_slices, world: int, row_begin: int, row_count: int, stream: Optional[int] = None, out=None):
        """Sum ``world`` partial slices in rank order + mean division; columns with one owner per row take
        the owner's value.  ``out``: a contiguous float32 [row_count, width] device tensor to write into (its EXTERNAL
        holes are left alone), else a fresh one."""
        torch = self.torch
        a, _keep = self._args(concated_inputs, concated_offsets, concated_shapes, inputs, symbols, stream)
        width = self.plan.group_width(group)
        if out is None:
            out = torch.empty((row_count, width), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (row_count, width) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"shard_finalize: out= must be a contiguous float32 [{row_count}, {width}] tensor")
        _lib.check(self._L.fcp_shard_finalize(self.plan.handle, C.byref(a), group, partial_slices.data_ptr(),
                                              world, row_begin, row_count, out.data_ptr(), a.stream),
                   "fcp_shard_finalize")
        return out


# ----------------------------------------------------------------------------
# Addons>ConcatOutputs[NoHost]
# ----------------------------------------------------------------------------
def concat_outputs(device_inputs: Sequence, stream: Optional[int] = None):
    """``out[p, off_k:off_k+dim_k] = in_k[p, :]`` for device tensors ``in_k``
    of shape ``[prefix..., dim_k]`` (``ConcatOutputsKnl``,
    ``concat_outputs_op_gpu.cu.cc:85-131``).  Needed only with
    ``LAYOUT_PER_COLUMN``; the fused path writes the concat layout directly."""
    import torch
    L = _lib.load()
    ins = [t.contiguous() for t in device_inputs]
    if not ins:
        raise ValueError("concat_outputs needs at least one input")
    prefix_shape = tuple(ins[0].shape[:-1])
    for t in ins:
        if tuple(t.shape[:-1]) != prefix_shape:
            raise ValueError("concat_outputs: prefix shapes differ")
        if t.element_size() != 4:
            raise ValueError("concat_outputs supports 4-byte types (float, int)")
    prefix = int(np.prod(prefix_shape)) if prefix_shape else 1
    dims = np.asarray([t.shape[-1] for t in ins], np.int32)
    out = torch.empty(prefix_shape + (int(dims.sum()),), dtype=ins[0].dtype, device=ins[0].device)
    ptrs = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    if stream is None:
        stream = torch.cuda.current_stream(ins[0].device).cuda_stream
    _lib.check(L.fcp_concat_outputs(ptrs, dims.ctypes.data, len(ins), prefix, out.data_ptr(), stream),
               "ConcatOutputs")
    return out


def _temp_allocator(device):
    """malloc_temp callback (the op's allocate_temp): torch tensors kept alive by the returned list."""
    import torch
    keep = []

    def _alloc(_ctx, nbytes):
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        keep.append(t)
        return t.data_ptr()

    return keep, _lib.ALLOC_FN(_alloc)


def concat_outputs_scatter(device_inputs: Sequence, col_offsets: Sequence[int], out, stream: Optional[int] = None):
    """``out[p, col_offsets[k] : +dim_k] = in_k[p, :]`` into an existing row-major matrix ``out``
    (``ScatterBlock<EmbedDim, Offset>``, ``concat_outputs_op_gpu.cu.cc:85-99``, run-time offsets)."""
    import torch
    L = _lib.load()
    ins = [t.contiguous() for t in device_inputs]
    if not ins:
        return out
    assert out.is_contiguous() and out.element_size() == 4
    width = int(out.shape[-1])
    prefix = int(out.numel() // max(width, 1))
    dims = np.asarray([t.shape[-1] for t in ins], np.int32)
    offs = np.asarray(col_offsets, np.int32)
    ptrs = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    if stream is None:
        stream = torch.cuda.current_stream(out.device).cuda_stream
    _lib.check(L.fcp_concat_outputs_scatter(ptrs, dims.ctypes.data, offs.ctypes.data, len(ins), prefix, width,
                                            out.data_ptr(), stream), "ConcatOutputs")
    return out


def concat_outputs_host(host_inputs: Sequence[np.ndarray], col_offsets: Sequence[int], out,
                        stream: Optional[int] = None):
    """The ``host_inputs`` half of ``Addons>ConcatOutputs`` (``concat_outputs_op_gpu.cu.cc:186-216``):
    host tensors ``[prefix..., dim_k]`` -> one pinned staging buffer -> one H2D copy -> scattered into
    columns ``[col_offsets[k], +dim_k)`` of the device matrix ``out`` (the group's matrix inside the
    FeatureColumnProcess arena when the plan reserves ``FORM_EXTERNAL`` slots for them)."""
    import torch
    L = _lib.load()
    arrs = [np.require(np.asarray(a), requirements="C") for a in host_inputs]
    if not arrs:
        return out
    for a in arrs:
        if a.dtype.itemsize != 4:
            raise ValueError("ConcatOutputs supports 4-byte types (float, int)")
    assert out.is_contiguous() and out.element_size() == 4
    width = int(out.shape[-1])
    prefix = int(out.numel() // max(width, 1))
    for a in arrs:
        if a.size != prefix * a.shape[-1]:
            raise ValueError("ConcatOutputs: prefix shapes differ")
    dims = np.asarray([a.shape[-1] for a in arrs], np.int32)
    offs = np.asarray(col_offsets, np.int32)
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    if stream is None:
        stream = torch.cuda.current_stream(out.device).cuda_stream
    keep, cb = _temp_allocator(out.device)
    _lib.check(L.fcp_concat_outputs_host(ptrs, dims.ctypes.data, offs.ctypes.data, len(arrs), prefix, width,
                                         out.data_ptr(), cb, None, out.device.index or 0, stream), "ConcatOutputs")
    out._fcp_keep = keep  # the staging scratch must outlive the enqueued copy + scatter
    return out


class ConcatOutputs:
    """``Addons>ConcatOutputs`` / ``Addons>ConcatOutputsNoHost`` with the reference's attrs
    (``concat_outputs_op_gpu.cu.cc:39-79, 180-235``; written by ``Rewrite``,
    ``cuda_emitter.cc:2534-2647``) — what ``tf_shim/fcp_tf_ops.cc::ConcatOutputsOp`` does, in Python.

    With ``FCP_LAYOUT_CONCAT`` the FeatureColumnProcess arena already holds the group's
    ``[prefix, sum(embedd_dims)]`` matrix: device columns sit at their concat offsets, host columns are
    ``FORM_EXTERNAL`` holes.  The op checks that (pointer arithmetic on ``device_input_ptrs``), copies the
    ``host_inputs`` into the holes and returns the matrix as a view of the arena — no second pass over
    the pooled data, no stream synchronisation."""

    def __init__(self, N: int, embedd_dims: Sequence[int], device_input_indices: Sequence[int],
                 device_concat_indices: Sequence[int], host_concat_indices: Sequence[int], prefix_begin: int,
                 prefix_end: int) -> None:
        if N != len(host_concat_indices):
            raise ValueError("N != host_concat_indices.size()")
        if len(device_input_indices) != len(device_concat_indices):
            raise ValueError("device_input_indices.size() != device_concat_indices.size()")
        if len(embedd_dims) != len(device_concat_indices) + len(host_concat_indices):
            raise ValueError("embedd_dims.size() != device_concat_indices.size() + host_concat_indices.size()")
        if not device_input_indices:
            raise ValueError("ConcatOutputs without device inputs")
        self.dims = [int(d) for d in embedd_dims]
        self.scan = np.concatenate([[0], np.cumsum(self.dims)]).astype(np.int64)   # output_scans, :74-79
        self.dev_in, self.dev_pos = list(device_input_indices), list(device_concat_indices)
        self.host_pos = list(host_concat_indices)
        self.prefix_begin, self.prefix_end = prefix_begin, prefix_end

    def __call__(self, device_input_ptrs: np.ndarray, device_input_shapes: np.ndarray, host_inputs: Sequence[np.ndarray],
                 arena, stream: Optional[int] = None):
        import torch
        prefix_shape = tuple(int(x) for x in device_input_shapes[self.prefix_begin:self.prefix_end])
        prefix = int(np.prod(prefix_shape)) if prefix_shape else 1
        width = int(self.scan[-1])
        base = int(device_input_ptrs[self.dev_in[0]]) - 4 * int(self.scan[self.dev_pos[0]])
        for i, pos in zip(self.dev_in, self.dev_pos):
            if int(device_input_ptrs[i]) - base != 4 * int(self.scan[pos]):
                raise ValueError("ConcatOutputs: the plan's concat layout does not match embedd_dims "
                                 "(the column plan must reserve FORM_EXTERNAL slots for host concat inputs)")
        begin = base - arena.data_ptr()
        nbytes = prefix * width * 4
        if begin < 0 or begin + nbytes > arena.numel() * arena.element_size():
            raise ValueError("ConcatOutputs: group outside the arena")
        out = arena.view(torch.uint8)[begin:begin + nbytes].view(torch.float32).view(prefix_shape + (width,))
        # the lookup kernels may run on one of the plan's private streams: this op's stream — and everything downstream of
        # its output — waits for them on the device (a no-op when private streams are off; tf_shim/fcp_tf_ops.cc does the same)
        if stream is None:
            stream = torch.cuda.current_stream(arena.device).cuda_stream
        _lib.check(_lib.load().fcp_result_wait(arena.data_ptr(), stream), "fcp_result_wait")
        if len(host_inputs) != len(self.host_pos):
            raise ValueError("ConcatOutputs: wrong number of host inputs")
        if host_inputs:
            for a, pos in zip(host_inputs, self.host_pos):
                if np.asarray(a).shape[-1] != self.dims[pos]:
                    raise ValueError("ConcatOutputs: host input width != embedd_dims entry")
            concat_outputs_host(host_inputs, [int(self.scan[p]) for p in self.host_pos], out, stream)
        return out


# ----------------------------------------------------------------------------
# request staging: ConcatInputs + H2D in one step
# ----------------------------------------------------------------------------
class RequestStager:
    """Ring of pinned host buffers with device twins: ``stage(inputs)`` packs the host
    tensors exactly like :func:`concat_inputs` (multi-threaded, straight into pinned
    memory) and enqueues one async H2D copy on the stager's copy stream (``stream`` waits
    for it).  Returns ``(device_blob_ptr, nbytes, offsets, shapes)``; the device blob
    stays valid for the next ``depth - 1`` calls.  ``zero_copy``: no copy — the "device blob" is the pinned
    ring itself, mapped into the device's address space (``FCP_STAGER_ZERO_COPY``)."""

    def __init__(self, capacity_bytes: int, max_inputs: int, max_rank_sum: int, device: int = 0, depth: int = 4,
                 n_threads: int = 8, zero_copy: bool = False, copy: Optional[str] = None) -> None:
        """``copy``: "kernel" (``FCP_STAGER_COPY_KERNEL``, the default: a kernel on the stager's stream reads the pinned
        ring) or "sdma" (``FCP_STAGER_COPY_SDMA``: ``hipMemcpyAsync``)."""
        self._L = _lib.load()
        h = C.c_void_p()
        flags = (1 if zero_copy else 0) | {None: 0, "kernel": 2, "sdma": 4}[copy]
        _lib.check(self._L.fcp_stager_create_ex(device, capacity_bytes, max_inputs, max_rank_sum, depth, n_threads,
                                                flags, C.byref(h)), "fcp_stager_create_ex")
        self.handle = h

    def stats(self) -> dict:
        """``fcp_stager_stats``: staging calls, copy calls, copy calls that held their host thread > 1 ms, the slowest."""
        st = _lib.StagerStats()
        _lib.check(self._L.fcp_stager_stats(self.handle, C.byref(st)), "fcp_stager_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def stage_ex(self, inputs: Sequence[np.ndarray], modes: Sequence[int], mode_args: Sequence[int],
                 stream: Optional[int] = None):
        """``fcp_stager_stage_ex``: ``modes[i]`` in ``plan.STAGE_*`` (``PlanSpec.staged()`` gives them and the matching
        plan); ``mode_args[i]`` = number of rows for ``STAGE_SEG_TO_CSR`` inputs."""
        import torch
        arrs = [np.require(np.asarray(a), requirements="C") for a in inputs]
        n = len(arrs)
        dims_keep = [np.asarray(a.shape, np.int64) for a in arrs]
        tens = (_lib.HostTensor * max(n, 1))()
        for i, a in enumerate(arrs):
            tens[i] = _lib.HostTensor(a.ctypes.data, a.dtype.itemsize, a.ndim, dims_keep[i].ctypes.data_as(C.POINTER(C.c_int64)))
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        blob, nbytes = C.c_void_p(), C.c_int64()
        offs, shps = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        m = np.asarray(list(modes), np.uint8)
        a64 = np.asarray(list(mode_args), np.int64)
        _lib.check(self._L.fcp_stager_stage_ex(self.handle, tens, n, m.ctypes.data, a64.ctypes.data, stream, C.byref(blob),
                                               C.byref(nbytes), C.byref(offs), C.byref(shps)), "fcp_stager_stage_ex")
        rank_sum = sum(1 if mm == 2 else a.ndim for mm, a in zip(m, arrs))
        offsets = np.ctypeslib.as_array(offs, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        shapes = np.ctypeslib.as_array(shps, shape=(rank_sum,)).copy() if rank_sum else np.zeros(0, np.int32)
        return blob.value, nbytes.value, offsets, shapes

    def stage(self, inputs: Sequence[np.ndarray], stream: Optional[int] = None,
              narrow: Optional[Sequence[bool]] = None):
        """``narrow[i]``: ship int64 input ``i`` as int32 (``PlanSpec.narrowed()`` gives the
        flags and the matching plan)."""
        import torch
        arrs = [np.require(np.asarray(a), requirements="C") for a in inputs]
        n = len(arrs)
        dims_keep = [np.asarray(a.shape, np.int64) for a in arrs]
        tens = (_lib.HostTensor * max(n, 1))()
        for i, a in enumerate(arrs):
            tens[i] = _lib.HostTensor(a.ctypes.data, a.dtype.itemsize, a.ndim,
                                      dims_keep[i].ctypes.data_as(C.POINTER(C.c_int64)))
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        blob, nbytes = C.c_void_p(), C.c_int64()
        offs, shps = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        flags = None
        if narrow is not None:
            flags = (C.c_uint8 * max(n, 1))(*[1 if f else 0 for f in narrow])
        _lib.check(self._L.fcp_stager_stage_narrow(self.handle, tens, n, flags, stream, C.byref(blob),
                                                   C.byref(nbytes), C.byref(offs), C.byref(shps)),
                   "fcp_stager_stage")
        rank_sum = sum(a.ndim for a in arrs)
        offsets = np.ctypeslib.as_array(offs, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        shapes = np.ctypeslib.as_array(shps, shape=(rank_sum,)).copy() if rank_sum else np.zeros(0, np.int32)
        return blob.value, nbytes.value, offsets, shapes

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._L.fcp_stager_destroy(self.handle)
            self.handle = None
