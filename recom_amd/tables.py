"""Table conversion on the device (``fcp_table_convert``, recom_amd/csrc/fcp_convert.hip): float32 embedding tables to the
formats the plans read — bf16, fp16 and 8-bit row-quantised ("q8") — and back, on torch device tensors; and rows of such a
table written and read back by id (``fcp_table_update_rows`` / ``fcp_table_read_rows``, recom_amd/csrc/fcp_table_rows.hip);
and, in front of both, the audit of a float32 table against all three formats in one pass (``fcp_table_audit``,
recom_amd/csrc/fcp_table_audit.hip) with the choice of one format per table from a byte budget (``fcp_table_formats_choose``);
and the rows' read counts, taken from request ids on the device (``fcp_table_count_ids``, recom_amd/csrc/fcp_table_traffic.hip),
by which the audit weighs its sums (``fcp_table_audit_weighted``); ``new_plan_counts`` makes the count tensors of a whole plan,
which ``Plan.traffic_bind`` / ``Plan.traffic_count`` (recom_amd/ops.py) fill from requests through the plan's own id path;
and the digest of a table of any format — an order-free 64-bit sum of row hashes, on the device (``fcp_table_digest`` /
``fcp_table_digest_rows``, recom_amd/csrc/fcp_table_digest.hip) and from host memory (``fcp_table_digest_host``) — by which a
deployment checks that a served table is, byte for byte, the table it should be, and keeps that check across ``update_rows``
— for a whole model's tables in one call (``fcp_tables_digest``, recom_amd/csrc/fcp_tables_digest.hip: ``digests_grouped``,
``digest_rows_grouped``, ``update_rows_grouped_tracked``, ``digest_tables``);
and, for deltas that name a row more than once, the ids made distinct on the device with the last occurrence winning
(``fcp_table_delta_distinct``, recom_amd/csrc/fcp_table_delta.hip), in front of ``update_rows`` and the digest bookkeeping, which
both ask for distinct ids and do not check (``apply_delta``);
and, for a trainer that ships a whole new float32 master instead of a delta, the rows of a served table whose stored bytes
would change, found on the device in one pass without a temporary table (``fcp_table_diff``,
recom_amd/csrc/fcp_table_diff.hip: ``diff``, ``diff_from_host``, ``sync_from_host``).

Plans do not quantise; this does, once, at load time.  The value model is the header's (include/fcp_hip.h): float32 -> q8 is
exactly the tensor ``quantized::embedding_bag_byte_prepack`` returns, q8 -> float32 is ``fma(code, scale, bias)`` rounded
once, float32 -> 16-bit is one rounding to nearest-even, 16-bit -> float32 is exact.  Nothing here falls back to torch: a
missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, Optional, Sequence

from . import lib as _lib
from .plan import FORM_GATHER, FORM_GATHER_SCATTER, FORM_SEGMENT_REDUCE, TABLE_FORMATS, PlanSpec

_FORMS_WITH_TABLES = (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER)


def _torch_dtypes():
    import torch
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "q8": torch.uint8}


def row_bytes(dtype: str, dim: int) -> int:
    """``fcp_table_row_bytes``: bytes of one row of a ``dtype`` ("f32" | "bf16" | "f16" | "q8") table of width ``dim``."""
    if dtype not in _lib.TABLE_KINDS:
        raise ValueError(f"unknown table dtype {dtype!r}")
    n = int(_lib.load().fcp_table_row_bytes(_lib.TABLE_KINDS[dtype], int(dim)))
    if n < 0:
        raise ValueError(f"no {dtype} table has rows of dim {dim}")
    return n


def _kind_and_dim(t, what: str):
    """(table dtype name, dim) of a 2-D contiguous device tensor in one of the four table formats."""
    names = {v: k for k, v in _torch_dtypes().items()}
    if t.dtype not in names:
        raise ValueError(f"{what}: {t.dtype} is no table format (float32, bfloat16, float16, or uint8 [rows, dim + 8])")
    if t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{what}: a table is a contiguous 2-D tensor")
    if not t.is_cuda:
        raise ValueError(f"{what}: fcp_table_convert works device to device; the tensor is on {t.device}")
    name = names[t.dtype]
    dim = t.shape[1] - TABLE_FORMATS[name].row_tail
    if dim <= 0:
        raise ValueError(f"{what}: a {name} table of shape {tuple(t.shape)} has no elements in a row")
    return name, int(dim)


def convert(src, dtype: str, out=None, dst_row0: int = 0, stream: Optional[int] = None):
    """Convert the table rows ``src`` (a device tensor: float32 / bfloat16 / float16 ``[rows, dim]`` or uint8
    ``[rows, dim + 8]``) to ``dtype``; exactly one side is float32.  ``out``: the WHOLE destination table (the rows land at
    row ``dst_row0`` and below it), allocated as ``[rows, dim]`` / ``[rows, dim + 8]`` when not given.  Asynchronous on
    ``stream`` (a hipStream_t; torch's current stream of the device by default).  Returns ``out``."""
    import torch
    if dtype not in _lib.TABLE_KINDS:
        raise ValueError(f"unknown table dtype {dtype!r}")
    src_name, dim = _kind_and_dim(src, "src")
    rows = int(src.shape[0])
    if out is None:
        if dst_row0:
            raise ValueError("dst_row0 needs out=: the whole destination table")
        out = torch.empty((rows, dim + TABLE_FORMATS[dtype].row_tail), dtype=_torch_dtypes()[dtype], device=src.device)
    out_name, out_dim = _kind_and_dim(out, "out")
    if out_name != dtype or out_dim != dim:
        raise ValueError(f"out is a {out_name} table of dim {out_dim}; the call writes a {dtype} table of dim {dim}")
    if out.device != src.device:
        raise ValueError(f"src is on {src.device}, out on {out.device}")
    if dst_row0 < 0 or dst_row0 + rows > out.shape[0]:
        raise ValueError(f"rows [{dst_row0}, {dst_row0 + rows}) do not lie in a table of {out.shape[0]} rows")
    if stream is None:
        stream = torch.cuda.current_stream(src.device).cuda_stream
    status = _lib.load().fcp_table_convert(C.c_void_p(out.data_ptr()), _lib.TABLE_KINDS[dtype], int(dst_row0),
                                           C.c_void_p(src.data_ptr()), _lib.TABLE_KINDS[src_name], rows, dim,
                                           src.device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_table_convert")
    return out


def convert_tables(spec: PlanSpec, tables: Sequence, table_dtype: str, stream: Optional[int] = None) -> list:
    """The device inputs of ``spec`` with every table a lookup column reads converted to ``table_dtype`` — what
    ``spec.with_table_dtype(table_dtype)`` serves.  Inputs no column reads as a table, and tables that already are of that
    dtype, are passed through; a table shared by several columns is converted once."""
    want = _torch_dtypes()[table_dtype]
    read = {c.table_input for c in spec.columns if c.form in _FORMS_WITH_TABLES and c.table_input >= 0}
    return [convert(t, table_dtype, stream=stream) if i in read and t.dtype != want else t for i, t in enumerate(tables)]


def convert_from_host(table_cpu, dtype: str, device, chunk_rows: int = 1 << 16):
    """A host table (torch CPU tensor, float32 ``[rows, dim]``) to a ``dtype`` table on ``device``, streamed through ONE
    pinned bounce buffer and one device buffer of ``chunk_rows`` rows: the device never holds the float32 table.  Chunks
    land at their row index (``dst_row0``).  The copy of a chunk waits for the conversion of the one before (one buffer);
    returns after the last conversion is enqueued on torch's current stream."""
    import torch
    if table_cpu.dtype != torch.float32 or table_cpu.dim() != 2 or table_cpu.is_cuda:
        raise ValueError("convert_from_host takes a float32 [rows, dim] tensor on the host")
    if chunk_rows <= 0:
        raise ValueError("chunk_rows must be positive")
    device = torch.device(device)
    rows, dim = (int(v) for v in table_cpu.shape)
    out = torch.empty((rows, dim + TABLE_FORMATS[dtype].row_tail), dtype=_torch_dtypes()[dtype], device=device)
    chunk = min(chunk_rows, max(rows, 1))
    bounce = torch.empty((chunk, dim), dtype=torch.float32, pin_memory=True)
    staged = torch.empty((chunk, dim), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            stream.synchronize()                      # the bounce buffer's last copy has left it
            bounce[:n].copy_(table_cpu[r0:r0 + n])
            staged[:n].copy_(bounce[:n], non_blocking=True)
            convert(staged[:n], dtype, out=out, dst_row0=r0, stream=stream.cuda_stream)
    return out


# ---- rows by id (fcp_table_update_rows / fcp_table_read_rows) --------------------------------------------------------------
def _ids_of(torch, table, row_ids):
    if row_ids.dtype != torch.int64 or row_ids.dim() != 1 or not row_ids.is_contiguous():
        raise ValueError("row_ids is a contiguous int64 [n] tensor")
    if row_ids.device != table.device:
        raise ValueError(f"table is on {table.device}, row_ids on {row_ids.device}")
    return int(row_ids.shape[0])


def _rows_of(torch, table, dim: int, n: int, rows, what: str) -> None:
    if rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError(f"{what} is a contiguous float32 [n, dim] tensor")
    if rows.device != table.device:
        raise ValueError(f"table is on {table.device}, {what} on {rows.device}")
    if rows.shape[0] != n:
        raise ValueError(f"{what} has {rows.shape[0]} rows, row_ids names {n}")
    if rows.shape[1] != dim:
        raise ValueError(f"{what} has rows of dim {rows.shape[1]}; the table's are of dim {dim}")


def update_rows(table, row_ids, rows, skipped=None, stream: Optional[int] = None):
    """``fcp_table_update_rows``: write the float32 ``rows`` ``[n, dim]`` into ``table`` (a device tensor in one of the four
    table formats) at the row indices ``row_ids`` (int64 ``[n]``, pairwise distinct — not checked), each converted as
    ``convert`` converts float32 to the table's format.  Ids outside the table are skipped; ``skipped``, an int64 device
    tensor of one element, is increased by their number (the caller zeroes it).  Asynchronous on ``stream`` (torch's current
    stream of the device by default).  Returns ``table``."""
    import torch
    name, dim = _kind_and_dim(table, "table")
    n = _ids_of(torch, table, row_ids)
    _rows_of(torch, table, dim, n, rows, "rows")
    if skipped is not None:
        if skipped.dtype != torch.int64 or skipped.numel() != 1 or skipped.device != table.device:
            raise ValueError("skipped is an int64 tensor of one element on the table's device")
    if stream is None:
        stream = torch.cuda.current_stream(table.device).cuda_stream
    status = _lib.load().fcp_table_update_rows(C.c_void_p(table.data_ptr()), _lib.TABLE_KINDS[name], int(table.shape[0]), dim,
                                               C.c_void_p(row_ids.data_ptr()), C.c_void_p(rows.data_ptr()), n,
                                               C.c_void_p(skipped.data_ptr()) if skipped is not None else None,
                                               table.device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_table_update_rows")
    return table


def read_rows(table, row_ids, out=None, stream: Optional[int] = None):
    """``fcp_table_read_rows``: the float32 values a plan reads at ``row_ids`` (int64 ``[n]``) of ``table`` — a row of +0.0
    for an id outside the table.  ``out``: float32 ``[n, dim]`` on the table's device, allocated when not given.
    Asynchronous on ``stream`` (torch's current stream of the device by default).  Returns ``out``."""
    import torch
    name, dim = _kind_and_dim(table, "table")
    n = _ids_of(torch, table, row_ids)
    if out is None:
        out = torch.empty((n, dim), dtype=torch.float32, device=table.device)
    _rows_of(torch, table, dim, n, out, "out")
    if stream is None:
        stream = torch.cuda.current_stream(table.device).cuda_stream
    status = _lib.load().fcp_table_read_rows(C.c_void_p(out.data_ptr()), C.c_void_p(table.data_ptr()), _lib.TABLE_KINDS[name],
                                             int(table.shape[0]), dim, C.c_void_p(row_ids.data_ptr()), n,
                                             table.device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_table_read_rows")
    return out


# ---- rows by id, many tables in one call (fcp_tables_update_rows / fcp_tables_read_rows) --------------------------------------
def _entries_of(struct, tables_, entry_of):
    """The ``struct`` array of a grouped call and the one device all of it lives on (``None`` for no entries):
    ``entry_of(k, table)`` validates entry k and returns the arguments of its struct; what it refuses goes behind "entry k: "."""
    entries = (struct * max(len(tables_), 1))()
    device = None
    for k, t in enumerate(tables_):
        try:
            args = entry_of(k, t)
        except ValueError as e:
            raise ValueError(f"entry {k}: {e}") from None
        if device is None:
            device = t.device
        elif t.device != device:
            raise ValueError(f"entry {k}: table is on {t.device}, entry 0's on {device}")
        entries[k] = struct(*args)
    return entries, device


def _as_streams(torch, device, stream: int, *shapes) -> list:
    """int64 device tensors of ``shapes``, in that order, allocated as that stream's: a block the caching allocator hands out
    may still have work pending on the stream it was freed on.  A workspace of N bytes is ``(N // 8,)``."""
    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device)):
        return [torch.empty(shape, dtype=torch.int64, device=device) for shape in shapes]


def _grouped_entries(torch, tables_, row_ids, rows, what: str):
    """The ``fcp_table_rows_t`` array of equally long sequences, each entry validated as ``update_rows`` / ``read_rows``
    validate theirs, and the one device all of it lives on (``None`` for no entries)."""
    if len(row_ids) != len(tables_) or len(rows) != len(tables_):
        raise ValueError(f"tables names {len(tables_)} entries, row_ids {len(row_ids)}, {what} {len(rows)}")

    def entry_of(k, t):
        name, dim = _kind_and_dim(t, "table")
        n = _ids_of(torch, t, row_ids[k])
        _rows_of(torch, t, dim, n, rows[k], what)
        return t.data_ptr(), row_ids[k].data_ptr(), rows[k].data_ptr(), int(t.shape[0]), n, _lib.TABLE_KINDS[name], dim
    return _entries_of(_lib.TableRows, tables_, entry_of)


def _grouped_workspace(torch, L, device, stream: int, n_tables: int):
    """the call's workspace, allocated as that stream's"""
    return _as_streams(torch, device, stream, (int(L.fcp_tables_rows_workspace_bytes(n_tables)) // 8,))[0]


def update_rows_grouped(tables, row_ids, rows, skipped=None, stream: Optional[int] = None):
    """``fcp_tables_update_rows``: ``update_rows`` for a whole model's delta in ONE call — ``tables``, ``row_ids`` and ``rows``
    are equally long sequences, entry k what ``update_rows(tables[k], row_ids[k], rows[k])`` takes, in any mix of formats and
    dims on one device; the number of launches does not grow with their length.  Every table ends up, byte for byte, as
    after one ``update_rows`` per entry.  ``skipped``: one int64 ``[len(tables)]`` device tensor; element k is increased by
    entry k's ids outside its table (the caller zeroes it).  Two entries may name one table if their ids are distinct
    together.  Asynchronous on ``stream`` (torch's current stream of the device by default).  Returns ``tables``."""
    import torch
    entries, device = _grouped_entries(torch, tables, row_ids, rows, "rows")
    n_tables = len(tables)
    if skipped is not None:
        if skipped.dtype != torch.int64 or skipped.dim() != 1 or skipped.shape[0] != n_tables or not skipped.is_contiguous() or \
                (device is not None and skipped.device != device):
            raise ValueError("skipped is a contiguous int64 [len(tables)] tensor on the tables' device")
    if device is None:
        return tables
    L = _lib.load()
    stream = _stream_of(torch, device, stream)
    workspace = _grouped_workspace(torch, L, device, stream, n_tables)
    status = L.fcp_tables_update_rows(entries, n_tables, C.c_void_p(skipped.data_ptr()) if skipped is not None else None,
                                      C.c_void_p(workspace.data_ptr()), device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_tables_update_rows")
    return tables


def read_rows_grouped(tables, row_ids, out=None, stream: Optional[int] = None) -> list:
    """``fcp_tables_read_rows``: ``read_rows`` of many tables in ONE call — entry k gives what
    ``read_rows(tables[k], row_ids[k])`` gives, bit for bit, a row of +0.0 for an id outside the table.  ``out``: a sequence
    of float32 ``[n_k, dim_k]`` tensors on the tables' device, allocated when not given.  Asynchronous on ``stream`` (torch's
    current stream of the device by default).  Returns the list of outputs."""
    import torch
    if len(row_ids) != len(tables):
        raise ValueError(f"tables names {len(tables)} entries, row_ids {len(row_ids)}")
    if len(tables) and getattr(tables[0], "is_cuda", False):
        stream = _stream_of(torch, tables[0].device, stream)
    if out is None:
        out = []
        for k, (t, ids) in enumerate(zip(tables, row_ids)):
            try:
                _name, dim = _kind_and_dim(t, "table")
                n = _ids_of(torch, t, ids)
            except ValueError as e:
                raise ValueError(f"entry {k}: {e}") from None
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=t.device)):
                out.append(torch.empty((n, dim), dtype=torch.float32, device=t.device))
    out = list(out)
    entries, device = _grouped_entries(torch, tables, row_ids, out, "out")
    if device is None:
        return out
    L = _lib.load()
    workspace = _grouped_workspace(torch, L, device, stream, len(tables))
    status = L.fcp_tables_read_rows(entries, len(tables), C.c_void_p(workspace.data_ptr()), device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_tables_read_rows")
    return out


def update_from_host(table, ids_cpu, rows_cpu, chunk_rows: int = 1 << 16):
    """A host delta — ``ids_cpu`` int64 ``[n]`` and ``rows_cpu`` float32 ``[n, dim]``, torch CPU tensors — into the device
    ``table``, streamed through ONE pinned bounce buffer and one device buffer of ``chunk_rows`` rows (and as many ids), as
    ``convert_from_host`` streams a table.  The copy of a chunk waits for the update of the one before; returns ``table``
    after the last update is enqueued on torch's current stream."""
    import torch
    if ids_cpu.dtype != torch.int64 or ids_cpu.dim() != 1 or ids_cpu.is_cuda:
        raise ValueError("update_from_host takes an int64 [n] tensor of ids on the host")
    if rows_cpu.dtype != torch.float32 or rows_cpu.dim() != 2 or rows_cpu.is_cuda:
        raise ValueError("update_from_host takes a float32 [n, dim] tensor of rows on the host")
    if chunk_rows <= 0:
        raise ValueError("chunk_rows must be positive")
    _name, dim = _kind_and_dim(table, "table")
    n = int(ids_cpu.shape[0])
    if rows_cpu.shape[0] != n:
        raise ValueError(f"rows has {rows_cpu.shape[0]} rows, ids names {n}")
    if rows_cpu.shape[1] != dim:
        raise ValueError(f"rows has rows of dim {rows_cpu.shape[1]}; the table's are of dim {dim}")
    device = table.device
    chunk = min(chunk_rows, max(n, 1))
    bounce = torch.empty((chunk, dim), dtype=torch.float32, pin_memory=True)
    bounce_ids = torch.empty((chunk,), dtype=torch.int64, pin_memory=True)
    staged = torch.empty((chunk, dim), dtype=torch.float32, device=device)
    staged_ids = torch.empty((chunk,), dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        for r0 in range(0, n, chunk):
            m = min(chunk, n - r0)
            stream.synchronize()                      # the bounce buffers' last copies have left them
            bounce[:m].copy_(rows_cpu[r0:r0 + m])
            bounce_ids[:m].copy_(ids_cpu[r0:r0 + m])
            staged[:m].copy_(bounce[:m], non_blocking=True)
            staged_ids[:m].copy_(bounce_ids[:m], non_blocking=True)
            update_rows(table, staged_ids[:m], staged[:m], stream=stream.cuda_stream)
    return table


# ---- audit and formats by budget (fcp_table_audit / fcp_table_formats_choose) ------------------------------------------------
@dataclasses.dataclass(frozen=True)
class KindAudit:
    """fcp_table_audit_kind_t: one format's verdict on a float32 table."""
    rows_bad: int          # finite rows the format cannot hold (an element rounds to +-inf; q8: max - min overflows)
    first_bad_row: int     # -1 if none
    sum_sq_err: float      # float64 sum over the good rows of e * e, e = x - rt(x) in float32
    max_abs_err: float     # float32 max over the good rows of |e|


@dataclasses.dataclass(frozen=True)
class TableAudit:
    """fcp_table_audit_t on the host.  ``kinds`` maps "f32" | "bf16" | "f16" | "q8" to its ``KindAudit``; ``raw`` is the C
    struct (what ``choose_dtypes`` hands to the library)."""
    rows: int
    dim: int
    rows_nonfinite: int
    first_nonfinite_row: int
    sum_sq: float
    kinds: Dict[str, KindAudit]
    raw: "_lib.TableAudit" = dataclasses.field(repr=False, compare=False, default=None)

    def admissible(self, dtype: str) -> bool:
        """Whether ``convert(table, dtype)`` holds every row of the table."""
        return dtype == "f32" or (self.rows_nonfinite == 0 and self.kinds[dtype].rows_bad == 0)


def _audit_of(raw: "_lib.TableAudit", dim: int) -> TableAudit:
    kinds = {name: KindAudit(int(raw.kind[k].rows_bad), int(raw.kind[k].first_bad_row), float(raw.kind[k].sum_sq_err),
                             float(raw.kind[k].max_abs_err)) for name, k in _lib.TABLE_KINDS.items()}
    return TableAudit(int(raw.rows), int(dim), int(raw.rows_nonfinite), int(raw.first_nonfinite_row), float(raw.sum_sq), kinds, raw)


def _counts_dtypes(torch):
    """the dtypes a count tensor may have: uint32 where the installed torch has it, and int32, whose bits are read as uint32"""
    return tuple(d for d in (getattr(torch, "uint32", None), torch.int32) if d is not None)


def _check_counts(torch, counts, what: str) -> int:
    if counts.dtype not in _counts_dtypes(torch) or counts.dim() != 1 or not counts.is_contiguous():
        raise ValueError(f"{what} is a contiguous 1-D uint32 tensor (or int32, its bits read as uint32): tables.new_counts")
    return int(counts.shape[0])


def new_counts(rows: int, device):
    """A zeroed read-count tensor of ``rows`` cells on ``device`` for ``count_ids`` and ``audit(..., row_counts=)``: uint32
    where the installed torch has that dtype, else int32 whose bits are read as uint32 (both are accepted wherever counts are)."""
    import torch
    return torch.zeros((int(rows),), dtype=_counts_dtypes(torch)[0], device=device)


def new_plan_counts(plan_or_spec, device) -> list:
    """One zeroed ``new_counts`` per device input of a plan (an ``ops.Plan``, an op that holds one, or a ``PlanSpec``) — as many
    cells as the unsharded table has rows, the largest ``vocab`` of the lookup columns that read the input — and ``None`` for
    the inputs no lookup column reads: what ``Plan.traffic_bind`` takes, and, once ``Plan.traffic_count`` has filled it, what
    ``audit_tables(spec, tables, row_counts=...)`` takes."""
    if hasattr(plan_or_spec, "table_rows"):
        rows = plan_or_spec.table_rows()
    else:
        rows = [-1] * plan_or_spec.n_device_inputs
        for c in plan_or_spec.columns:
            if c.form in _FORMS_WITH_TABLES:
                rows[c.table_input] = max(rows[c.table_input], int(c.vocab))
    return [None if r < 0 else new_counts(r, device) for r in rows]


def count_ids(counts, ids, skipped=None, stream: Optional[int] = None):
    """``fcp_table_count_ids``: add to ``counts[r]`` (``new_counts``; its length is the table's rows) the number of times ``r``
    occurs in ``ids`` — an int32 or int64 device tensor of any shape, contiguous: the id input of a sampled request as
    delivered.  Modulo 2^32.  Ids outside the table touch nothing; ``skipped``, an int64 device tensor of one element, is
    increased by their number (the caller zeroes it).  Asynchronous on ``stream`` (torch's current stream of the device by
    default).  Returns ``counts``."""
    import torch
    rows = _check_counts(torch, counts, "counts")
    if not counts.is_cuda:
        raise ValueError(f"counts: fcp_table_count_ids works on the device; the tensor is on {counts.device}")
    if ids.dtype not in (torch.int32, torch.int64) or not ids.is_contiguous():
        raise ValueError("ids is a contiguous int32 or int64 tensor")
    if ids.device != counts.device:
        raise ValueError(f"counts is on {counts.device}, ids on {ids.device}")
    if skipped is not None:
        if skipped.dtype != torch.int64 or skipped.numel() != 1 or skipped.device != counts.device:
            raise ValueError("skipped is an int64 tensor of one element on the counts' device")
    if stream is None:
        stream = torch.cuda.current_stream(counts.device).cuda_stream
    status = _lib.load().fcp_table_count_ids(C.c_void_p(counts.data_ptr()), rows, C.c_void_p(ids.data_ptr()), int(ids.element_size()),
                                             int(ids.numel()), C.c_void_p(skipped.data_ptr()) if skipped is not None else None,
                                             counts.device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_table_count_ids")
    return counts


def audit(table_or_rows, row_counts=None, stream: Optional[int] = None) -> TableAudit:
    """``fcp_table_audit``: what bf16, fp16 and q8 would do to the float32 ``[rows, dim]`` device tensor — a table before
    ``convert``, or the rows of a delta before ``update_rows`` — judged in one pass on the device.  ``row_counts`` (what
    ``count_ids`` filled: one cell per row, on the table's device) makes it ``fcp_table_audit_weighted``: ``sum_sq`` and every
    ``sum_sq_err`` weigh a row by its count; the fields that decide admissibility stay unweighted.  Allocates the result and
    the workspace, runs on ``stream`` (torch's current stream of the device by default), synchronises it, and returns the
    host ``TableAudit``."""
    import torch
    t = table_or_rows
    if row_counts is not None:          # (first: what can be seen of the pair wherever the two tensors live)
        if _check_counts(torch, row_counts, "row_counts") != t.shape[0]:
            raise ValueError(f"row_counts has {row_counts.shape[0]} cells, the table {t.shape[0]} rows")
        if row_counts.device != t.device:
            raise ValueError(f"the table is on {t.device}, row_counts on {row_counts.device}")
    name, dim = _kind_and_dim(t, "table_or_rows")
    if name != "f32":
        raise ValueError(f"audit takes a float32 table; this one is {name}")
    L = _lib.load()
    words = (C.sizeof(_lib.TableAudit) + 7) // 8
    if stream is None:
        stream = torch.cuda.current_stream(t.device).cuda_stream
    # allocated as that stream's: a block the caching allocator hands out may still have work pending on the stream it was freed on
    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=t.device)):
        out = torch.empty((words,), dtype=torch.int64, device=t.device)
        workspace = torch.empty((int(L.fcp_table_audit_workspace_bytes()) // 8,), dtype=torch.int64, device=t.device)
    if row_counts is None:
        status = L.fcp_table_audit(C.c_void_p(t.data_ptr()), int(t.shape[0]), dim, C.c_void_p(out.data_ptr()),
                                   C.c_void_p(workspace.data_ptr()), t.device.index or 0, C.c_void_p(stream))
        _lib.check(status, "fcp_table_audit")
    else:
        status = L.fcp_table_audit_weighted(C.c_void_p(t.data_ptr()), int(t.shape[0]), dim, C.c_void_p(row_counts.data_ptr()),
                                            C.c_void_p(out.data_ptr()), C.c_void_p(workspace.data_ptr()), t.device.index or 0,
                                            C.c_void_p(stream))
        _lib.check(status, "fcp_table_audit_weighted")
    torch.cuda.ExternalStream(stream, device=t.device).synchronize()
    raw = _lib.TableAudit.from_buffer_copy(out.cpu().numpy().tobytes()[:C.sizeof(_lib.TableAudit)])
    return _audit_of(raw, dim)


def audit_tables(spec: PlanSpec, tables: Sequence, row_counts: Optional[Sequence] = None, stream: Optional[int] = None) -> list:
    """One ``TableAudit`` per device input of ``spec``: every table a lookup column reads (a shared table once), ``None`` for
    the inputs no column reads as a table.  The tables are float32.  ``row_counts``: one entry per device input, a count
    tensor (the table's audit is the weighted one) or ``None`` (unweighted)."""
    if row_counts is not None and len(row_counts) != len(tables):
        raise ValueError(f"row_counts names {len(row_counts)} inputs, tables {len(tables)}")
    read = set(spec.read_inputs())
    return [audit(t, row_counts=None if row_counts is None else row_counts[i], stream=stream) if i in read else None
            for i, t in enumerate(tables)]


def choose_dtypes(spec: PlanSpec, audits: Sequence, budget_bytes: int, allowed: Sequence[str] = ("f32", "bf16", "f16", "q8"),
                  weights: Optional[Sequence[float]] = None):
    """``fcp_table_formats_choose`` over the tables ``spec`` reads: the formats that minimise the weighted squared error
    within ``budget_bytes`` of tables.  ``audits``: what ``audit_tables`` returned (one entry per device input).  ``weights``:
    one per device input (entries of unread inputs ignored), default 1 / sum of squares of the table.  Returns
    ``(dtypes, bytes, error)``: the tuple ``PlanSpec.with_table_dtypes`` takes — "-" for inputs no column reads —, the bytes
    of the chosen tables and their weighted error.  A budget even the smallest admissible assignment exceeds raises
    ``FcpError`` (FCP_ERR_UNSUPPORTED) naming the bytes needed."""
    read = spec.read_inputs()
    if len(audits) != spec.n_device_inputs:
        raise ValueError(f"audits names {len(audits)} inputs, the plan has {spec.n_device_inputs} device inputs")
    mask = 0
    for name in allowed:
        if name not in _lib.TABLE_KINDS:
            raise ValueError(f"unknown table dtype {name!r}")
        mask |= 1 << _lib.TABLE_KINDS[name]
    for t in read:
        if audits[t] is None:
            raise ValueError(f"device input {t} is read as a table and has no audit")
    n = len(read)
    raw = (_lib.TableAudit * max(n, 1))(*[audits[t].raw for t in read])
    rows = (C.c_int64 * max(n, 1))(*[audits[t].rows for t in read])
    dims = (C.c_int32 * max(n, 1))(*[audits[t].dim for t in read])
    w = None if weights is None else (C.c_double * max(n, 1))(*[float(weights[t]) for t in read])
    kinds = (C.c_int32 * max(n, 1))()
    nbytes, error = C.c_int64(0), C.c_double(0.0)
    status = _lib.load().fcp_table_formats_choose(raw, rows, dims, n, int(budget_bytes), mask, w, kinds, C.byref(nbytes), C.byref(error))
    _lib.check(status, "fcp_table_formats_choose")
    names = ["-"] * spec.n_device_inputs
    for i, t in enumerate(read):
        names[t] = _lib.ALL_TABLE_DTYPES[kinds[i]]
    return tuple(names), int(nbytes.value), float(error.value)


# ---- digest (fcp_table_digest / fcp_table_digest_rows / fcp_table_digest_host) -------------------------------------------------
def _digest_buffers(torch, L, device, stream: int, n_out: int = 1):
    """``n_out`` result records and one workspace (calls on one stream run one after the other and may share it), allocated as
    that stream's (``_as_streams`` says why)"""
    return _as_streams(torch, device, stream, (n_out, C.sizeof(_lib.TableDigest) // 8), (int(L.fcp_table_digest_workspace_bytes()) // 8,))


def _digests_of(outs) -> list:
    size = C.sizeof(_lib.TableDigest)
    raw = outs.cpu().numpy().tobytes()
    return [_lib.TableDigest.from_buffer_copy(raw[k * size:(k + 1) * size]) for k in range(outs.shape[0])]


def _enqueue_digest_rows(L, table, name: str, dim: int, row_ids, n: int, row0: int, row_step: int, out_ptr: int, workspace, stream: int):
    status = L.fcp_table_digest_rows(C.c_void_p(table.data_ptr()), _lib.TABLE_KINDS[name], int(table.shape[0]), dim, int(row0),
                                     int(row_step), C.c_void_p(row_ids.data_ptr()), n, C.c_void_p(out_ptr),
                                     C.c_void_p(workspace.data_ptr()), table.device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_table_digest_rows")


def digest(table, row0: int = 0, row_step: int = 1, stream: Optional[int] = None) -> int:
    """``fcp_table_digest``: the order-free 64-bit sum of row hashes of ``table`` — a device tensor in one of the four table
    formats, or a row range of one (``table[a:b]``, with ``row0=a``): local row ``i`` has the global index
    ``row0 + i * row_step``.  Chunks add up to the whole table, and the shards of a table row-sharded ``id % world`` — rank
    ``g`` passes ``row0=g, row_step=world`` — add up to the unsharded table, both modulo 2^64.  Detects accidents; not a MAC.
    Allocates the result and the workspace, runs on ``stream`` (torch's current stream of the device by default), synchronises
    it, and returns the sum."""
    import torch
    name, dim = _kind_and_dim(table, "table")
    L = _lib.load()
    if stream is None:
        stream = torch.cuda.current_stream(table.device).cuda_stream
    outs, workspace = _digest_buffers(torch, L, table.device, stream)
    status = L.fcp_table_digest(C.c_void_p(table.data_ptr()), _lib.TABLE_KINDS[name], int(table.shape[0]), dim, int(row0), int(row_step),
                                C.c_void_p(outs.data_ptr()), C.c_void_p(workspace.data_ptr()), table.device.index or 0,
                                C.c_void_p(stream))
    _lib.check(status, "fcp_table_digest")
    torch.cuda.ExternalStream(stream, device=table.device).synchronize()
    return int(_digests_of(outs)[0].sum)


def digest_rows(table, row_ids, row0: int = 0, row_step: int = 1, stream: Optional[int] = None):
    """``fcp_table_digest_rows``: the same sum over the rows ``row_ids`` (int64 ``[n]`` on the table's device) names of the WHOLE
    table ``table``: an id inside the table adds the hash of that row at global index ``row0 + id * row_step``, as often as it
    occurs; any other id adds nothing.  Synchronises ``stream`` and returns ``(sum, rows, skipped)``."""
    import torch
    name, dim = _kind_and_dim(table, "table")
    n = _ids_of(torch, table, row_ids)
    L = _lib.load()
    if stream is None:
        stream = torch.cuda.current_stream(table.device).cuda_stream
    outs, workspace = _digest_buffers(torch, L, table.device, stream)
    _enqueue_digest_rows(L, table, name, dim, row_ids, n, row0, row_step, outs.data_ptr(), workspace, stream)
    torch.cuda.ExternalStream(stream, device=table.device).synchronize()
    d = _digests_of(outs)[0]
    return int(d.sum), int(d.rows), int(d.skipped)


def digest_host(array, dtype: str, dim: Optional[int] = None, row0: int = 0, row_step: int = 1) -> int:
    """``fcp_table_digest_host``: the digest of table rows in HOST memory — a NumPy array or a torch CPU tensor that holds rows
    of a ``dtype`` ("f32" | "bf16" | "f16" | "q8") table back to back; its own element type plays no part, only its bytes do
    (NumPy has no bfloat16: hand over uint16 or uint8).  ``dim``: the table's width; by default that of a 2-D array whose
    rows are the table's.  No device is touched."""
    import numpy as np
    if dtype not in _lib.TABLE_KINDS:
        raise ValueError(f"unknown table dtype {dtype!r}")
    if hasattr(array, "is_cuda"):
        import torch
        if array.is_cuda:
            raise ValueError("digest_host takes host memory; tables.digest works on the device")
        shape, item = tuple(array.shape), array.element_size()
        array = array.contiguous().reshape(-1).view(torch.uint8).numpy()        # (bytes: NumPy has no bfloat16)
        if len(shape) == 2:
            array = array.reshape(shape[0], shape[1] * item)
    else:
        array = np.ascontiguousarray(array)
    fmt = TABLE_FORMATS[dtype]
    if dim is None:
        if array.ndim != 2:
            raise ValueError("digest_host needs dim= for anything but a 2-D array whose rows are the table's")
        dim, odd = divmod(array.shape[1] * array.itemsize - fmt.row_tail, fmt.elem)
        if odd or dim <= 0:
            raise ValueError(f"rows of {array.shape[1] * array.itemsize} bytes are no rows of a {dtype} table")
    if dim <= 0:
        raise ValueError("dim must be positive")
    rb = fmt.row_bytes(int(dim))
    if array.nbytes % rb:
        raise ValueError(f"{array.nbytes} bytes are no whole number of {dtype} rows of dim {dim} ({rb} bytes each)")
    if row0 < 0 or row_step < 1:
        raise ValueError("row0 must not be negative and row_step must be at least 1")
    raw = array.reshape(-1).view(np.uint8)
    return int(_lib.load().fcp_table_digest_host(C.c_void_p(raw.ctypes.data), _lib.TABLE_KINDS[dtype], raw.size // rb, int(dim),
                                                 int(row0), int(row_step)))


def digest_tables(spec: PlanSpec, tables: Sequence, stream: Optional[int] = None) -> list:
    """One ``digest`` per device input of ``spec`` that a lookup column reads (a shared table once), ``None`` for the others.
    The tables are the rank's own — any format — and ``row0 = spec.shard_rank, row_step = spec.shard_world``: the lists of the
    ranks of a row-sharded plan add up, entry by entry modulo 2^64, to the unsharded plan's.  One ``fcp_tables_digest`` call
    and one synchronise for the whole plan (``digests_grouped``)."""
    read = [i for i in sorted(set(spec.read_inputs())) if i < len(tables)]
    sums = digests_grouped([tables[i] for i in read], row0=spec.shard_rank, row_step=spec.shard_world, stream=stream)
    out = [None] * len(tables)
    for i, s in zip(read, sums):
        out[i] = s
    return out


# ---- digest, many tables in one call (fcp_tables_digest) --------------------------------------------------------------------------
def _per_table(value, n: int, what: str) -> list:
    """``value`` for each of n entries: a scalar for all of them, or a sequence of n"""
    if hasattr(value, "__len__"):
        if len(value) != n:
            raise ValueError(f"tables names {n} entries, {what} {len(value)}")
        return [int(v) for v in value]
    return [int(value)] * n


def _digest_entries(torch, tables_, row_ids, row0, row_step):
    """The ``fcp_table_digest_entry_t`` array of ``tables_`` — with ``row_ids`` (a sequence as long) the by-id entries, without
    the rows of each table back to back — each entry validated as ``digest`` / ``digest_rows`` validate theirs, and the one
    device all of it lives on (``None`` for no entries)."""
    n_tables = len(tables_)
    if row_ids is not None and len(row_ids) != n_tables:
        raise ValueError(f"tables names {n_tables} entries, row_ids {len(row_ids)}")
    row0s, steps = _per_table(row0, n_tables, "row0"), _per_table(row_step, n_tables, "row_step")

    def entry_of(k, t):
        name, dim = _kind_and_dim(t, "table")
        n = _ids_of(torch, t, row_ids[k]) if row_ids is not None else 0
        # (an empty id tensor may have no address: the entry then reads as "no rows back to back", which sums the same nothing)
        ids_ptr = row_ids[k].data_ptr() if n else None
        return t.data_ptr(), ids_ptr, int(t.shape[0]) if n or row_ids is None else 0, n, row0s[k], steps[k], _lib.TABLE_KINDS[name], dim, 0
    return _entries_of(_lib.TableDigestEntry, tables_, entry_of)


def _grouped_digest_buffers(torch, L, device, stream: int, n_tables: int, n_out: int = 1):
    """``n_out`` result arrays of ``n_tables`` records and one workspace (calls on one stream run one after the other and may
    share it), allocated as that stream's"""
    return _as_streams(torch, device, stream, (n_out, n_tables, C.sizeof(_lib.TableDigest) // 8),
                       (int(L.fcp_tables_digest_workspace_bytes(n_tables)) // 8,))


def _enqueue_digests(L, entries, n_tables: int, out, workspace, device, stream: int) -> None:
    status = L.fcp_tables_digest(entries, n_tables, C.c_void_p(out.data_ptr()), C.c_void_p(workspace.data_ptr()), device.index or 0,
                                 C.c_void_p(stream))
    _lib.check(status, "fcp_tables_digest")


def _grouped_digests(tables_, row_ids, row0, row_step, stream: Optional[int]) -> list:
    """the ``TableDigest`` records of one ``fcp_tables_digest`` call, read after one synchronise"""
    import torch
    entries, device = _digest_entries(torch, tables_, row_ids, row0, row_step)
    if device is None:
        return []
    L = _lib.load()
    stream = _stream_of(torch, device, stream)
    outs, workspace = _grouped_digest_buffers(torch, L, device, stream, len(tables_))
    _enqueue_digests(L, entries, len(tables_), outs[0], workspace, device, stream)
    torch.cuda.ExternalStream(stream, device=device).synchronize()
    return _digests_of(outs[0])


def digests_grouped(tables, row0=0, row_step=1, stream: Optional[int] = None) -> list:
    """``fcp_tables_digest``: ``digest`` of many tables in ONE call and one synchronise — entry k is what
    ``digest(tables[k], row0[k], row_step[k])`` returns, in any mix of formats and dims on one device; the number of launches
    does not grow with their number.  ``row0`` / ``row_step``: a scalar for every table, or one value per table.  Tables may
    be row ranges ``t[a:b]`` (with ``row0=a``) and may name the same memory more than once."""
    return [int(d.sum) for d in _grouped_digests(tables, None, row0, row_step, stream)]


def digest_rows_grouped(tables, row_ids, row0=0, row_step=1, stream: Optional[int] = None) -> list:
    """``fcp_tables_digest`` by id: ``digest_rows`` of many tables in ONE call and one synchronise — entry k is the
    ``(sum, rows, skipped)`` that ``digest_rows(tables[k], row_ids[k], row0[k], row_step[k])`` returns."""
    if row_ids is None:
        raise ValueError("row_ids is a sequence of int64 [n] tensors, one per table")
    return [(int(d.sum), int(d.rows), int(d.skipped)) for d in _grouped_digests(tables, row_ids, row0, row_step, stream)]


def update_rows_grouped_tracked(tables, row_ids, rows, digests, row0=0, row_step=1, skipped=None, stream: Optional[int] = None) -> list:
    """``update_rows_grouped`` with every table's digest kept up to date from the touched rows alone: one grouped digest of
    ``row_ids`` before, the grouped update, one grouped digest after — all on ``stream``, one synchronise at the end — and
    ``(digests[k] - before[k] + after[k]) mod 2^64`` is returned per table: the ``digest`` of the updated table when
    ``digests[k]`` was that of the table before and its ids are pairwise distinct (not checked)."""
    import torch
    if len(digests) != len(tables):
        raise ValueError(f"tables names {len(tables)} entries, digests {len(digests)}")
    entries, device = _digest_entries(torch, tables, row_ids, row0, row_step)
    if device is None:
        update_rows_grouped(tables, row_ids, rows, skipped=skipped, stream=stream)
        return []
    L = _lib.load()
    n_tables = len(tables)
    stream = _stream_of(torch, device, stream)
    outs, workspace = _grouped_digest_buffers(torch, L, device, stream, n_tables, n_out=2)
    _enqueue_digests(L, entries, n_tables, outs[0], workspace, device, stream)
    update_rows_grouped(tables, row_ids, rows, skipped=skipped, stream=stream)
    _enqueue_digests(L, entries, n_tables, outs[1], workspace, device, stream)
    torch.cuda.ExternalStream(stream, device=device).synchronize()
    before, after = _digests_of(outs[0]), _digests_of(outs[1])
    return [(int(d) - int(b.sum) + int(a.sum)) % (1 << 64) for d, b, a in zip(digests, before, after)]


def update_rows_tracked(table, row_ids, rows, digest: int, row0: int = 0, row_step: int = 1, skipped=None,
                        stream: Optional[int] = None) -> int:
    """``update_rows`` with the table's digest kept up to date from the touched rows alone: ``digest_rows`` of ``row_ids``
    before, the update, ``digest_rows`` after — all on ``stream``, one synchronise at the end — and
    ``(digest - before + after) mod 2^64`` is returned: the ``digest`` of the updated table when ``digest`` was that of the
    table before and the ids are pairwise distinct (``update_rows`` asks the same; not checked)."""
    import torch
    name, dim = _kind_and_dim(table, "table")
    n = _ids_of(torch, table, row_ids)
    L = _lib.load()
    if stream is None:
        stream = torch.cuda.current_stream(table.device).cuda_stream
    outs, workspace = _digest_buffers(torch, L, table.device, stream, n_out=2)
    size = C.sizeof(_lib.TableDigest)
    _enqueue_digest_rows(L, table, name, dim, row_ids, n, row0, row_step, outs.data_ptr(), workspace, stream)
    update_rows(table, row_ids, rows, skipped=skipped, stream=stream)
    _enqueue_digest_rows(L, table, name, dim, row_ids, n, row0, row_step, outs.data_ptr() + size, workspace, stream)
    torch.cuda.ExternalStream(stream, device=table.device).synchronize()
    before, after = _digests_of(outs)
    return (int(digest) - int(before.sum) + int(after.sum)) % (1 << 64)


# ---- a delta's ids made distinct (fcp_table_delta_distinct) ---------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class DeltaReport:
    """fcp_table_delta_report_t on the host; ``n == distinct + duplicates + skipped``."""
    n: int             # ids handed over
    distinct: int      # rows kept: one per distinct id inside the table
    duplicates: int    # occurrences dropped because a later position names the same row
    skipped: int       # ids outside [0, table_rows)


def _report_of(cls, report_t):          # cls: DeltaReport | DiffReport, the dataclass of the int64 device tensor report_t
    return cls(*(int(v) for v in report_t.cpu().tolist()))


def _stream_of(torch, device, stream: Optional[int]) -> int:
    return torch.cuda.current_stream(device).cuda_stream if stream is None else stream


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _selection_outputs(torch, device, stream: int, n: int, dim: Optional[int], pos: bool, report_t, need: int):
    """``(ids, pos, rows, report, workspace)`` of a selecting entry as that stream's; ``pos`` / ``rows`` ``None`` unless asked for"""
    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device)):
        ids_out = torch.empty((n,), dtype=torch.int64, device=device)
        pos_out = torch.empty((n,), dtype=torch.int64, device=device) if pos else None
        rows_out = torch.empty((n, dim), dtype=torch.float32, device=device) if dim is not None else None
        report = torch.empty((C.sizeof(report_t) // 8,), dtype=torch.int64, device=device)
        workspace = torch.empty((need // 8,), dtype=torch.int64, device=device)
    return ids_out, pos_out, rows_out, report, workspace


def _delta_ids_of(torch, row_ids) -> int:
    if row_ids.dtype not in (torch.int32, torch.int64) or row_ids.dim() != 1 or not row_ids.is_contiguous():
        raise ValueError("row_ids is a contiguous int64 or int32 [n] tensor")
    if not row_ids.is_cuda:
        raise ValueError(f"row_ids: fcp_table_delta_distinct works device to device; the tensor is on {row_ids.device}")
    return int(row_ids.shape[0])


def delta_distinct_async(row_ids, rows=None, table_rows: Optional[int] = None, pos: bool = False, stream: Optional[int] = None):
    """``fcp_table_delta_distinct`` enqueued on ``stream`` (torch's current stream of the device by default), nothing
    synchronised: returns ``(ids, rows, report)`` — plus ``pos`` when asked — at their full length ``n``: the winners in front,
    in ascending position, ``-1`` behind them in ``ids`` and ``pos``, rows behind them uninitialised; ``report`` is the int64
    ``[4]`` device tensor ``(n, distinct, duplicates, skipped)``.  The padded ``(ids, rows)`` go straight into ``update_rows`` /
    ``digest_rows`` on the same stream, which skip ``-1``.  Outputs and workspace are allocated as that stream's."""
    import torch
    n = _delta_ids_of(torch, row_ids)
    if table_rows is None:
        raise ValueError("table_rows= is needed: the rows of the table the delta is for")
    dim = 0
    if rows is not None:
        if rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous():
            raise ValueError("rows is a contiguous float32 [n, dim] tensor")
        if rows.device != row_ids.device:
            raise ValueError(f"row_ids is on {row_ids.device}, rows on {rows.device}")
        if rows.shape[0] != n:
            raise ValueError(f"rows has {rows.shape[0]} rows, row_ids names {n}")
        dim = int(rows.shape[1])
    L = _lib.load()
    device = row_ids.device
    need = int(L.fcp_table_delta_workspace_bytes(n))
    if need < 0:
        raise ValueError(f"row_ids names {n} ids; a delta stays below 2^32 - 3")
    stream = _stream_of(torch, device, stream)
    ids_out, pos_out, rows_out, report, workspace = _selection_outputs(torch, device, stream, n, dim if rows is not None else None, pos,
                                                                       _lib.TableDeltaReport, need)
    status = L.fcp_table_delta_distinct(_ptr(row_ids), int(row_ids.element_size()), _ptr(rows), dim, n, int(table_rows), _ptr(ids_out),
                                        _ptr(rows_out), _ptr(pos_out), _ptr(report), _ptr(workspace), device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_table_delta_distinct")
    return (ids_out, rows_out, report, pos_out) if pos else (ids_out, rows_out, report)


def delta_distinct(row_ids, rows=None, table_rows: Optional[int] = None, pos: bool = False, stream: Optional[int] = None):
    """``fcp_table_delta_distinct``: the delta ``(row_ids, rows)`` — int64 or int32 ids ``[n]`` and float32 rows ``[n, dim]`` on
    the device, or ids alone — with every id inside ``[0, table_rows)`` kept ONCE, at its LAST position, the kept positions in
    ascending order; rows are copied as bits.  Runs on ``stream`` (torch's current stream of the device by default),
    synchronises it, and returns ``(ids[:m], rows[:m] or None, report)`` — plus ``pos[:m]``, the kept positions, when ``pos`` —
    with ``report`` a ``DeltaReport``.  ``report.duplicates == 0`` and ``report.skipped == 0`` say the delta was distinct and
    inside the table as it stood: it comes back byte for byte."""
    import torch
    out = delta_distinct_async(row_ids, rows, table_rows=table_rows, pos=pos, stream=stream)
    torch.cuda.ExternalStream(_stream_of(torch, row_ids.device, stream), device=row_ids.device).synchronize()
    report = _report_of(DeltaReport, out[2])
    m = report.distinct
    head = (out[0][:m], out[1][:m] if out[1] is not None else None, report)
    return head + (out[3][:m],) if pos else head


def apply_delta(table, row_ids, rows, digest: Optional[int] = None, row0: int = 0, row_step: int = 1, skipped=None,
                stream: Optional[int] = None):
    """``update_rows`` for a delta whose ids may REPEAT, in every table format: ``delta_distinct_async``, then ``update_rows`` of
    the padded outputs — the table ends up, byte for byte, as if the rows had been written one after the other in position
    order.  With ``digest`` (that of the table before; ``row0`` / ``row_step`` as in ``digest``) the ``digest_rows`` bookkeeping
    of ``update_rows_tracked`` runs around the update.  ``skipped``, an int64 device tensor of one element, is increased by the
    delta's own ids outside the table (not by the ``-1`` padding).  All on ``stream``, one synchronise at the end.  Returns the
    ``DeltaReport``, or ``(report, new digest)`` when ``digest`` was given."""
    import torch
    name, dim = _kind_and_dim(table, "table")
    n = _delta_ids_of(torch, row_ids)
    if row_ids.device != table.device:
        raise ValueError(f"table is on {table.device}, row_ids on {row_ids.device}")
    _rows_of(torch, table, dim, n, rows, "rows")
    if skipped is not None:
        if skipped.dtype != torch.int64 or skipped.numel() != 1 or skipped.device != table.device:
            raise ValueError("skipped is an int64 tensor of one element on the table's device")
    L = _lib.load()
    stream = _stream_of(torch, table.device, stream)
    ids_d, rows_d, report_t = delta_distinct_async(row_ids, rows, table_rows=int(table.shape[0]), stream=stream)
    if digest is not None:
        outs, workspace = _digest_buffers(torch, L, table.device, stream, n_out=2)
        size = C.sizeof(_lib.TableDigest)
        _enqueue_digest_rows(L, table, name, dim, ids_d, n, row0, row_step, outs.data_ptr(), workspace, stream)
    update_rows(table, ids_d, rows_d, stream=stream)      # (its own skipped counter would count the padding too)
    if digest is not None:
        _enqueue_digest_rows(L, table, name, dim, ids_d, n, row0, row_step, outs.data_ptr() + size, workspace, stream)
    ext = torch.cuda.ExternalStream(stream, device=table.device)
    if skipped is not None:
        with torch.cuda.stream(ext):
            skipped.view(-1).add_(report_t[3:4])
    ext.synchronize()
    report = _report_of(DeltaReport, report_t)
    if digest is None:
        return report
    before, after = _digests_of(outs)
    return report, (int(digest) - int(before.sum) + int(after.sum)) % (1 << 64)


# ---- a model's delta made distinct, many tables in one call (fcp_tables_delta_distinct) -----------------------------------------
def _delta_entries(torch, row_ids, rows, table_rows, pos: bool, stream: Optional[int]):
    """What one ``fcp_tables_delta_distinct`` call takes: every entry validated as ``delta_distinct_async`` validates its own,
    the outputs carved out of ONE tensor per kind (int64 ids, int64 positions, float32 rows, each entry's rows at a 16-byte
    boundary, int64 reports) and the workspace, all allocated as that stream's.  Returns ``(entries, device, stream, ids_out,
    rows_out, pos_out, reports, workspace)`` — the per-entry outputs as lists of views — or ``device`` ``None`` without entries."""
    n_tables = len(row_ids)
    if rows is not None and len(rows) != n_tables:
        raise ValueError(f"row_ids names {n_tables} entries, rows {len(rows)}")
    if not hasattr(table_rows, "__len__") or len(table_rows) != n_tables:
        raise ValueError(f"row_ids names {n_tables} entries; table_rows is a sequence as long: the rows of each entry's table")
    if n_tables == 0:
        return None, None, stream, [], [], [], None, None
    device = None
    ns, dims = [], []
    for k in range(n_tables):
        try:
            n = _delta_ids_of(torch, row_ids[k])
            if device is None:
                device = row_ids[k].device
            elif row_ids[k].device != device:
                raise ValueError(f"row_ids is on {row_ids[k].device}, entry 0's on {device}")
            dim = None
            if rows is not None and rows[k] is not None:
                r = rows[k]
                if r.dtype != torch.float32 or r.dim() != 2 or not r.is_contiguous():
                    raise ValueError("rows is a contiguous float32 [n, dim] tensor")
                if r.device != device:
                    raise ValueError(f"row_ids is on {device}, rows on {r.device}")
                if r.shape[0] != n:
                    raise ValueError(f"rows has {r.shape[0]} rows, row_ids names {n}")
                dim = int(r.shape[1])
        except ValueError as e:
            raise ValueError(f"entry {k}: {e}") from None
        ns.append(n)
        dims.append(dim)
    L = _lib.load()
    need = int(L.fcp_tables_delta_workspace_bytes((C.c_int64 * n_tables)(*ns), n_tables))
    if need < 0:
        raise ValueError(f"row_ids names {n_tables} entries of {sum(ns)} ids together; a call takes at most 65536 entries and stays below 2^32 - 3 ids")
    stream = _stream_of(torch, device, stream)
    row_at, floats = [], 0
    for n, dim in zip(ns, dims):
        row_at.append(floats)
        floats += (n * (dim or 0) + 3) // 4 * 4
    total = sum(ns)
    with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device)):
        ids_all = torch.empty((total,), dtype=torch.int64, device=device)
        pos_all = torch.empty((total,), dtype=torch.int64, device=device) if pos else None
        rows_all = torch.empty((floats,), dtype=torch.float32, device=device)
        reports = torch.empty((n_tables, C.sizeof(_lib.TableDeltaReport) // 8), dtype=torch.int64, device=device)
        workspace = torch.empty((need // 8,), dtype=torch.int64, device=device)
    entries = (_lib.TableDeltaEntry * n_tables)()
    ids_out, rows_out, pos_out = [], [], []
    at = 0
    for k, (n, dim) in enumerate(zip(ns, dims)):
        ids_out.append(ids_all[at:at + n])
        pos_out.append(pos_all[at:at + n] if pos else None)
        rows_out.append(rows_all[row_at[k]:row_at[k] + n * dim].view(n, dim) if dim is not None else None)
        # (an empty tensor may have no address; the entry reads none of its pointers at n == 0)
        with_rows = dim is not None and n > 0
        entries[k] = _lib.TableDeltaEntry(row_ids[k].data_ptr() if n else None, rows[k].data_ptr() if with_rows else None,
                                          ids_out[k].data_ptr() if n else None, rows_out[k].data_ptr() if with_rows else None,
                                          pos_out[k].data_ptr() if pos and n else None, int(table_rows[k]), n,
                                          int(row_ids[k].element_size()), dim or 0)
        at += n
    return entries, device, stream, ids_out, rows_out, pos_out, reports, workspace


def delta_distinct_grouped_async(row_ids, rows, table_rows, pos: bool = False, stream: Optional[int] = None):
    """``fcp_tables_delta_distinct`` enqueued on ``stream`` (torch's current stream of the device by default), nothing
    synchronised: ``delta_distinct_async`` for a whole model's delta in ONE call.  ``row_ids`` and ``table_rows`` are equally
    long sequences, ``rows`` a sequence as long (an entry ``None``: ids only) or ``None`` for ids only throughout; entry k is
    what ``delta_distinct_async(row_ids[k], rows[k], table_rows=table_rows[k])`` takes, int32 and int64 ids and any dims mixed,
    on one device; the number of launches does not grow with their number.  Returns one tuple per entry, ``(ids, rows,
    report)`` — plus ``pos`` when asked — byte for byte what the single-table function leaves, each at its full length n_k.
    Entries are independent: an id that repeats ACROSS two entries is not seen."""
    import torch
    entries, device, stream, ids_out, rows_out, pos_out, reports, workspace = _delta_entries(torch, row_ids, rows, table_rows, pos, stream)
    if device is None:
        return []
    status = _lib.load().fcp_tables_delta_distinct(entries, len(row_ids), _ptr(reports), _ptr(workspace), device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_tables_delta_distinct")
    return [(ids_out[k], rows_out[k], reports[k], pos_out[k]) if pos else (ids_out[k], rows_out[k], reports[k]) for k in range(len(row_ids))]


def _reports_of(reports) -> list:
    return [DeltaReport(*(int(v) for v in r)) for r in reports.cpu().tolist()]


def delta_distinct_grouped(row_ids, rows, table_rows, pos: bool = False, stream: Optional[int] = None):
    """``fcp_tables_delta_distinct``: ``delta_distinct`` for a whole model's delta in ONE call and one synchronise — one tuple
    ``(ids[:m], rows[:m] or None, report)`` per entry, plus ``pos[:m]`` when ``pos``, with ``report`` a ``DeltaReport``."""
    import torch
    out = delta_distinct_grouped_async(row_ids, rows, table_rows, pos=pos, stream=stream)
    if not out:
        return []
    device = row_ids[0].device
    torch.cuda.ExternalStream(_stream_of(torch, device, stream), device=device).synchronize()
    reports = _reports_of(torch.stack([o[2] for o in out]))
    result = []
    for o, report in zip(out, reports):
        m = report.distinct
        head = (o[0][:m], o[1][:m] if o[1] is not None else None, report)
        result.append(head + (o[3][:m],) if pos else head)
    return result


def apply_delta_grouped(tables, row_ids, rows, digests=None, row0=0, row_step=1, skipped=None, stream: Optional[int] = None):
    """``apply_delta`` for a whole model in FOUR library calls: the grouped distinct, (``fcp_tables_digest`` of the winners'
    rows,) ``update_rows_grouped`` of the padded outputs, (the same digest again) — every table ends up, byte for byte, as one
    ``apply_delta`` per entry leaves it.  ``tables``, ``row_ids`` (int64) and ``rows`` are equally long sequences; ``digests``, if
    given, every table's digest before (``row0`` / ``row_step``: a scalar or one per table, as in ``digests_grouped``).
    ``skipped``: one int64 ``[len(tables)]`` device tensor; element k grows by entry k's own ids outside its table (not by the
    ``-1`` padding).  An id that repeats across two entries is not seen: entries that name one table are merged first.  All on
    ``stream``, one synchronise at the end.  Returns the list of ``DeltaReport``s, or ``(reports, new digests)``."""
    import torch
    n_tables = len(tables)
    if len(row_ids) != n_tables or len(rows) != n_tables:
        raise ValueError(f"tables names {n_tables} entries, row_ids {len(row_ids)}, rows {len(rows)}")
    if digests is not None and len(digests) != n_tables:
        raise ValueError(f"tables names {n_tables} entries, digests {len(digests)}")
    device = None
    for k, t in enumerate(tables):
        try:
            _name, dim = _kind_and_dim(t, "table")
            n = _delta_ids_of(torch, row_ids[k])
            if row_ids[k].device != t.device:
                raise ValueError(f"table is on {t.device}, row_ids on {row_ids[k].device}")
            _rows_of(torch, t, dim, n, rows[k], "rows")
            if device is None:
                device = t.device
            elif t.device != device:
                raise ValueError(f"table is on {t.device}, entry 0's on {device}")
        except ValueError as e:
            raise ValueError(f"entry {k}: {e}") from None
    if skipped is not None:
        if skipped.dtype != torch.int64 or skipped.dim() != 1 or skipped.shape[0] != n_tables or not skipped.is_contiguous() or \
                (device is not None and skipped.device != device):
            raise ValueError("skipped is a contiguous int64 [len(tables)] tensor on the tables' device")
    if device is None:
        return [] if digests is None else ([], [])
    L = _lib.load()
    stream = _stream_of(torch, device, stream)
    entries, _device, _stream, ids_d, rows_d, _pos, reports_t, workspace = _delta_entries(torch, row_ids, rows, [int(t.shape[0]) for t in tables],
                                                                                         False, stream)
    status = L.fcp_tables_delta_distinct(entries, n_tables, _ptr(reports_t), _ptr(workspace), device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_tables_delta_distinct")
    if digests is not None:
        d_entries, _d = _digest_entries(torch, tables, ids_d, row0, row_step)
        outs, d_workspace = _grouped_digest_buffers(torch, L, device, stream, n_tables, n_out=2)
        _enqueue_digests(L, d_entries, n_tables, outs[0], d_workspace, device, stream)
    update_rows_grouped(tables, ids_d, rows_d, stream=stream)      # (its own skipped counters would count the padding too)
    if digests is not None:
        _enqueue_digests(L, d_entries, n_tables, outs[1], d_workspace, device, stream)
    ext = torch.cuda.ExternalStream(stream, device=device)
    if skipped is not None:
        with torch.cuda.stream(ext):
            skipped.add_(reports_t[:, 3])
    ext.synchronize()
    reports = _reports_of(reports_t)
    if digests is None:
        return reports
    before, after = _digests_of(outs[0]), _digests_of(outs[1])
    return reports, [(int(d) - int(b.sum) + int(a.sum)) % (1 << 64) for d, b, a in zip(digests, before, after)]


# ---- a new master against a served table (fcp_table_diff) ----------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class DiffReport:
    """fcp_table_diff_report_t on the host."""
    rows: int            # rows compared
    changed: int         # rows whose stored bytes would change
    first_changed: int   # smallest changed table row index, -1 if none
    last_changed: int    # largest, -1 if none


def diff_async(table, src, row0: int = 0, want_rows: bool = True, stream: Optional[int] = None):
    """``fcp_table_diff`` enqueued on ``stream`` (torch's current stream of the device by default), nothing synchronised.
    ``table``: a device tensor in one of the four table formats; ``src``: the candidates for its rows ``row0 ..
    row0 + len(src) - 1`` — float32 ``[rows, dim]`` (a new master), or rows in the table's own format (a replica: ids only,
    ``want_rows=False``).  Returns ``(ids, rows, report)`` at their full length: the changed rows' table indices in front, in
    ascending order, ``-1`` behind them; the changed ``src`` rows behind one another, the rest uninitialised (``None`` without
    ``want_rows``); ``report`` the int64 ``[4]`` device tensor ``(rows, changed, first_changed, last_changed)``.  The padded
    ``(ids, rows)`` go straight into ``update_rows`` / ``digest_rows`` on the same stream, which skip ``-1``.  Outputs and
    workspace are allocated as that stream's."""
    import torch
    name, dim = _kind_and_dim(table, "table")
    src_name, src_dim = _kind_and_dim(src, "src")
    if src_name not in ("f32", name):
        raise ValueError(f"src is {src_name}; a {name} table is compared with a float32 master or a {name} replica")
    if src_dim != dim:
        raise ValueError(f"src has rows of dim {src_dim}; the table's are of dim {dim}")
    if src.device != table.device:
        raise ValueError(f"table is on {table.device}, src on {src.device}")
    rows = int(src.shape[0])
    if row0 < 0 or row0 + rows > table.shape[0]:
        raise ValueError(f"rows [{row0}, {row0 + rows}) do not lie in a table of {table.shape[0]} rows")
    if want_rows and src_name != "f32":
        raise ValueError(f"a {src_name} replica gives ids only: want_rows=False")
    L = _lib.load()
    device = table.device
    need = int(L.fcp_table_diff_workspace_bytes(rows))
    if need < 0:
        raise ValueError(f"src has {rows} rows; a call stays below 2^32 - 3")
    stream = _stream_of(torch, device, stream)
    ids_out, _pos, rows_out, report, workspace = _selection_outputs(torch, device, stream, rows, dim if want_rows else None, False,
                                                                    _lib.TableDiffReport, need)
    status = L.fcp_table_diff(_ptr(table), _lib.TABLE_KINDS[name], int(table.shape[0]), dim, _ptr(src), _lib.TABLE_KINDS[src_name], int(row0),
                              rows, _ptr(ids_out), _ptr(rows_out), _ptr(report), _ptr(workspace), device.index or 0, C.c_void_p(stream))
    _lib.check(status, "fcp_table_diff")
    return ids_out, rows_out, report


def diff(table, src, row0: int = 0, want_rows: bool = True, stream: Optional[int] = None):
    """``fcp_table_diff``: the rows of ``table`` whose stored bytes would change if ``src`` — a new float32 master, or a replica
    in the table's format — were converted over its rows ``row0`` and below: a row counts when the bytes ``convert`` writes for
    it differ from the bytes stored, so a float32 change the format cannot see is not reported.  Runs on ``stream`` (torch's
    current stream of the device by default), synchronises it, and returns ``(ids[:m], rows[:m] or None, report)`` with
    ``report`` a ``DiffReport`` — the delta ``update_rows`` takes."""
    import torch
    ids, rows, report_t = diff_async(table, src, row0=row0, want_rows=want_rows, stream=stream)
    torch.cuda.ExternalStream(_stream_of(torch, table.device, stream), device=table.device).synchronize()
    report = _report_of(DiffReport, report_t)
    m = report.changed
    return ids[:m], rows[:m] if rows is not None else None, report


def _host_master_of(torch, table, master_cpu, who: str, chunk_rows: int):
    if master_cpu.dtype != torch.float32 or master_cpu.dim() != 2 or master_cpu.is_cuda:
        raise ValueError(f"{who} takes a float32 [rows, dim] tensor on the host")
    if chunk_rows <= 0:
        raise ValueError("chunk_rows must be positive")
    _name, dim = _kind_and_dim(table, "table")
    if tuple(master_cpu.shape) != (int(table.shape[0]), dim):
        raise ValueError(f"the master is {tuple(master_cpu.shape)}; the table has {table.shape[0]} rows of dim {dim}")
    return int(table.shape[0]), dim


def diff_from_host(table, master_cpu, chunk_rows: int = 1 << 16):
    """``diff`` of the device ``table`` against a whole new master in HOST memory (torch CPU tensor, float32 ``[rows, dim]``,
    as many rows as the table), streamed through ONE pinned bounce buffer and one device buffer of ``chunk_rows`` rows, as
    ``convert_from_host`` streams a table: the device never holds the float32 master.  Synchronises torch's current stream once
    per chunk and returns the concatenated delta ``(ids, rows, report)`` — ascending ids, ``report`` a ``DiffReport`` of the
    whole table."""
    import torch
    rows, dim = _host_master_of(torch, table, master_cpu, "diff_from_host", chunk_rows)
    device = table.device
    chunk = min(chunk_rows, max(rows, 1))
    bounce = torch.empty((chunk, dim), dtype=torch.float32, pin_memory=True)
    staged = torch.empty((chunk, dim), dtype=torch.float32, device=device)
    ids, deltas, first, last = [], [], -1, -1
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        for r0 in range(0, rows, chunk):
            n = min(chunk, rows - r0)
            bounce[:n].copy_(master_cpu[r0:r0 + n])
            staged[:n].copy_(bounce[:n], non_blocking=True)
            ids_d, rows_d, report_t = diff_async(table, staged[:n], row0=r0, stream=stream.cuda_stream)
            stream.synchronize()                      # the bounce buffer's copy has left it; the chunk's m is known
            r = _report_of(DiffReport, report_t)
            if r.changed:
                ids.append(ids_d[:r.changed].clone())
                deltas.append(rows_d[:r.changed].clone())
                first, last = (r.first_changed if first < 0 else first), r.last_changed
    m = sum(int(t.shape[0]) for t in ids)
    all_ids = torch.cat(ids) if ids else torch.empty((0,), dtype=torch.int64, device=device)
    all_rows = torch.cat(deltas) if deltas else torch.empty((0, dim), dtype=torch.float32, device=device)
    return all_ids, all_rows, DiffReport(rows, m, first, last)


def sync_from_host(table, master_cpu, digest: Optional[int] = None, chunk_rows: int = 1 << 16):
    """Make the device ``table`` what ``convert`` writes from a whole new master in HOST memory, rewriting only the rows whose
    stored bytes change: per chunk, on torch's current stream, copy -> ``diff_async`` -> ``update_rows`` of the padded outputs,
    through one pinned bounce buffer and one device buffer of ``chunk_rows`` rows.  With ``digest`` (that of the whole table
    before) the ``digest_rows`` bookkeeping of ``apply_delta`` runs around every update.  Returns the number of rows rewritten,
    or ``(rows rewritten, new digest)`` when ``digest`` was given."""
    import torch
    rows, dim = _host_master_of(torch, table, master_cpu, "sync_from_host", chunk_rows)
    name, _dim = _kind_and_dim(table, "table")
    device = table.device
    L = _lib.load()
    chunk = min(chunk_rows, max(rows, 1))
    n_chunks = (rows + chunk - 1) // chunk
    bounce = torch.empty((chunk, dim), dtype=torch.float32, pin_memory=True)
    staged = torch.empty((chunk, dim), dtype=torch.float32, device=device)
    size = C.sizeof(_lib.TableDigest)
    reports = []
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        s = stream.cuda_stream
        if digest is not None:
            outs, workspace = _digest_buffers(torch, L, device, s, n_out=2 * max(n_chunks, 1))
        for k, r0 in enumerate(range(0, rows, chunk)):
            n = min(chunk, rows - r0)
            stream.synchronize()                      # the bounce buffer's last copy has left it
            bounce[:n].copy_(master_cpu[r0:r0 + n])
            staged[:n].copy_(bounce[:n], non_blocking=True)
            ids_d, rows_d, report_t = diff_async(table, staged[:n], row0=r0, stream=s)
            if digest is not None:
                _enqueue_digest_rows(L, table, name, dim, ids_d, n, 0, 1, outs.data_ptr() + 2 * k * size, workspace, s)
            update_rows(table, ids_d, rows_d, stream=s)
            if digest is not None:
                _enqueue_digest_rows(L, table, name, dim, ids_d, n, 0, 1, outs.data_ptr() + (2 * k + 1) * size, workspace, s)
            reports.append(report_t)
        stream.synchronize()
    changed = sum(_report_of(DiffReport, t).changed for t in reports)
    if digest is None:
        return changed
    new = int(digest)
    if n_chunks:
        records = _digests_of(outs)
        for k in range(n_chunks):
            new = new - int(records[2 * k].sum) + int(records[2 * k + 1].sum)
    return changed, new % (1 << 64)
