"""Table conversion on the device (``fcp_table_convert``, recom_amd/csrc/fcp_convert.hip): float32 embedding tables to the
formats the plans read — bf16, fp16 and 8-bit row-quantised ("q8") — and back, on torch device tensors.

Plans do not quantise; this does, once, at load time.  The value model is the header's (include/fcp_hip.h): float32 -> q8 is
exactly the tensor ``quantized::embedding_bag_byte_prepack`` returns, q8 -> float32 is ``fma(code, scale, bias)`` rounded
once, float32 -> 16-bit is one rounding to nearest-even, 16-bit -> float32 is exact.  Nothing here falls back to torch: a
missing library or device is an error.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

from . import lib as _lib
from .plan import FORM_GATHER, FORM_GATHER_SCATTER, FORM_SEGMENT_REDUCE, PlanSpec

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
    dim = t.shape[1] - 8 if name == "q8" else t.shape[1]
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
        out = torch.empty((rows, dim + 8 if dtype == "q8" else dim), dtype=_torch_dtypes()[dtype], device=src.device)
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
    out = torch.empty((rows, dim + 8 if dtype == "q8" else dim), dtype=_torch_dtypes()[dtype], device=device)
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
