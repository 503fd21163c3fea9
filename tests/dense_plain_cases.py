"""Plans and requests for the plain dense kernel (fcp_dense_kernel_plain, recom_amd/csrc/fcp_dense_plain.hip): float32
concat plans of one group whose columns are all gathers by int32 ids, int64 ids or float32 values bucketized with
reproducible boundaries.  Test data only (tests/test_gpu_dense_plain.py, tests/test_dense_plain_host.py).

Widths are chosen around the 64-slot span (a slot is 4 floats): exactly one span, one span plus one slot, 64 columns of
dim 4 in one span (1 024 (column, row) pairs: four passes of the pair loop), a dim-64 column that starts at slot 60
(straddles two spans: it is in both span records and its bad ids count once), a dim-512 column that covers two whole
spans, and dims 4..128 mixed over ten spans (eight or more spans take the XCD mapping with its padded, idle blocks).
Ids carry every edge of the conversion: -1, vocab, the type's minimum, 2^32 + k (int64), vocab 1, and for bucketized
values a boundary, its two neighbours, below the first and above the last boundary, +-inf and NaN."""
import dataclasses
import functools
from typing import List

import numpy as np

from recom_amd.plan import (COMBINER_NONE, FLAG_COUNT_BAD_IDS, FORM_GATHER, IDS_F32_BUCKETIZE, IDS_I32, IDS_I64, ROWS_FROM_IDS,
                            SEG_NONE, ColumnSpec, PlanSpec)

ROWS = (64, 65, 79, 80)                  # R = 4 from 64 rows on; 16 rows per block: full, one over, one short of the fifth, full
BOUNDARIES = np.arange(0.0, 40.0, 5.0, dtype=np.float32)      # 0, 5, ..., 35: reproducible as fma(i, 5, 0)
WIDTHS = {
    "one_span": [64, 128, 32, 32],
    "span_plus_slot": [64, 128, 32, 32, 4],
    "cols64": [4] * 64,
    "straddle": [240, 64, 8],
    "dim512": [512, 16],
    "mixed": [4, 8, 12, 20, 128, 64, 36, 100, 16, 4, 72, 128, 44, 28, 8, 124] * 3 + [128, 128, 16],
}


@dataclasses.dataclass
class Case:
    spec: PlanSpec
    tables: List[np.ndarray]


def gather(dim, vocab, src, table, host, slot, boundaries=None, group=0, **kw) -> ColumnSpec:
    return ColumnSpec(FORM_GATHER, dim, vocab, COMBINER_NONE, src, table, host, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0,
                      boundaries, group, slot, **kw)


@functools.lru_cache(maxsize=None)
def build_case(width: str, count_bad: bool = True) -> Case:
    rng = np.random.default_rng(sorted(WIDTHS).index(width) + 17)
    cols, ranks, esz, tables = [], [], [], []
    for k, dim in enumerate(WIDTHS[width]):
        src = (IDS_I32, IDS_I64, IDS_F32_BUCKETIZE)[k % 3]
        vocab = 1 if k % 7 == 3 else int(rng.integers(5, 40))         # (below 9: some buckets are outside the table)
        t = rng.standard_normal((vocab, dim)).astype(np.float32)
        t[0, 0] = -0.0
        tables.append(t)
        ranks.append(1)
        esz.append(8 if src == IDS_I64 else 4)
        cols.append(gather(dim, vocab, src, k, k, k, BOUNDARIES if src == IDS_F32_BUCKETIZE else None))
    spec = PlanSpec(cols, ranks, esz, len(tables), flags=FLAG_COUNT_BAD_IDS if count_bad else 0)
    spec.validate()
    return Case(spec, tables)


def make_inputs(spec: PlanSpec, rows: int, seed: int) -> List[np.ndarray]:
    """One id / value tensor per gather column (other forms: see the gate test), with the edge values at fixed rows."""
    rng = np.random.default_rng(seed)
    out = []
    for k, c in enumerate(spec.columns):
        if c.form != FORM_GATHER:
            continue
        if c.id_source == IDS_F32_BUCKETIZE:
            b = np.asarray(c.boundaries, np.float32)
            x = rng.uniform(float(b[0]) - 5.0, float(b[-1]) + 5.0, rows).astype(np.float32)
            edge = [b[1], np.nextafter(b[1], np.float32(-np.inf)), np.nextafter(b[1], np.float32(np.inf)), b[0], b[-1],
                    np.float32(b[0] - 3.0), np.float32(1e9), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan),
                    np.float32(-0.0)]
            for i, v in enumerate(edge):
                x[(5 * k + 3 * i) % rows] = v
            out.append(x)
        else:
            dt = np.int64 if c.id_source == IDS_I64 else np.int32
            ids = rng.integers(0, c.vocab, rows).astype(dt)
            edge = [-1, c.vocab, np.iinfo(dt).min, np.iinfo(dt).max, c.vocab - 1, 0]
            if dt == np.int64:
                edge += [2 ** 32 + 0, 2 ** 32 + (c.vocab - 1), -2 ** 32, 2 ** 31]
            for i, v in enumerate(edge):
                ids[(5 * k + 3 * i) % rows] = v
            out.append(ids)
    return out


def restate(spec: PlanSpec, tables, inputs, rows: int):
    """(float32 [rows, width], bad ids) of a plan of gather columns, in NumPy: Bucketize = the number of boundaries <= value
    (NaN: all of them), an id outside [0, vocab) — the whole 64-bit id — reads zeros and counts once."""
    offs = spec.column_offsets()
    out = np.zeros((rows, spec.group_width(0)), np.float32)
    bad = 0
    for k, c in enumerate(spec.columns):
        x = inputs[c.ids_input]
        if c.id_source == IDS_F32_BUCKETIZE:
            idx = np.searchsorted(np.asarray(c.boundaries, np.float32), x, side="right").astype(np.int64)
        else:
            idx = x.astype(np.int64)
        ok = (idx >= 0) & (idx < c.vocab)
        bad += int((~ok).sum())
        out[ok, offs[k]:offs[k] + c.dim] = tables[c.table_input][idx[ok]]
    return out, bad
