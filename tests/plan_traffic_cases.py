"""fcp_plan_traffic_count (recom_amd/csrc/fcp_table_traffic.hip, fcp_process.hip): the value model restated in NumPy, the
kernel's constants, and the small plans of tests/test_plan_traffic_host.py (CPU) and tests/test_zz_gpu_plan_traffic.py (GPU).
Test data only.

expected_counts is built from pieces that tests/test_oracle.py pins: fcp_oracle.np_bucketize, np_fingerprint64 of the decimal
string, the closed-interval test of SELECT / FILTER, and the 64-bit unsigned compare against the column's vocab.  Every id
that reaches the lookup counts once: each id of a bag, a scatter column's overwritten ids, ids of weight 0."""
import dataclasses

import numpy as np

import fcp_oracle as O
from recom_amd.plan import (COMBINER_NONE, COMBINER_SUM, FORM_GATHER, FORM_GATHER_SCATTER, FORM_SEGMENT_REDUCE,  # noqa: F401
                            IDS_F32_BUCKETIZE, IDS_I32, IDS_I64, ROWS_FROM_IDS, ROWS_FROM_SYMBOL, SEG_CSR_I32, SEG_NONE,
                            XFORM_FILTER, XFORM_NONE, XFORM_SELECT, ColumnSpec, PlanSpec)

# the kernel's constants (fcp_table_traffic.hip)
THREADS = 256                      # kTrafficThreads
IDS_PER_THREAD = 4                 # kTrafficIdsPerThread
TILE = THREADS * IDS_PER_THREAD    # kTrafficTile: positions of an id stream per block
CELLS = 2048                       # kTrafficSlots: cells of a block's LDS table; home slot = row mod CELLS
PROBES = 4                         # kCountProbes
INT64_MIN = -2 ** 63
LOOKUP_FORMS = (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER)


def lookup_ids(c, inputs) -> np.ndarray:
    """int64: the ids of column `c` that reach the lookup, in stream order — decoded (int32 widens with its sign, float32 is
    bucketized), hashed, then SELECT substitutes / FILTER drops what lies outside the closed intervals."""
    raw = np.asarray(inputs[c.ids_input]).reshape(-1)
    ids = O.np_bucketize(c.boundaries, raw).astype(np.int64) if c.id_source == IDS_F32_BUCKETIZE else raw.astype(np.int64)
    if c.hash_buckets:
        ids = np.asarray([O.np_fingerprint64(str(int(v)).encode()) % c.hash_buckets for v in ids], np.int64).reshape(-1)
    if c.xform_mode == XFORM_NONE:
        return ids
    inside = np.zeros(ids.size, bool)
    for lo, hi in zip(c.xform_lo, c.xform_hi):
        inside |= (ids >= lo) & (ids <= hi)
    if c.xform_mode == XFORM_SELECT:
        return np.where(inside, ids, np.int64(c.xform_substitute)).astype(np.int64)
    return ids[inside]


def n_filtered(c, inputs) -> int:
    """ids of column `c` its FILTER drops"""
    return int(np.asarray(inputs[c.ids_input]).size - lookup_ids(c, inputs).size)


def table_rows(spec) -> list:
    """fcp_plan_table_rows: per device input the largest vocab of the lookup columns that read it, -1 for an unread input"""
    rows = [-1] * spec.n_device_inputs
    for c in spec.columns:
        if c.form in LOOKUP_FORMS:
            rows[c.table_input] = max(rows[c.table_input], int(c.vocab))
    return rows


def expected_counts(spec, inputs, symbols=None, start=None):
    """(list of uint32 arrays — None for a device input no lookup column reads —, skipped) of one request: `start` (default
    zeros) plus, per lookup column, the occurrences of every row among its lookup_ids, modulo 2^32; an id outside [0, vocab) of
    ITS column — compared as unsigned 64-bit numbers — adds 1 to skipped."""
    rows = table_rows(spec)
    acc = [None if r < 0 else (np.zeros(r, np.uint64) if start is None or start[t] is None else np.asarray(start[t], np.uint32).astype(np.uint64))
           for t, r in enumerate(rows)]
    skipped = 0
    for c in spec.columns:
        if c.form not in LOOKUP_FORMS:
            continue
        ids = lookup_ids(c, inputs)
        good = ids.view(np.uint64) < np.uint64(c.vocab)
        skipped += int((~good).sum())
        acc[c.table_input] += np.bincount(ids[good], minlength=rows[c.table_input]).astype(np.uint64)
    return [None if a is None else (a & np.uint64(0xFFFFFFFF)).astype(np.uint32) for a in acc], skipped


# ---- small plans ------------------------------------------------------------------------------------------------------------
def gather_col(k, vocab, table, id_source=IDS_I64, dim=4, **kw):
    """GATHER column k: host input k holds its ids, one per row"""
    return ColumnSpec(FORM_GATHER, dim, vocab, COMBINER_NONE, id_source, table, k, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0,
                      kw.pop("boundaries", None), 0, k, **kw)


def gather_spec(cols, n_tables):
    """a one-group plan of GATHER columns, host input k = ids of column k"""
    esz = [8 if c.id_source == IDS_I64 else 4 for c in cols]
    spec = PlanSpec(list(cols), [1] * len(cols), esz, n_tables, n_groups=1, n_symbols=0)
    spec.validate()
    return spec


def bag_spec(n_cols, vocab, tables, dim=4, combiner=COMBINER_SUM, id_source=IDS_I64):
    """a one-group plan of `n_cols` pooled columns with CSR offsets: host inputs 2k (ids) and 2k + 1 (int32 offsets [rows + 1]),
    rows = symbol 0; tables[k] = the device input column k reads"""
    cols = [ColumnSpec(FORM_SEGMENT_REDUCE, dim, vocab, combiner, id_source, tables[k], 2 * k, 2 * k + 1, SEG_CSR_I32, 1,
                       ROWS_FROM_SYMBOL, 0, None, 0, k) for k in range(n_cols)]
    spec = PlanSpec(cols, [1] * (2 * n_cols), [8 if id_source == IDS_I64 else 4, 4] * n_cols, max(tables) + 1, n_groups=1, n_symbols=1)
    spec.validate()
    return spec


def bag_inputs(id_streams, rows, id_dtype=np.int64):
    """host inputs of a bag_spec request: every stream dealt over `rows` bags as evenly as CSR offsets allow"""
    out = []
    for ids in id_streams:
        ids = np.asarray(ids, id_dtype)
        out += [ids, np.floor(np.arange(rows + 1) * (ids.size / max(rows, 1))).astype(np.int32) if rows else np.zeros(1, np.int32)]
        if rows:
            out[-1][-1] = ids.size
    return out


def hand_example():
    """Three columns, written out by hand (tests/test_plan_traffic_host.py): column 0 FILTERs [0, 9] on table 0 (vocab 6),
    column 1 reads table 1 (vocab 5) by int32 ids, column 2 shares table 1 with the smaller vocab 4.
    ids 0: [1, 12, 5, 7, 1]  -> 12 filtered, 7 kept and outside vocab 6 (skipped), rows 1, 5, 1
    ids 1: [4, 0, 4, -1, 2]  -> -1 skipped, rows 4, 0, 4, 2
    ids 2: [3, 4, 0, 3, 3]   -> 4 is outside THIS column's vocab 4 (skipped) though table 1 has a row 4; rows 3, 0, 3, 3"""
    cols = [gather_col(0, 6, 0, xform_mode=XFORM_FILTER, xform_lo=(0,), xform_hi=(9,)),
            gather_col(1, 5, 1, IDS_I32), gather_col(2, 4, 1)]
    inputs = [np.asarray([1, 12, 5, 7, 1], np.int64), np.asarray([4, 0, 4, -1, 2], np.int32), np.asarray([3, 4, 0, 3, 3], np.int64)]
    want = [np.asarray([0, 2, 0, 0, 0, 1], np.uint32), np.asarray([2, 0, 1, 3, 2], np.uint32)]
    return gather_spec(cols, 2), inputs, want, 3


def with_replaced(spec, **kw):
    out = dataclasses.replace(spec, **kw)
    out.validate()
    return out
