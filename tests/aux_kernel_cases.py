"""The kernels of recom_amd/csrc/fcp_kernels.hip outside the fused matrix (tests/kernel_variant_cases.py), as explicit
cells, and NumPy restatements of what each must compute (tests/test_gpu_aux_kernels.py on the GPU; the inventory of
tests/test_host.py on the CPU).  Test data only.

  * fcp_segment_offsets_kernel — the pre-pass: raw CSR offsets of (mapped) segment ids, or the inverse map of an any-order
    ScatterNd column;
  * fcp_shard_finalize_kernel<V> — rank-order adds of the partial slices, then the mean division;
  * fcp_concat_outputs_kernel<VEC> — ConcatOutputs, VEC from the alignment of every address of a launch;
  * fcp_upload_kernel — descriptor upload (FCP_DYN_UPLOAD=kernel);
  * fcp_h2d_copy_kernel — the request stager's copy.

Every comparison is of bit patterns (uint32 views): -0.0 against +0.0 and NaN payloads count."""
import dataclasses
import itertools
from typing import List

import numpy as np

from recom_amd.plan import (COMBINER_MEAN, COMBINER_NONE, COMBINER_SUM, FORM_BATCH_COL_REDUCTION, FORM_EXTERNAL,
                            FORM_GATHER, FORM_GATHER_SCATTER, FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE, IDS_F32_BUCKETIZE,
                            IDS_I32, IDS_I64, ROWS_FROM_GROUP, ROWS_FROM_IDS, ROWS_FROM_INPUT_DIM0, ROWS_FROM_SYMBOL,
                            SEG_CSR_I32, SEG_IDS_I32, SEG_IDS_I64, SEG_NONE, XFORM_FILTER, ColumnSpec, PlanSpec,
                            FLAG_COUNT_BAD_IDS)

# the launch counters (recom_amd.lib.AUX_KERNELS) and the instantiations of the fused matrix: together, every kernel of
# the code object
AUX_INSTANTIATIONS = {
    "segment_offsets": "fcp_segment_offsets_kernel",
    "shard_finalize_v4": "fcp_shard_finalize_kernel<4>", "shard_finalize_v2": "fcp_shard_finalize_kernel<2>",
    "shard_finalize_v1": "fcp_shard_finalize_kernel<1>",
    "concat_v4": "fcp_concat_outputs_kernel<4>", "concat_v2": "fcp_concat_outputs_kernel<2>",
    "concat_v1": "fcp_concat_outputs_kernel<1>",
    "upload": "fcp_upload_kernel", "h2d_copy": "fcp_h2d_copy_kernel",
}

BLOCK = 256                       # FCP_BLOCK_THREADS
SEG_IDS_PER_BLOCK = 4 * BLOCK     # FCP_SEG_IDS_PER_BLOCK: ids per pre-pass block
CONCAT_CHUNK = 192                # FCP_CONCAT_CHUNK: inputs per concat launch
SENTINEL = np.uint32(0x7FC0DEAD)  # a NaN no kernel computes: prefilled where outputs go
NEG0 = np.float32(-0.0)
NAN_PAYLOAD = np.uint32(0x7FC01234).view(np.float32)
SUBNORMAL = np.uint32(0x00000301).view(np.float32)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, want, what) -> None:
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    diff = g != w
    if diff.any():
        idx = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} elements differ bit for bit, first {idx}: got {g[idx]:#010x} "
                             f"want {w[idx]:#010x}")


def counter_delta(before: dict, after: dict) -> dict:
    """The counters that moved."""
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def special_values(rng, shape) -> np.ndarray:
    """float32 payload with -0.0, +-inf, NaNs with payloads and subnormals among normal values."""
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    sp = np.asarray([NEG0, np.inf, -np.inf, NAN_PAYLOAD, np.uint32(0xFFC00077).view(np.float32), SUBNORMAL,
                     -SUBNORMAL, 0.0], np.float32)
    if flat.size:
        pick = rng.random(flat.size) < 0.2
        flat[pick] = sp[rng.integers(0, sp.size, int(pick.sum()))]
        flat[:min(flat.size, sp.size)] = sp[:min(flat.size, sp.size)]
    return x


# ---- pre-pass ----------------------------------------------------------------------------------------------------------
PREPASS_NNZ = (0, 1, 63, 64, 65, 255, 256, 1023, 1024, 1025, 4 * SEG_IDS_PER_BLOCK + 77)
PREPASS_KINDS = ("ids_i32", "ids_i64", "indices2", "mul3", "div_const", "div_sym")
PREPASS_PLACEMENTS = ("lane0", "block_start", "span_block", "empty_runs", "one_row", "bad_ends", "rows1")


@dataclasses.dataclass(frozen=True)
class PrepassCell:
    kind: str
    nnz: int
    placement: str
    any_order: bool

    @property
    def id(self) -> str:
        return f"{self.kind}-nnz{self.nnz}-{self.placement}-{'anyorder' if self.any_order else 'stream'}"


def prepass_cells() -> List[PrepassCell]:
    """Every segment kind at every nnz (one placement each, cycling), and every placement at a few nnz, both orders."""
    out = []
    for j, (kind, nnz) in enumerate(itertools.product(PREPASS_KINDS, PREPASS_NNZ)):
        out.append(PrepassCell(kind, nnz, PREPASS_PLACEMENTS[j % len(PREPASS_PLACEMENTS)], j % 2 == 1))
    for j, (pl, nnz, ao) in enumerate(itertools.product(PREPASS_PLACEMENTS, (1025, 4 * SEG_IDS_PER_BLOCK + 77),
                                                        (False, True))):
        out.append(PrepassCell(PREPASS_KINDS[j % len(PREPASS_KINDS)], nnz, pl, ao))
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


def prepass_rows(cell: PrepassCell, rng) -> (np.ndarray, int):
    """Sorted row ids [nnz] (int64) of the placement and the row count."""
    n = cell.nnz
    if cell.placement == "rows1":
        return np.zeros(n, np.int64), 1
    if cell.placement == "one_row":
        return np.full(n, 5, np.int64), 11
    rows = max(n // 3, 2) + 5
    if cell.placement == "empty_runs":         # runs of empty rows, one across every block boundary
        r = np.sort(rng.integers(0, rows, n))
        for b in range(SEG_IDS_PER_BLOCK, n, SEG_IDS_PER_BLOCK):
            r[b:] = np.maximum(r[b:], r[b - 1] + 4)
        rows = int(r.max()) + 3 if n else rows
        return r, rows
    if cell.placement in ("lane0", "block_start"):   # bags start at wave lanes 0 / at block starts
        step = 64 if cell.placement == "lane0" else SEG_IDS_PER_BLOCK
        r = np.arange(n, dtype=np.int64) // step
        return r, int(r.max()) + 2 if n else 2
    if cell.placement == "span_block":          # one bag across every block boundary
        r = np.sort(rng.integers(0, rows, n))
        for b in range(SEG_IDS_PER_BLOCK, n, SEG_IDS_PER_BLOCK):
            lo, hi = max(b - 40, 0), min(b + 40, n)
            r[lo:hi] = r[lo]
        return np.maximum.accumulate(r), rows
    # bad_ends: ids < 0 in front (not for the division maps: C's division truncates toward zero, a negative idx0 is not
    # a negative row there), ids >= rows at the tail
    r = np.sort(rng.integers(0, rows, n))
    k = min(n // 5, 40)
    if k:
        if not cell.kind.startswith("div"):
            r[:k] = -np.sort(rng.integers(1, 9, k))[::-1]
        r[n - k:] = rows + np.sort(rng.integers(0, 9, k))
    return np.sort(r), rows


def prepass_column(kind: str, ids_input: int, seg_input: int, table: int, n_groups: int):
    """A pooled mean column whose segment input has the encoding `kind` (symbol 1 is the map's factor for div_sym)."""
    base = dict(form=FORM_SEGMENT_REDUCE, dim=4, vocab=50, combiner=COMBINER_MEAN, id_source=IDS_I32, table_input=table,
                ids_input=ids_input, seg_input=seg_input, rows_source=ROWS_FROM_SYMBOL, rows_arg=0, concat_group=0)
    if kind == "ids_i32":
        return ColumnSpec(seg_kind=SEG_IDS_I32, seg_stride=1, **base)
    if kind == "ids_i64":
        return ColumnSpec(seg_kind=SEG_IDS_I64, seg_stride=1, **base)
    if kind == "indices2":
        return ColumnSpec(seg_kind=SEG_IDS_I64, seg_stride=2, **base)
    if kind == "mul3":            # row = idx0 * 3 + idx1 of [nnz, 3] indices
        return ColumnSpec(seg_kind=SEG_IDS_I64, seg_stride=3, seg_mul=(3, 1), seg_div=1, **base)
    if kind == "div_const":       # row = idx0 // 4
        return ColumnSpec(seg_kind=SEG_IDS_I64, seg_stride=2, seg_mul=(1,), seg_div=4, **base)
    # div_sym: row = idx0 // symbols[1]
    return ColumnSpec(seg_kind=SEG_IDS_I64, seg_stride=2, seg_mul=(1,), seg_div=1, seg_sym=1, seg_sym_slot=4, **base)


DIV_SYM = 3


def prepass_segment_input(kind: str, rows_ids: np.ndarray, rng) -> np.ndarray:
    """The segment tensor whose mapped row ids are `rows_ids` (negative ones included: Python's floor division)."""
    n = rows_ids.size
    if kind == "ids_i32":
        return rows_ids.astype(np.int32)
    if kind == "ids_i64":
        return rows_ids.astype(np.int64)
    if kind == "indices2":
        return np.stack([rows_ids, rng.integers(0, 7, n)], 1).astype(np.int64)
    if kind == "mul3":
        q, r = np.divmod(rows_ids, 3)
        return np.stack([q, r, rng.integers(0, 7, n)], 1).astype(np.int64)
    f = 4 if kind == "div_const" else DIV_SYM
    # idx0 anywhere in [row * f, row * f + f): only the mapped rows need to be sorted (rows >= 0: see prepass_rows)
    idx0 = rows_ids * f + rng.integers(0, f, n)
    return np.stack([idx0, rng.integers(0, 7, n)], 1).astype(np.int64)


def mapped_rows(kind: str, seg: np.ndarray) -> np.ndarray:
    """The segment map of the kind, restated (int64 floor division, as the kernel's)."""
    s = np.asarray(seg).astype(np.int64)
    if kind in ("ids_i32", "ids_i64"):
        return s.reshape(-1)
    if kind == "indices2":
        return s[:, 0]
    if kind == "mul3":
        return s[:, 0] * 3 + s[:, 1]
    return s[:, 0] // (4 if kind == "div_const" else DIV_SYM)


def raw_offsets(row_ids: np.ndarray, rows: int) -> np.ndarray:
    """What the pre-pass writes for entries 0..rows: np_segment_offsets of the ids clamped to `rows` (ids < 0 lie before
    row 0 and shift its start; ids >= rows lie after the last row)."""
    import fcp_oracle
    return fcp_oracle.np_segment_offsets(np.minimum(row_ids, rows), rows)


# ---- finalize ----------------------------------------------------------------------------------------------------------
FINALIZE_VECS = (4, 2, 1)
FINALIZE_WORLDS = (2, 3, 8)
FINALIZE_SLICES = ("row0", "middle", "last", "all")
FINALIZE_ROWS = 37


@dataclasses.dataclass(frozen=True)
class FinalizeCell:
    vec: int
    world: int
    where: str

    @property
    def id(self) -> str:
        return f"V{self.vec}-world{self.world}-{self.where}"

    def rows(self, B: int):
        """(row_begin, row_count)"""
        return {"row0": (0, 1), "middle": (B // 2, 1), "last": (B - 1, 1), "all": (0, B)}[self.where]


def finalize_cells() -> List[FinalizeCell]:
    return [FinalizeCell(v, w, s) for v, w, s in itertools.product(FINALIZE_VECS, FINALIZE_WORLDS, FINALIZE_SLICES)]


HASH_BUCKETS = 40
FILTER_LO, FILTER_HI = (2, 30), (12, 38)          # kept: [2, 12] and [30, 38]
BUCKETS = np.asarray([-2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0], np.float32)


def finalize_plan(vec: int):
    """One group: gather (-0.0 / NaN / subnormal table rows), ScatterNd over CSR, passthrough, BatchColReduction, an
    EXTERNAL hole, sum and mean over CSR, mean over segment ids, filtered means (hash + intervals; bucketize).  Returns
    (spec, roles)."""
    d = lambda m: vec * m               # noqa: E731  (dims V x odd: the plan's V is exactly vec)
    cols, ranks, esz, roles = [], [], [], []

    def host(rank, e):
        ranks.append(rank)
        esz.append(e)
        return len(ranks) - 1

    k = 0

    def add(role, c):
        nonlocal k
        c.concat_group, c.concat_slot = 0, k
        cols.append(c)
        roles.append(role)
        k += 1

    i = host(1, 4)
    add("gather", ColumnSpec(FORM_GATHER, d(3), 23, COMBINER_NONE, IDS_I32, 0, i, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0))
    i, s = host(1, 8), host(1, 4)
    add("scatter", ColumnSpec(FORM_GATHER_SCATTER, d(1), 23, COMBINER_NONE, IDS_I64, 1, i, s, SEG_CSR_I32, 1,
                              ROWS_FROM_SYMBOL, 0))
    i = host(2, 4)
    add("passthrough", ColumnSpec(FORM_PASSTHROUGH, d(5), 0, COMBINER_NONE, IDS_I32, -1, i, -1, SEG_NONE, 1,
                                  ROWS_FROM_INPUT_DIM0, i))
    i = host(3, 4)
    add("bcr", ColumnSpec(FORM_BATCH_COL_REDUCTION, d(1), 0, COMBINER_NONE, IDS_I32, -1, i, -1, SEG_NONE, 1,
                          ROWS_FROM_INPUT_DIM0, i))
    add("external", ColumnSpec(FORM_EXTERNAL, d(3), 0, COMBINER_NONE, IDS_I32, -1, -1, -1, SEG_NONE, 1, ROWS_FROM_GROUP, 0))
    for role, comb in (("sum_csr", COMBINER_SUM), ("mean_csr", COMBINER_MEAN)):
        i, s = host(1, 4), host(1, 4)
        add(role, ColumnSpec(FORM_SEGMENT_REDUCE, d(7), 23, comb, IDS_I32, 2, i, s, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0))
    i, s = host(1, 8), host(1, 4)
    add("mean_segids", ColumnSpec(FORM_SEGMENT_REDUCE, d(7), 23, COMBINER_MEAN, IDS_I64, 2, i, s, SEG_IDS_I32, 1,
                                  ROWS_FROM_SYMBOL, 0))
    i, s = host(1, 8), host(1, 4)
    add("mean_hash_filter", ColumnSpec(FORM_SEGMENT_REDUCE, d(3), 41, COMBINER_MEAN, IDS_I64, 3, i, s, SEG_IDS_I32, 1,
                                       ROWS_FROM_SYMBOL, 0, xform_mode=XFORM_FILTER, xform_lo=FILTER_LO,
                                       xform_hi=FILTER_HI, hash_buckets=HASH_BUCKETS))
    i, s = host(1, 4), host(1, 4)
    add("mean_bucketize_filter", ColumnSpec(FORM_SEGMENT_REDUCE, d(1), BUCKETS.size + 1, COMBINER_MEAN,
                                            IDS_F32_BUCKETIZE, 4, i, s, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0,
                                            boundaries=BUCKETS, xform_mode=XFORM_FILTER, xform_lo=(1,), xform_hi=(5,)))
    spec = PlanSpec(cols, ranks, esz, 5, n_groups=1, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    return spec, roles


def finalize_tables(spec, rng) -> List[np.ndarray]:
    """Table 0 (gather) and 1 (scatter) carry -0.0, NaN payloads and subnormals in whole rows; the pooled tables are
    normal values here — pooled sums and means over non-finite and subnormal values, through the finalize's adds as well,
    are the cells of tests/value_edge_cases.py (where a NaN an add produced is compared by class, not by payload)."""
    dims = {}
    vocab = {}
    for c in spec.columns:
        if c.table_input >= 0:
            dims[c.table_input] = c.dim
            vocab[c.table_input] = c.vocab
    tabs = []
    for t in range(5):
        x = rng.standard_normal((vocab[t], dims[t])).astype(np.float32)
        if t < 2:
            x[3] = NEG0
            x[5] = NAN_PAYLOAD
            x[7] = SUBNORMAL
            x[8, ::2] = NEG0
        tabs.append(x)
    return tabs


def finalize_request(spec, roles, rng, B: int):
    """Inputs: empty bags, bags of only bad ids, ids that pick the special table rows."""
    inputs = []
    lens = rng.integers(0, 6, B)
    lens[::7] = 0
    special = np.asarray([3, 5, 7, 8], np.int64)
    for c, role in zip(spec.columns, roles):
        if role == "gather":
            ids = rng.integers(0, c.vocab, B)
            ids[::3] = special[np.arange(0, B, 3) % 4]
            ids[1::11] = -1                              # bad ids read zeros
            inputs.append(ids.astype(np.int32))
        elif role == "scatter":
            ln = (np.arange(B) % 4 != 1).astype(np.int64) + (np.arange(B) % 9 == 0)   # 0, 1 or 2 ids a row
            ids = rng.integers(0, c.vocab, int(ln.sum()))
            ids[::2] = special[np.arange(0, ids.size, 2) % 4]
            inputs += [ids.astype(np.int64), np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)]
        elif role == "passthrough":
            inputs.append(special_values(rng, (B, c.dim)))
        elif role == "bcr":
            x = rng.standard_normal((B, 3, c.dim)).astype(np.float32)
            x[::4] = NEG0                                 # a sum of -0.0s
            inputs.append(x)
        elif role == "external":
            continue
        else:
            n = int(lens.sum())
            if role == "mean_bucketize_filter":
                ids = rng.uniform(-3, 4, n).astype(np.float32)
            elif role == "mean_hash_filter":
                ids = rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64)
            else:
                ids = rng.integers(0, c.vocab, n).astype(np.int64 if c.id_source == IDS_I64 else np.int32)
                starts = np.cumsum(lens) - lens
                for r in range(2, B, 9):                  # bags of only bad ids
                    ids[starts[r]:starts[r] + lens[r]] = c.vocab + 1
            if c.seg_kind == SEG_CSR_I32:
                seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            else:
                seg = np.repeat(np.arange(B, dtype=np.int32), lens)
            inputs += [ids, seg]
    return inputs, np.asarray([B], np.int32)


def kept_counts(c, ids: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """Ids of each row a mean divides by: every id of the row (out-of-vocabulary ones too), less the ones the column's
    filter drops (hash and intervals on the raw id; bucketize first)."""
    import fcp_oracle
    keep = np.ones(ids.size, bool)
    if c.xform_mode == XFORM_FILTER:
        if c.id_source == IDS_F32_BUCKETIZE:
            v = fcp_oracle.np_bucketize(c.boundaries, ids).astype(np.int64)
        elif c.hash_buckets:
            v = np.asarray([fcp_oracle.np_fingerprint64(str(int(x)).encode()) % c.hash_buckets for x in ids], np.int64)
        else:
            v = ids.astype(np.int64)
        keep = np.zeros(ids.size, bool)
        for lo, hi in zip(c.xform_lo, c.xform_hi):
            keep |= (v >= lo) & (v <= hi)
    cs = np.concatenate([[0], np.cumsum(keep)])
    lo = np.clip(offsets[:-1], 0, ids.size)
    hi = np.clip(offsets[1:], lo, ids.size)
    return (cs[hi] - cs[lo]).astype(np.int64)


def finalize_restated(spec, slices: np.ndarray, kept: dict) -> np.ndarray:
    """float32: pooled columns — the slices [world, count, width] added in rank order from +0.0, then every mean column
    divided by its kept count where that is > 0 (an unsharded plan — world 1 — divides nowhere: its kernels have); columns
    with one owner per row — the OR of the slices' bits, i.e. the owner's value (every other rank wrote +0.0)."""
    acc = np.zeros(slices.shape[1:], np.float32)
    for w in range(slices.shape[0]):
        acc = acc + slices[w]
    owner = np.bitwise_or.reduce(np.ascontiguousarray(slices, np.float32).view(np.uint32), axis=0).view(np.float32)
    offs = spec.column_offsets()
    for k, c in enumerate(spec.columns):
        if c.form not in (FORM_SEGMENT_REDUCE, FORM_EXTERNAL):
            acc[:, offs[k]:offs[k] + c.dim] = owner[:, offs[k]:offs[k] + c.dim]
    for k, cnt in kept.items():
        c = spec.columns[k]
        sl = acc[:, offs[k]:offs[k] + c.dim]
        m = cnt > 0
        sl[m] = sl[m] / cnt[m, None].astype(np.float32)
    return acc


# ---- concat ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class ConcatCell:
    entry: str            # concat | scatter | strided | host_direct | host_copied
    vec: int              # expected VEC of every launch (chunks of different VEC: 0)
    cause: str            # what forces it: none | out_ptr | width | dim | offset | stride | in_ptr
    dims: tuple           # per input
    prefix: int

    @property
    def id(self) -> str:
        return f"{self.entry}-V{self.vec or 'mixed'}-{self.cause}-n{len(self.dims)}-max{max(self.dims)}-p{self.prefix}"


def _ty(max_dim: int, vec: int) -> int:
    dv = -(-max_dim // vec)
    tx = 1
    while tx < dv and tx < BLOCK:
        tx *= 2
    return BLOCK // tx


def concat_cells() -> List[ConcatCell]:
    out = []
    # VEC 4 / 2 / 1, each forced by each alignment source (4: none of them)
    for entry in ("scatter", "strided"):
        out.append(ConcatCell(entry, 4, "none", (8, 4, 12), 5))
        for cause in ("out_ptr", "width", "dim", "offset", "stride", "in_ptr"):
            if cause == "stride" and entry != "strided":
                continue
            for vec in (2, 1):
                out.append(ConcatCell(entry, vec, cause, (8, 4, 12), 7))
    # tx_log2 0..8 and cpr 1 / 2 / 3: the widest input in vectors; prefix around the tile height ty
    for j, maxv in enumerate((1, 2, 3, 8, 16, 31, 64, 128, 256, 257, 512, 513, 700)):
        vec = (4, 2, 1)[j % 3]
        ty = _ty(maxv * vec, vec)
        for p in sorted({1, max(ty - 1, 1), ty, ty + 1}):
            out.append(ConcatCell("concat", vec, "none", (maxv * vec, vec), p))
    # 192-input chunks: n around the chunk size, the chunks of different VEC
    for n in (1, 191, 192, 193, 385):       # inputs of chunk 0 16-byte aligned, of chunk 1 8-byte, of chunk 2 4-byte
        out.append(ConcatCell("concat", 0 if n > CONCAT_CHUNK else 4, "chunks", tuple(4 for _ in range(n)), 3))
    # the host entry: direct (<= 1 MiB packed) and copied
    out.append(ConcatCell("host_direct", 4, "none", (8, 4, 12), 9))
    out.append(ConcatCell("host_direct", 1, "dim", (8, 5, 12), 9))
    out.append(ConcatCell("host_copied", 4, "none", (256, 128, 4), 1100))
    out.append(ConcatCell("host_copied", 2, "offset", (256, 130, 4), 1100))
    return out
