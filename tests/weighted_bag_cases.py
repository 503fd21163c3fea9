"""Pooled columns with per-id weights and the sqrtn combiner, as explicit cells: plans + requests that land in the
weighted ragged kernel (fcp_weighted_bag_kernel<V, SHARDED>), and the restatement of their arithmetic in float32 NumPy —
the contract of include/fcp_hip.h (fcp_column_ext_t::weights_input1, FCP_COMBINER_SQRTN), written out once more:

  * ids pass through hash / id transform / vocabulary check / row shard as in every lookup column; an id the FILTER drops
    contributes neither a term nor a weight; an id outside [0, vocab) reads a row of zeros and its weight counts;
  * numerator, in id order from +0.0f: unweighted acc = acc + row; weighted acc = fl32(acc + fl32(w * row)) — a rounded
    product, then a rounded add (`restate(..., fused=True)` is the contracted variant the kernels must NOT compute);
  * denominator d, float32, in id order from +0.0f over the kept ids: MEAN the count / the sum of the weights, SQRTN the
    correctly rounded square root of the count / of the sum of the rounded squares; none for SUM;
  * one IEEE float32 division acc / d per element; d == 0 gives a row of +0.0 whatever the numerator holds;
  * row-sharded plans: a rank adds the rows it owns (an id outside the vocabulary is a zero row on EVERY rank: its product
    is added everywhere) and divides nothing; the finalize adds the slices in rank order and divides by the d of the WHOLE
    row (`finalize_restated`).

Test data only: used by tests/test_weighted_bags_host.py (no GPU) and tests/test_gpu_weighted_bags.py."""
import dataclasses
import functools
from typing import List

import numpy as np

import value_edge_cases as E
from kernel_variant_cases import CAPW, EDGE_LENS
from recom_amd.plan import (COMBINER_MEAN, COMBINER_NONE, COMBINER_SQRTN, COMBINER_SUM, FLAG_COUNT_BAD_IDS, FORM_GATHER,
                            FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE, IDS_I32, IDS_I64, ROWS_FROM_IDS, ROWS_FROM_INPUT_DIM0,
                            ROWS_FROM_SYMBOL, SEG_CSR_I32, SEG_IDS_I32, SEG_IDS_I64, SEG_NONE, XFORM_FILTER, XFORM_SELECT,
                            ColumnSpec, PlanSpec)

VECS = (1, 2, 4)
FORMS = ("wsum", "wmean", "wsqrtn", "sqrtn")            # weighted sum / mean / sqrtn, unweighted sqrtn
ENCODINGS = ("csr", "ids32", "idx64")                   # CSR int32, sorted ids int32, SparseTensor indices int64 stride 2
ID_PATHS = ("filter", "select", "hash", "oov")
WORLDS = (2, 3)
_COMBINER = {"wsum": COMBINER_SUM, "wmean": COMBINER_MEAN, "wsqrtn": COMBINER_SQRTN, "sqrtn": COMBINER_SQRTN,
             "sum": COMBINER_SUM, "mean": COMBINER_MEAN}
NAN_PAYLOAD = E.NAN_PAYLOAD
FLT_MAX = np.finfo(np.float32).max


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _rows_of_groups(spec, inputs, symbols) -> dict:
    rows = {}
    for c in spec.columns:
        if c.rows_source == ROWS_FROM_SYMBOL:
            rows[c.concat_group] = int(symbols[c.rows_arg])
        elif c.form == FORM_GATHER:
            rows[c.concat_group] = int(np.asarray(inputs[c.ids_input]).size)
        elif c.form == FORM_PASSTHROUGH:
            rows[c.concat_group] = int(inputs[c.ids_input].shape[0])
    return rows


def _weights_of(c: ColumnSpec, inputs):
    return None if c.weights_input < 0 else np.asarray(inputs[c.weights_input], np.float32).ravel()


def denominator(c: ColumnSpec, kept: np.ndarray, w) -> "np.float32 | None":
    """d of one bag (`kept`: bool per id of the bag, `w`: its weights or None), float32, accumulated in id order."""
    if c.combiner == COMBINER_SUM:
        return None
    if w is None:
        d = np.float32(int(kept.sum()))
    else:
        d = np.float32(0.0)
        with np.errstate(all="ignore"):
            for i in np.flatnonzero(kept):
                d = np.float32(d + (np.float32(w[i] * w[i]) if c.combiner == COMBINER_SQRTN else w[i]))
    if c.combiner == COMBINER_SQRTN:
        with np.errstate(all="ignore"):
            d = np.sqrt(np.float32(d))
    return np.float32(d)


def _divide(acc: np.ndarray, d) -> np.ndarray:
    if d is None:
        return acc
    if d == 0:
        return np.zeros_like(acc)
    with np.errstate(all="ignore"):
        return (acc / d).astype(acc.dtype)


@dataclasses.dataclass
class Restated:
    groups: list      # per group float32 (or float64) [rows, width]
    bad: int          # ids that reached the lookup outside the vocabulary
    kept: list        # per group float64 [rows, width]: ids the bag of a WEIGHTED pooled element kept, -1 elsewhere
    pooled: list      # per group bool [width]: elements of pooled columns


def restate(spec: PlanSpec, tables, inputs, symbols, rank: int = 0, world: int = 1, fused: bool = False,
            f64: bool = False) -> Restated:
    """One request.  `tables` are the GLOBAL tables; a rank of a row-sharded plan (world > 1) adds what it owns and divides
    nothing.  fused: the contracted numerator fl32(acc + w * x), product exact in float64 — what the kernels must not
    compute.  f64: the same semantics in float64 throughout (the truth the float32 results are bounded against)."""
    ft = np.float64 if f64 else np.float32
    offs = spec.column_offsets()
    rows_g = _rows_of_groups(spec, inputs, symbols)
    out = [np.zeros((rows_g[g], spec.group_width(g)), ft) for g in range(spec.n_groups)]
    kept_n = [np.full((rows_g[g], spec.group_width(g)), -1.0) for g in range(spec.n_groups)]
    pooled = [np.zeros(spec.group_width(g), bool) for g in range(spec.n_groups)]
    bad = 0
    for k, c in enumerate(spec.columns):
        sl = slice(offs[k], offs[k] + c.dim)
        dst = out[c.concat_group][:, sl]
        if c.form == FORM_PASSTHROUGH:
            if rank == 0:
                dst[:] = inputs[c.ids_input]
            continue
        table = tables[c.table_input]
        ids, kept = E.lookup_ids(c, np.asarray(inputs[c.ids_input]).ravel())
        valid = (ids >= 0) & (ids < c.vocab)
        mine = kept & valid & (ids % world == rank)
        bad += int((kept & ~valid).sum())
        if c.form == FORM_GATHER:
            dst[mine] = table[ids[mine]]
            continue
        assert c.form == FORM_SEGMENT_REDUCE
        pooled[c.concat_group][sl] = True
        w = _weights_of(c, inputs)
        o = row_offsets(c, inputs[c.seg_input], dst.shape[0])
        zero_row = np.zeros(c.dim, ft)
        for r in range(dst.shape[0]):
            lo, hi = int(o[r]), int(o[r + 1])
            acc = np.zeros(c.dim, ft)
            with np.errstate(all="ignore"):
                for i in range(lo, hi):
                    if not kept[i] or (valid[i] and not mine[i]):
                        continue                                    # dropped by the filter / another rank's row
                    x = table[ids[i]].astype(ft) if valid[i] else zero_row
                    if w is None:
                        acc = acc + x
                    elif f64:
                        acc = acc + np.float64(w[i]) * x
                    elif fused:
                        acc = (acc.astype(np.float64) + np.float64(w[i]) * x.astype(np.float64)).astype(np.float32)
                    else:
                        acc = acc + (w[i] * x).astype(np.float32)   # fl32(acc + fl32(w * x))
            if world == 1:
                if f64:
                    acc = _divide(acc, _denominator64(c, kept[lo:hi], None if w is None else w[lo:hi]))
                else:
                    acc = _divide(acc, denominator(c, kept[lo:hi], None if w is None else w[lo:hi]))
            dst[r] = acc
            if w is not None:
                kept_n[c.concat_group][r, sl] = float(kept[lo:hi].sum())
    return Restated(out, bad, kept_n, pooled)


def _denominator64(c, kept, w):
    if c.combiner == COMBINER_SUM:
        return None
    t = np.ones(int(kept.sum())) if w is None else np.asarray(w, np.float64)[kept]
    with np.errstate(all="ignore"):
        return np.float64(t.sum()) if c.combiner == COMBINER_MEAN else np.sqrt(np.float64((t * t).sum()))


def row_offsets(c: ColumnSpec, seg, rows: int) -> np.ndarray:
    seg = np.asarray(seg)
    if c.seg_kind != SEG_CSR_I32 and c.seg_stride > 1:
        seg = seg.reshape(-1, c.seg_stride)[:, 0]
    return E.row_offsets(c, seg.ravel(), rows)


def finalize_restated(spec: PlanSpec, g: int, slices: np.ndarray, inputs, rows: int) -> np.ndarray:
    """fcp_shard_finalize of group g: slices [world, rows, width] added in rank order from +0.0f, then divided by the d of
    the whole row; one-owner columns (gather, passthrough) take the OR of the slices' bits."""
    out = np.zeros(slices.shape[1:], np.float32)
    offs = spec.column_offsets()
    for k, c in enumerate(spec.columns):
        if c.concat_group != g:
            continue
        sl = slice(offs[k], offs[k] + c.dim)
        if c.form != FORM_SEGMENT_REDUCE:
            b = np.zeros(out[:, sl].shape, np.uint32)
            for wv in range(slices.shape[0]):
                b |= E.bits(slices[wv][:, sl])
            out[:, sl] = b.view(np.float32)
            continue
        _, kept = E.lookup_ids(c, np.asarray(inputs[c.ids_input]).ravel())
        w = _weights_of(c, inputs)
        o = row_offsets(c, inputs[c.seg_input], rows)
        for r in range(rows):
            acc = np.zeros(c.dim, np.float32)
            with np.errstate(all="ignore"):
                for wv in range(slices.shape[0]):
                    acc = acc + slices[wv][r, sl]
            lo, hi = int(o[r]), int(o[r + 1])
            out[r, sl] = _divide(acc, denominator(c, kept[lo:hi], None if w is None else w[lo:hi]))
    return out


def copy_mask(spec: PlanSpec, g: int) -> np.ndarray:
    return E.copy_mask(spec, g)


def nan_share(spec: PlanSpec, res: Restated) -> float:
    """Share of the pooled elements (the ones compared as "is NaN" where the expectation is NaN) that are NaN."""
    n = tot = 0
    for g in range(spec.n_groups):
        m = res.pooled[g]
        n += int(np.isnan(res.groups[g][:, m]).sum())
        tot += int(res.groups[g][:, m].size)
    return n / max(tot, 1)


def fused_share(spec: PlanSpec, tables, inputs, symbols) -> float:
    """Share of the weighted pooled elements of bags with >= 2 kept ids whose bits differ between the specified arithmetic
    and the contracted one: how well these inputs tell a fused multiply-add from a product and an add."""
    a = restate(spec, tables, inputs, symbols)
    b = restate(spec, tables, inputs, symbols, fused=True)
    diff = tot = 0
    for g in range(spec.n_groups):
        m = a.kept[g] >= 2
        diff += int((E.bits(a.groups[g])[m] != E.bits(b.groups[g])[m]).sum())
        tot += int(m.sum())
    return diff / max(tot, 1)


def float64_bound(spec: PlanSpec, tables, inputs, symbols) -> list:
    """Per group: |float32 result - float64 truth| allowed for every element, derived as
    `kernel_variant_cases.rounding_bound` derives its own (u = 2^-24, first order).  A bag of n kept ids: the numerator N
    is n rounded products and n rounded adds — every term passes through at most n + 1 roundings: |dN| <= (n + 1) u S with
    S = sum |w x| (unweighted: n u S).  The denominator d is n adds (of n rounded squares, then a square root that halves
    the relative error and adds u, for sqrtn): |dd| / |d| <= (n + 1) u K with K = sum |t| / |sum t| over its terms (1 for
    weights of one sign and for counts, which are exact).  The division adds u.  With |N| <= S:
        |d(N / d)| <= u (S / |d|) ((n + 1) + (n + 1) K + 1)  <=  (n + 2) (1 + K) u S / |d|        (SUM: (n + 2) u S).
    Copies (gather, passthrough) are exact.  Finite inputs only."""
    offs = spec.column_offsets()
    rows_g = _rows_of_groups(spec, inputs, symbols)
    out = [np.zeros((rows_g[g], spec.group_width(g))) for g in range(spec.n_groups)]
    for k, c in enumerate(spec.columns):
        if c.form != FORM_SEGMENT_REDUCE:
            continue
        sl = slice(offs[k], offs[k] + c.dim)
        ids, kept = E.lookup_ids(c, np.asarray(inputs[c.ids_input]).ravel())
        valid = (ids >= 0) & (ids < c.vocab)
        w = _weights_of(c, inputs)
        o = row_offsets(c, inputs[c.seg_input], rows_g[c.concat_group])
        tab = np.abs(tables[c.table_input].astype(np.float64))
        for r in range(rows_g[c.concat_group]):
            sel = np.arange(int(o[r]), int(o[r + 1]))
            sel = sel[kept[sel]]
            n = sel.size
            use = sel[valid[sel]]
            aw = np.ones(use.size) if w is None else np.abs(w[use].astype(np.float64))
            S = (aw[:, None] * tab[ids[use]]).sum(axis=0) if use.size else np.zeros(c.dim)
            if c.combiner == COMBINER_SUM:
                out[c.concat_group][r, sl] = (n + 2) * 2.0 ** -24 * S
                continue
            t = np.ones(n) if w is None else w[sel].astype(np.float64)
            if c.combiner == COMBINER_SQRTN:
                t = t * t
            d = t.sum() if c.combiner == COMBINER_MEAN else np.sqrt(t.sum())
            if n == 0 or d == 0:
                continue                                            # a row of +0.0: exact
            K = np.abs(t).sum() / abs(t.sum())
            out[c.concat_group][r, sl] = (n + 2) * (1 + K) * 2.0 ** -24 * S / abs(d)
    return out


# ---- plans ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    spec: PlanSpec
    tables: List[np.ndarray]
    requests: list            # [(inputs, symbols)]: the first, another shape, the first again
    weighted_kernel: bool = True
    lens_seen: frozenset = frozenset()


class _Builder:
    def __init__(self, vec: int, seed: int, flags: int = 0) -> None:
        self.vec, self.rng, self.flags = vec, np.random.default_rng(seed), flags
        self.cols, self.ranks, self.esz, self.tables, self.roles = [], [], [], [], []

    def host(self, rank: int, e: int) -> int:
        self.ranks.append(rank)
        self.esz.append(e)
        return len(self.ranks) - 1

    def table(self, vocab: int, dim: int) -> int:
        t = self.rng.standard_normal((vocab, dim)).astype(np.float32)
        t[0] = np.float32(-0.0)                                      # (row 0 of every table: -0.0)
        self.tables.append(t)
        return len(self.tables) - 1

    def pooled(self, role: str, slots: int, enc: str, vocab: int, i64: bool, share: "ColumnSpec | None" = None, **xf) -> None:
        """`share`: read that column's id, segment and weights tensors instead of tensors of its own."""
        dim = slots * self.vec
        k = len(self.cols)
        if share is not None:
            self.cols.append(dataclasses.replace(share, dim=dim, vocab=vocab, combiner=_COMBINER[role],
                                                 table_input=self.table(vocab, dim), concat_slot=k))
            self.roles.append(role)
            return
        ids = self.host(1, 8 if i64 else 4)
        if enc == "csr":
            seg, kind, stride = self.host(1, 4), SEG_CSR_I32, 1
        elif enc == "ids32":
            seg, kind, stride = self.host(1, 4), SEG_IDS_I32, 1
        else:
            seg, kind, stride = self.host(2, 8), SEG_IDS_I64, 2
        wi = self.host(1, 4) if role.startswith("w") else -1
        self.cols.append(ColumnSpec(FORM_SEGMENT_REDUCE, dim, vocab, _COMBINER[role], IDS_I64 if i64 else IDS_I32,
                                    self.table(vocab, dim), ids, seg, kind, stride, ROWS_FROM_SYMBOL, 0, None, 0, k,
                                    weights_input=wi, **xf))
        self.roles.append(role)

    def gather(self, slots: int, vocab: int) -> None:
        dim, k = slots * self.vec, len(self.cols)
        t = self.table(vocab, dim)
        self.tables[t][1] = NAN_PAYLOAD                              # rows 0 / 1: -0.0 / a NaN payload, copied bit for bit
        self.cols.append(ColumnSpec(FORM_GATHER, dim, vocab, COMBINER_NONE, IDS_I32, t, self.host(1, 4), -1, SEG_NONE, 1,
                                    ROWS_FROM_IDS, 0, None, 0, k))
        self.roles.append("gather")

    def passthrough(self, slots: int) -> None:
        dim, k = slots * self.vec, len(self.cols)
        i = self.host(2, 4)
        self.cols.append(ColumnSpec(FORM_PASSTHROUGH, dim, 0, COMBINER_NONE, IDS_I32, -1, i, -1, SEG_NONE, 1,
                                    ROWS_FROM_INPUT_DIM0, i, None, 0, k))
        self.roles.append("passthrough")

    def spec(self) -> PlanSpec:
        s = PlanSpec(self.cols, self.ranks, self.esz, len(self.tables), n_groups=1, n_symbols=1, flags=self.flags)
        s.validate()
        return s


def _segments(c: ColumnSpec, lens: np.ndarray) -> np.ndarray:
    B = lens.size
    if c.seg_kind == SEG_CSR_I32:
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = np.repeat(np.arange(B), lens)
    if c.seg_kind == SEG_IDS_I32:
        return rows.astype(np.int32)
    pos = np.concatenate([np.arange(n) for n in lens]) if lens.sum() else np.zeros(0, np.int64)
    return np.stack([rows, pos], axis=1).astype(np.int64).reshape(-1, 2)   # SparseTensor indices [nnz, 2]


def _request(b: _Builder, spec: PlanSpec, lens: dict, B: int, ids_of=None, weights_of=None):
    """Inputs of one request: `lens[k]` the bag lengths of pooled column k; ids uniform in the vocabulary unless `ids_of(k,
    c, n)` gives them; weights uniform in [0.1, 2) unless `weights_of(k, c, n)` does."""
    rng = b.rng
    inputs = [None] * spec.n_host_inputs
    for k, c in enumerate(spec.columns):
        if c.form == FORM_PASSTHROUGH:
            x = rng.standard_normal((B, c.dim)).astype(np.float32)
            x.ravel()[0::7] = np.float32(-0.0)
            x.ravel()[3::11] = NAN_PAYLOAD
            inputs[c.ids_input] = x
            continue
        dt = np.int64 if c.id_source == IDS_I64 else np.int32
        if c.form == FORM_GATHER:
            ids = rng.integers(0, c.vocab, B).astype(dt)
            ids[0::3] = 0
            ids[1::3] = 1
            inputs[c.ids_input] = ids
            continue
        n = int(lens[k].sum())
        ids = ids_of(k, c, lens[k]) if ids_of else None
        inputs[c.ids_input] = rng.integers(1, c.vocab, n).astype(dt) if ids is None else np.asarray(ids, dt)
        inputs[c.seg_input] = _segments(c, lens[k])
        if c.weights_input >= 0:
            w = weights_of(k, c, lens[k]) if weights_of else None
            inputs[c.weights_input] = rng.uniform(0.1, 2.0, n).astype(np.float32) if w is None else np.asarray(w, np.float32)
    return inputs, np.asarray([B], np.int32)


def _edge_lens(pooled: List[int], B: int, phase: int) -> dict:
    return {k: np.asarray([EDGE_LENS[(r * 5 + j * 3 + phase) % len(EDGE_LENS)] for r in range(B)], np.int64)
            for j, k in enumerate(pooled)}


# ---- item 7: V x form x segment encoding -----------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class FormCell:
    vec: int
    form: str
    enc: str

    @property
    def id(self) -> str:
        return f"V{self.vec}-{self.form}-{self.enc}"


def form_cells() -> List[FormCell]:
    return [FormCell(v, f, e) for v in VECS for f in FORMS for e in ENCODINGS]


def _form_builder(vec: int, form: str, enc: str, seed: int, flags: int = 0, **xf) -> _Builder:
    """Two spans: the cell's form four times (widths 3, 7, 49 — across the span boundary — and 11 slots) with an unweighted
    SUM, an unweighted MEAN, a GATHER and a PASSTHROUGH column between them (86 slots; odd widths: the gcd is V)."""
    b = _Builder(vec, seed, flags)
    b.pooled(form, 3, enc, 53, False, **xf)
    b.gather(5, 31)
    b.pooled(form, 7, enc, 67, True, **xf)
    b.pooled("sum", 3, enc, 41, False)
    b.pooled("mean", 5, enc, 47, True)
    b.passthrough(3)
    b.pooled(form, 49, enc, 83, False, **xf)
    b.pooled(form, 11, enc, 59, True, **xf)
    return b


def _form_lens(spec: PlanSpec, B: int, phase: int, special: bool) -> dict:
    pooled = [k for k, c in enumerate(spec.columns) if c.form == FORM_SEGMENT_REDUCE]
    lens = _edge_lens(pooled, B, phase)
    if B > 1:
        for k in pooled:
            lens[k][1] = 0                                           # an empty row
    if special:
        # span 0 holds columns 0..6 (the 49-slot one starts in it): its wave stages their bags plus the gather's one id
        span0 = [k for k in pooled if k <= 6]
        for r, total in ((2, CAPW), (3, CAPW + 1)):
            each = (total - 1) // len(span0)
            for k in span0:
                lens[k][r] = each
            lens[span0[-1]][r] = total - 1 - each * (len(span0) - 1)
        lens[pooled[0]][4] = CAPW + 1                                # one bag of 385 ids
        lens[pooled[4]][5] = 1000                                    # one bag of 1000 ids (the 49-slot column)
    return lens


@functools.lru_cache(maxsize=None)
def form_case(cell: FormCell) -> Case:
    b = _form_builder(cell.vec, cell.form, cell.enc, 7000 + 100 * cell.vec + 10 * FORMS.index(cell.form) + ENCODINGS.index(cell.enc))
    spec = b.spec()
    first = _request(b, spec, _form_lens(spec, 13, 0, True), 13)
    other = _request(b, spec, _form_lens(spec, 6, 4, False), 6)
    seen = set()
    for inputs, sym in (first, other):
        for c in spec.columns:
            if c.form == FORM_SEGMENT_REDUCE:
                seen.update(int(v) for v in np.diff(row_offsets(c, inputs[c.seg_input], int(sym[0]))))
    return Case(spec, b.tables, [first, other, first], True, frozenset(seen))


# ---- item 8: weights x id path ------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class IdPathCell:
    path: str
    form: str
    vec: int

    @property
    def id(self) -> str:
        return f"{self.path}-{self.form}-V{self.vec}"


def id_path_cells() -> List[IdPathCell]:
    out = []
    for i, path in enumerate(ID_PATHS):
        for j, form in enumerate(("wsum", "wmean", "wsqrtn")):
            out.append(IdPathCell(path, form, VECS[(i + j) % 3]))
    return out


@functools.lru_cache(maxsize=None)
def id_path_case(cell: IdPathCell) -> Case:
    """FILTER: every bag of three or more ids has a dropped id in the middle and one at the end (their weights must not
    count); SELECT: ids outside the interval become id 2; hash: raw ids of any size into 37 buckets; oov: ids outside the
    vocabulary with FCP_FLAG_COUNT_BAD_IDS (each counted once; a zero row whose weight still counts)."""
    xf = {}
    if cell.path == "filter":
        xf = dict(xform_mode=XFORM_FILTER, xform_lo=(1,), xform_hi=(30,))
    elif cell.path == "select":
        xf = dict(xform_mode=XFORM_SELECT, xform_lo=(1,), xform_hi=(30,), xform_substitute=2)
    elif cell.path == "hash":
        xf = dict(hash_buckets=37)
    enc = ENCODINGS[(ID_PATHS.index(cell.path) + cell.vec) % 3]
    b = _form_builder(cell.vec, cell.form, enc, 8000 + 10 * ID_PATHS.index(cell.path) + cell.vec,
                      FLAG_COUNT_BAD_IDS if cell.path == "oov" else 0, **xf)
    spec = b.spec()

    def ids_of(k, c, lens):
        if not (c.weights_input >= 0):
            return None
        n = int(lens.sum())
        if cell.path == "hash":
            return b.rng.integers(-2 ** 40, 2 ** 40, n) if c.id_source == IDS_I64 else b.rng.integers(-2 ** 31, 2 ** 31, n)
        ids = b.rng.integers(1, 31, n)
        start = np.concatenate([[0], np.cumsum(lens)])
        for r, L in enumerate(lens):
            if L >= 3:
                if cell.path == "oov":
                    ids[start[r] + L // 2] = (-1, c.vocab, c.vocab + 7, -5)[r % 4]
                    ids[start[r + 1] - 1] = c.vocab
                else:                                                # outside [1, 30]: dropped (FILTER) / substituted (SELECT)
                    ids[start[r] + L // 2] = 31 + r % 5
                    ids[start[r + 1] - 1] = 36
        return ids
    first = _request(b, spec, _form_lens(spec, 9, 1, True), 9, ids_of)
    other = _request(b, spec, _form_lens(spec, 5, 3, False), 5, ids_of)
    return Case(spec, b.tables, [first, other, first])


# ---- item 9: weight values ---------------------------------------------------------------------------------------------
SCENARIOS = ("zero_w", "neg_zero_w", "negative", "cancel", "all_zero", "subnormal_w", "subnormal_prod", "overflow_prod",
             "overflow_order", "inf_w", "nan_w", "ordinary")


def _scenario(name: str, rng):
    """(ids, weights) of one bag; table rows 36..39 are FLT_MAX, 1e-20, -0.0 and 1.0 (rows 2..35 standard normal)."""
    f = np.float32
    if name == "zero_w":
        return [5, 6, 7], [f(0.0), f(1.25), f(0.0)]
    if name == "neg_zero_w":
        return [5, 6], [f(-0.0), f(-0.0)]
    if name == "negative":
        return [8, 9, 10, 11, 12], [f(-1.5), f(0.75), f(-0.3), f(1.1), f(-2.0)]
    if name == "cancel":                                             # the weights sum to exactly zero, the numerator does not
        return [13, 14], [f(1.0), f(-1.0)]
    if name == "all_zero":
        return [15, 16, 17], [f(0.0), f(0.0), f(0.0)]
    if name == "subnormal_w":
        return [18, 19, 39], [f(1e-40), f(3e-41), f(2e-42)]
    if name == "subnormal_prod":
        return [37, 37, 39], [f(1e-20), f(3e-21), f(1e-39)]
    if name == "overflow_prod":                                      # a product that overflows
        return [36, 20], [f(1.5), f(1.0)]
    if name == "overflow_order":                                     # finite in exact arithmetic, +inf in id order
        return [36, 36, 36], [f(1.0), f(1.0), f(-1.0)]
    if name == "inf_w":
        return [21, 22], [f(np.inf), f(1.0)]
    if name == "nan_w":
        return [23, 24, 25], [f(1.0), f(np.nan), f(1.0)]
    n = int(rng.integers(2, 12))
    return list(rng.integers(2, 36, n)), list(rng.uniform(0.1, 2.0, n).astype(np.float32))


@functools.lru_cache(maxsize=None)
def value_case(vec: int) -> Case:
    """Weighted SUM, MEAN and SQRTN columns (3, 5 and 7 slots) reading the same ids, segments and weights; one row per
    scenario, the ordinary ones repeated so that NaN rows stay a small share."""
    b = _Builder(vec, 9000 + vec)
    for role, slots in (("wsum", 3), ("wmean", 5), ("wsqrtn", 7)):
        b.pooled(role, slots, "csr", 40, True, share=b.cols[0] if b.cols else None)
    for t in b.tables:
        t[36], t[37], t[38], t[39] = FLT_MAX, np.float32(1e-20), np.float32(-0.0), np.float32(1.0)
    spec = b.spec()

    def request(order):
        ids, ws, lens = [], [], []
        for name in order:
            i, w = _scenario(name, b.rng)
            ids += list(i)
            ws += list(w)
            lens.append(len(i))
        inputs = [None] * spec.n_host_inputs
        c = spec.columns[0]
        inputs[c.ids_input] = np.asarray(ids, np.int64)
        inputs[c.seg_input] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        inputs[c.weights_input] = np.asarray(ws, np.float32)
        return inputs, np.asarray([len(order)], np.int32)
    first = request(SCENARIOS + ("ordinary",) * 6)
    other = request(("ordinary", "cancel", "inf_w", "ordinary", "subnormal_prod", "ordinary", "ordinary"))
    return Case(spec, b.tables, [first, other, first])


# ---- item 10: row-sharded ------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class ShardCell:
    world: int
    form: str
    vec: int
    enc: str
    filtered: bool

    @property
    def id(self) -> str:
        return f"world{self.world}-{self.form}-V{self.vec}-{self.enc}{'-filter' if self.filtered else ''}"


def shard_cells() -> List[ShardCell]:
    out = []
    for i, world in enumerate(WORLDS):
        for j, form in enumerate(FORMS):
            out.append(ShardCell(world, form, VECS[(i + j) % 3], ENCODINGS[(2 * i + j) % 3], False))
    out.append(ShardCell(2, "wmean", 4, "ids32", True))
    out.append(ShardCell(3, "wsqrtn", 1, "csr", True))
    return out


@functools.lru_cache(maxsize=None)
def shard_case(cell: ShardCell) -> Case:
    xf = dict(xform_mode=XFORM_FILTER, xform_lo=(1,), xform_hi=(30,)) if cell.filtered else {}
    b = _form_builder(cell.vec, cell.form, cell.enc, 9500 + 100 * cell.world + 10 * FORMS.index(cell.form) + cell.vec, **xf)
    spec = b.spec()

    def ids_of(k, c, lens):
        if not cell.filtered or not len(c.xform_lo):
            return None
        ids = b.rng.integers(1, 31, int(lens.sum()))
        ids[2::5] = 33                                               # dropped
        return ids
    first = _request(b, spec, _form_lens(spec, 7, 2, True), 7, ids_of)
    other = _request(b, spec, _form_lens(spec, 3, 5, False), 3, ids_of)
    return Case(spec, b.tables, [first, other, first])


def all_weighted_cases():
    """(id, case) of every cell of items 7 and 8: finite inputs."""
    for cell in form_cells():
        yield cell.id, form_case(cell), cell.form != "sqrtn"
    for cell in id_path_cells():
        yield cell.id, id_path_case(cell), True
