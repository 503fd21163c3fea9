"""The matrix of fused-kernel instantiations and output store policies, as an explicit table of cells, and a
deterministic generator of small plans + requests that land in each cell (tests/test_gpu_kernel_variants.py on the GPU,
tests/test_oracle.py's cell test on the CPU).  Test data only.

A cell is (kernel, V, R, SHARDED, store policy, wide rows):
  * kernel — which fused kernel the request launches: `dense` (gathers / passthrough only), `ragged` (every 64-slot span
    holds a pooled column), `hybrid` (both kinds of span);
  * V — floats per slot, the gcd of the plan's column dims (capped at 4): dims V x {3, 5, 7, ...} slots;
  * R — rows per wave of the dense body, from the largest group's row count: < 32 -> 1, 32..63 -> 2, >= 64 -> 4;
  * SHARDED — a row-sharded plan (world 2 or 3);
  * store — `nt` (outputs below FCP_STORE_THROUGH_BYTES), `sc1_nt` (threshold 0, a ring of three arenas), `plain`
    (threshold 0, the same arena again);
  * wide rows — FCP_DIAG=wide_rows at plan creation: the dense body's 64-bit row arithmetic.

Every plan with pooled columns has sum, mean, and filtered-mean (XFORM_FILTER) columns and ids outside the vocabulary;
its bags cross the ragged kernel's fixed limits: lengths 0..17 around the walk batches (4 / 8 / 10 / 6) and the
`take <= 16` split, per-wave totals of exactly 384 (the staging tile) and 385, single bags of 384, 385 and 1000 ids,
and a span of 64 one-slot columns whose bags all outlast the first tile (a long-bag round with all 64 lanes active).
Span counts per group and kernel kind are 1, 7, 8, 9 and 17 (the XCD mapping pads lists of 8 or more to a multiple of
8), hybrid span lists are not the identity, and some plans have two groups of which the first has no ragged span."""
import dataclasses
import functools
import itertools
from typing import List, Tuple

import numpy as np

from recom_amd.plan import (COMBINER_MEAN, COMBINER_NONE, COMBINER_SUM, FLAG_COUNT_BAD_IDS, FORM_GATHER, FORM_PASSTHROUGH,
                            FORM_SEGMENT_REDUCE, IDS_I32, IDS_I64, ROWS_FROM_IDS, ROWS_FROM_INPUT_DIM0, ROWS_FROM_SYMBOL,
                            SEG_CSR_I32, SEG_IDS_I32, SEG_NONE, XFORM_FILTER, ColumnSpec, PlanSpec)

KERNELS = ("dense", "ragged", "hybrid")
VECS = (1, 2, 4)
RPWS = (1, 2, 4)
STORES = ("nt", "sc1_nt", "plain")
# row counts of the requests of a cell, per rows-per-wave value (none a multiple of the 16-row block but 32 and 64)
ROWS = {1: (1, 31), 2: (32, 63), 4: (64, 65)}
SPAN_COUNTS = (1, 7, 8, 9, 17)
EDGE_LENS = (0, 1, 4, 5, 8, 9, 10, 11, 12, 13, 14, 16, 17)    # (14: the first short tail of a walk, 10 + 4, full)
CAPW = 384                                 # ids a wave stages per round (RaggedLds::CAPW)
SPECIAL_ROWS = ("total384", "total385", "bag384", "bag385", "bag1000", "lanes64")
N_REQUESTS = 3
WAVE = 64                                  # slots per span


@dataclasses.dataclass(frozen=True)
class Cell:
    kernel: str
    vec: int
    rpw: int          # dense rows per wave (ragged cells: only chooses the row counts; the ragged body has one)
    sharded: bool
    store: str
    wide: bool

    @property
    def id(self) -> str:
        r = f"R{self.rpw}" if self.kernel != "ragged" else f"rows{self.rpw}"
        return (f"{self.kernel}-V{self.vec}-{r}-{'shard' if self.sharded else 'one'}-{self.store}"
                f"{'-wide' if self.wide else ''}")

    @property
    def key(self) -> Tuple[str, int, int, int]:
        """What the plan and its requests depend on: (kernel, V, R, variant) — the same for a cell's sharded / unsharded
        and wide / default twins."""
        return (self.kernel, self.vec, self.rpw, (3 * RPWS.index(self.rpw) + STORES.index(self.store) + VECS.index(self.vec)) % 5)


def cells() -> List[Cell]:
    """Every (kernel, V, R, SHARDED, store, wide rows) cell: the 42 instantiations x 3 store policies, the dense and
    hybrid ones also with wide rows.  (Ragged cells vary the row counts in R's place.)"""
    out = []
    for kernel, vec, rpw, sharded, store in itertools.product(KERNELS, VECS, RPWS, (False, True), STORES):
        if kernel == "ragged" and rpw != RPWS[STORES.index(store)]:
            continue                       # ragged: one row count pair per store policy
        for wide in ((False, True) if kernel != "ragged" else (False,)):
            out.append(Cell(kernel, vec, rpw, sharded, store, wide))
    return out


def instantiation(cell: Cell) -> Tuple[str, int, int, bool]:
    """The kernel template a cell runs: (kernel, V, R, SHARDED) — R is 0 for the ragged kernel."""
    return (cell.kernel, cell.vec, cell.rpw if cell.kernel != "ragged" else 0, cell.sharded)


# ---- plan layout --------------------------------------------------------------------------------------------------------
# column widths in slots, cycled through a run of spans of one kind (sums to 64 per pattern except the straddling pair
# 100 + 28, one column across a span boundary); 3 / 5 / 7 make the dims' gcd exactly V
_SLOT_CYCLE = (3, 5, 7, 49, 64, 16, 16, 16, 16, 13, 11, 9, 31, 100, 28)


def _run_slots(nspans: int, start: int, lanes64: bool, short_tail: int) -> List[int]:
    """Column widths (slots) filling `nspans` spans, starting at position `start` of the cycle; `lanes64`: the first span
    is 64 one-slot columns; `short_tail`: the last span is that many slots short of 64 (a partial last span)."""
    total = WAVE * nspans - (0 if lanes64 and nspans == 1 else short_tail)
    out = [1] * WAVE if lanes64 else []
    cyc = itertools.cycle(_SLOT_CYCLE[start % len(_SLOT_CYCLE):] + _SLOT_CYCLE[:start % len(_SLOT_CYCLE)])
    while sum(out) < total:
        out.append(min(next(cyc), total - sum(out)))
    if not any(s % 2 for s in out):
        out[-1] -= 1                       # (keep an odd width somewhere: the gcd is V, not 2V)
        out.append(1)
    return out


def _layout(kernel: str, variant: int):
    """Per group: a list of runs (kind, nspans, lanes64, short_tail); kind 0 dense, 1 ragged."""
    n = SPAN_COUNTS[variant]
    m = SPAN_COUNTS[(variant + 2) % 5]
    tail = (0, 21, 0, 40, 7)[variant]
    if kernel == "dense":
        if variant % 2:
            return [[(0, n, False, tail)], [(0, m, False, 0)]]
        return [[(0, n, False, tail)]]
    if kernel == "ragged":
        if variant % 2:
            return [[(1, n, variant == 3, tail)], [(1, m, False, 0)]]
        return [[(1, n, variant in (0, 4), tail)]]
    # hybrid: spans of the two kinds interleaved (neither list is the identity); odd variants put a dense-only group first
    nd, nr = n, (17, 9, 8, 7, 1)[variant]
    runs, k = [], 0
    while nd or nr:
        if nd and (k % 2 == 0 or not nr):
            runs.append((0, 1, False, 0))
            nd -= 1
        elif nr:
            runs.append((1, 1, k == 1, 0))
            nr -= 1
        k += 1
    runs[-1] = runs[-1][:3] + (tail,)
    return [[(0, m, False, 0)], runs] if variant % 2 else [runs]


@dataclasses.dataclass
class Case:
    spec: PlanSpec
    tables: List[np.ndarray]
    requests: list          # [(inputs, symbols)]
    abs_requests: list      # the same with every float payload replaced by its magnitude
    span_counts: list       # per group: [spans of the dense kind, spans of the ragged kind]
    bag_max: list           # per request, per group: float64[width], the longest bag of the column (-1: not pooled)


@functools.lru_cache(maxsize=None)
def build_case(kernel: str, vec: int, rpw: int, variant: int) -> Case:
    rng = np.random.default_rng(KERNELS.index(kernel) * 1000 + vec * 100 + rpw * 10 + variant)
    groups = _layout(kernel, variant)
    cols, ranks, esz, tables = [], [], [], []
    col_info = []           # per column: group, kind (0 dense, 1 ragged), role, first slot in the group, slots, vocab

    def host(rank, e):
        ranks.append(rank)
        esz.append(e)
        return len(ranks) - 1

    n_pool = 0
    for g, runs in enumerate(groups):
        slot = 0
        for ri, (kind, nspans, lanes64, tail) in enumerate(runs):
            widths = _run_slots(nspans, 3 * ri + 5 * g + variant, lanes64, tail)
            for w in widths:
                dim = w * vec
                if kind == 0:
                    role = ("gather", "passthrough", "gather_filter")[len(cols) % 3]
                else:
                    role = ("sum", "mean", "mean_filter")[n_pool % 3]
                    n_pool += 1
                vocab = int(rng.integers(23, 90))
                k = len(cols)
                if role == "passthrough":
                    i = host(2, 4)
                    cols.append(ColumnSpec(FORM_PASSTHROUGH, dim, 0, COMBINER_NONE, IDS_I32, -1, i, -1, SEG_NONE, 1,
                                           ROWS_FROM_INPUT_DIM0, i, None, g, k))
                else:
                    tables.append(rng.standard_normal((vocab, dim)).astype(np.float32))
                    t = len(tables) - 1
                    src = IDS_I64 if k % 2 else IDS_I32
                    i = host(1, 8 if src == IDS_I64 else 4)
                    xf = {}
                    if role.endswith("_filter"):    # drops ids above 2/3 of the vocabulary, and the negative ones
                        xf = dict(xform_mode=XFORM_FILTER, xform_lo=(0,), xform_hi=(2 * vocab // 3,))
                    if kind == 0:
                        cols.append(ColumnSpec(FORM_GATHER, dim, vocab, COMBINER_NONE, src, t, i, -1, SEG_NONE, 1,
                                               ROWS_FROM_IDS, 0, None, g, k, **xf))
                    else:
                        csr = k % 2 == 0
                        si = host(1, 4)
                        comb = COMBINER_SUM if role == "sum" else COMBINER_MEAN
                        cols.append(ColumnSpec(FORM_SEGMENT_REDUCE, dim, vocab, comb, src, t, i, si,
                                               SEG_CSR_I32 if csr else SEG_IDS_I32, 1, ROWS_FROM_SYMBOL, g, None, g, k, **xf))
                col_info.append(dict(group=g, kind=kind, role=role, slot=slot, slots=w, vocab=vocab))
                slot += w
    # concat slots are numbered per group in column order
    nxt = [0] * len(groups)
    for c in cols:
        c.concat_slot = nxt[c.concat_group]
        nxt[c.concat_group] += 1
    spec = PlanSpec(cols, ranks, esz, len(tables), n_groups=len(groups), n_symbols=len(groups), flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    span_counts = []
    for g in range(len(groups)):
        nslots = sum(ci["slots"] for ci in col_info if ci["group"] == g)
        ragged = set()
        for ci in col_info:
            if ci["group"] == g and ci["kind"] == 1:
                ragged.update(range(ci["slot"] // WAVE, (ci["slot"] + ci["slots"] - 1) // WAVE + 1))
        nspans = (nslots + WAVE - 1) // WAVE
        span_counts.append([nspans - len(ragged), len(ragged)])

    requests, abs_requests, bag_max = [], [], []
    for t in range(N_REQUESTS):
        r0 = ROWS[rpw][t % 2]
        batches = [r0] + [max(1, r0 - r0 // 3)] * (len(groups) - 1)
        inputs, abs_inputs, bm = _request(rng, spec, col_info, groups, batches, t + variant)
        requests.append((inputs, np.asarray(batches, np.int32)))
        abs_requests.append((abs_inputs, np.asarray(batches, np.int32)))
        bag_max.append(bm)
    return Case(spec, tables, requests, abs_requests, span_counts, bag_max)


def _bag_lengths(col_info, g, B, phase) -> dict:
    """Bag lengths [B] of every pooled column of group g: the edge lengths, and special rows."""
    pooled = [k for k, ci in enumerate(col_info) if ci["group"] == g and ci["kind"] == 1]
    lens = {k: np.asarray([EDGE_LENS[(r * 7 + j * 3 + phase) % len(EDGE_LENS)] for r in range(B)], np.int64)
            for j, k in enumerate(pooled)}
    if not pooled:
        return lens
    # spans of the group (by first slot): the pooled columns whose first slot lies in each
    by_span = {}
    for k in pooled:
        by_span.setdefault(col_info[k]["slot"] // WAVE, []).append(k)
    lanes64 = [ks for ks in by_span.values() if len(ks) == WAVE and all(col_info[k]["slots"] == 1 for k in ks)]
    for r in range(B):
        if (r + phase) % 4 and B > 1:
            continue
        kind = SPECIAL_ROWS[(r // 4 + phase) % len(SPECIAL_ROWS)]
        if kind in ("total384", "total385"):
            total = CAPW + (kind == "total385")
            for ks in by_span.values():     # the ids of the span's columns in this row add up to `total`
                each = total // len(ks)
                for k in ks:
                    lens[k][r] = each
                lens[ks[-1]][r] = total - each * (len(ks) - 1)
        elif kind.startswith("bag"):
            k = pooled[(r + phase) % len(pooled)]
            lens[k][r] = int(kind[3:])
        elif lanes64:
            ks = lanes64[0]                 # lane 0 fills the tile, every other lane keeps all its ids: 64 active bags
            lens[ks[0]][r] = CAPW + 1
            for j, k in enumerate(ks[1:]):
                lens[k][r] = EDGE_LENS[1 + (j + r) % (len(EDGE_LENS) - 1)]
    return lens


def _request(rng, spec, col_info, groups, batches, phase):
    lens = {}
    for g in range(len(groups)):
        lens.update(_bag_lengths(col_info, g, batches[g], phase))
    inputs, abs_inputs = [], []
    widths = [spec.group_width(g) for g in range(spec.n_groups)]
    offs = spec.column_offsets()
    bm = [np.full(widths[g], -1.0) for g in range(spec.n_groups)]
    for k, (c, ci) in enumerate(zip(spec.columns, col_info)):
        B = batches[c.concat_group]
        if c.form == FORM_PASSTHROUGH:
            x = rng.standard_normal((B, c.dim)).astype(np.float32)
            inputs.append(x)
            abs_inputs.append(np.abs(x))
            continue
        dt = np.int64 if c.id_source == IDS_I64 else np.int32
        n = B if c.form == FORM_GATHER else int(lens[k].sum())
        ids = rng.integers(0, c.vocab, n).astype(dt)
        if n:                               # ids outside the vocabulary (the filter drops some of them first)
            bad = rng.random(n) < 0.04
            ids[bad] = rng.choice(np.asarray([-1, -9, c.vocab, c.vocab + 5, np.iinfo(np.int32).max], dt), int(bad.sum()))
        inputs.append(ids)
        abs_inputs.append(ids)
        if c.form == FORM_SEGMENT_REDUCE:
            if c.seg_kind == SEG_CSR_I32:
                seg = np.concatenate([[0], np.cumsum(lens[k])]).astype(np.int32)
            else:
                seg = np.repeat(np.arange(B, dtype=np.int32), lens[k])
            inputs.append(seg)
            abs_inputs.append(seg)
            bm[c.concat_group][offs[k]:offs[k] + c.dim] = float(lens[k].max()) if B else 0.0
    return inputs, abs_inputs, bm


def rounding_bound(bag_max: np.ndarray, magnitude: np.ndarray) -> np.ndarray:
    """|fp32 result - float64 truth| of a pooled element: n sequential fp32 adds and a division, each off by at most
    2^-24 of the running magnitude, so (n + 2) * 2^-24 * S with S = the sum of |x| of the bag (divided by the count for
    a mean).  Not-pooled elements (bag_max < 0) are copies: exact."""
    return np.where(bag_max < 0, 0.0, (np.maximum(bag_max, 0) + 2) * 2.0 ** -24 * magnitude)


def expected_blocks(span_counts, rows, rpw: int) -> Tuple[int, int]:
    """(dense, ragged) grid blocks: per group, the listed spans — a list of 8 or more padded to a multiple of 8 (the XCD
    mapping's idle blocks) — times the row tiles of 4 waves x rows per wave (the ragged body: 1)."""
    out = []
    for kind, r in ((0, rpw), (1, 1)):
        blocks = 0
        for g, counts in enumerate(span_counts):
            n = counts[kind]
            if n:
                blocks += (8 * ((n + 7) // 8) if n >= 8 else n) * ((int(rows[g]) + 4 * r - 1) // (4 * r))
        out.append(blocks)
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def float64_reference(key, t: int):
    """(float64 truth, its rounding bound) per group of request t of the case `key` (unsharded plan)."""
    import fcp_oracle
    from recom_amd.ops import concat_inputs
    case = build_case(*key)
    plan = case.spec.to_dict()
    inputs, symbols = case.requests[t]
    blob, offsets, shapes = concat_inputs(inputs)
    truth = fcp_oracle.np_process_feature_columns(plan, blob, offsets, shapes, case.tables, symbols)
    ablob, aoffsets, ashapes = concat_inputs(case.abs_requests[t][0])
    mag = fcp_oracle.np_process_feature_columns(plan, ablob, aoffsets, ashapes, [np.abs(x) for x in case.tables], symbols)
    return truth, [rounding_bound(case.bag_max[t][g][None, :], m) for g, m in enumerate(mag)]


def check_against_float64(got_groups, key, t: int, what) -> None:
    """Every group of a request's fp32 result within the rounding bound of the float64 truth (copies exact)."""
    truth, bound = float64_reference(key, t)
    for g, (got, want, b) in enumerate(zip(got_groups, truth, bound)):
        assert got.shape == want.shape, (what, g)
        err = np.abs(got.astype(np.float64) - want)
        bad = ~(err <= b)                     # (NaN fails)
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"{what} group {g}: {int(bad.sum())} elements outside the float64 bound, first [{r}, {c}] "
                                 f"got {got[r, c]!r} want {want[r, c]!r} bound {b[r, c]!r}")
