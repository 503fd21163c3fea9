"""The fused kernels at their edge VALUES, as explicit cells (tests/test_gpu_value_edges.py on the GPU, tests/test_oracle.py
on the CPU): what decides a result inside the kernels per element, where tests/kernel_variant_cases.py pins shapes.  Test
data only.  Three families:

  * id-path cells (`id_cells`) — hash, id transform, vocabulary check and row-shard split as the four readers of the id
    path evaluate them.  Every cell's plan holds all four: a one-hot gather in a span of its own (the dense body), a sum
    over CSR and a mean over segment ids (the ragged body), a ScatterNd column over row ids in any order (the pre-pass
    when the cell's transform is a filter), and — sharded cells — the finalize's kept count of the filtered mean.  Hashed
    columns read the identity table (row r = float(r)), so the output is the bucket; unhashed ones read row r =
    dim * r + 1 .. dim * r + dim;
  * sharded ids at and beyond 2^31 and 2^32 (`big_case`) — a table of 2^32 + 2^16 rows over three ranks, with decoy rows
    where a truncated or 32-bit split would read;
  * pooled specials (`special_cells`) — bags built so that the sums and means meet +-inf, inf - inf, NaN rows, overflow in
    id order, subnormal sums and quotients, -0.0 and the zero line.

Expected values are restated here in NumPy (`restate`): float32 adds one by one in id order from +0.0, the division in
float32; row-sharded: each rank's partial sums, then `aux_kernel_cases.finalize_restated` (rank order, then the division).
The comparison rule (`assert_same`): bit patterns equal wherever the expected value is not NaN; where it is NaN the result
must be NaN — a NaN's sign and payload after an add or a division are the hardware's (the host's SSE and the GPU's VALU
choose differently among several NaN operands), the one thing here that cannot be equal by design.  Copies (gather,
ScatterNd, passthrough) keep NaN payloads bit for bit and are compared so."""
import dataclasses
import functools
from typing import List

import numpy as np

import kernel_variant_cases as K
from recom_amd.plan import (COMBINER_MEAN, COMBINER_NONE, COMBINER_SUM, FLAG_COUNT_BAD_IDS, FORM_GATHER, FORM_GATHER_SCATTER,
                            FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE, IDS_F32_BUCKETIZE, IDS_I32, IDS_I64, ROWS_FROM_IDS,
                            ROWS_FROM_INPUT_DIM0, ROWS_FROM_SYMBOL, SEG_CSR_I32, SEG_IDS_I32, SEG_NONE, XFORM_FILTER,
                            XFORM_NONE, XFORM_SELECT, ColumnSpec, PlanSpec)

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
N_REQUESTS = 3            # the first installs descriptors, then a different one, then the first again


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what, copies=None) -> None:
    """Bit patterns equal where `want` is not NaN; NaN where it is (in columns of `copies` — a bool mask over the width —
    NaNs are compared bit for bit as well)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    if copies is not None:
        nan = nan & ~np.asarray(copies, bool)[None, :]
    diff = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    if diff.any():
        r, c = (int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} elements differ, first [{r}, {c}] got {got[r, c]!r} "
                             f"({bits(got)[r, c]:#010x}) want {want[r, c]!r} ({bits(want)[r, c]:#010x})")


# ---- the restatement --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fp(v: int) -> int:
    import fcp_oracle
    return fcp_oracle.np_fingerprint64(str(v).encode())


def lookup_ids(c: ColumnSpec, raw: np.ndarray):
    """(id the lookup sees [int64], kept by the filter [bool]) of a column's raw ids: bucketize or the integer itself, the
    hash, then the interval test — closed intervals, any of them — which substitutes (SELECT) or drops (FILTER)."""
    import fcp_oracle
    if c.id_source == IDS_F32_BUCKETIZE:
        ids = fcp_oracle.np_bucketize(c.boundaries, raw).astype(np.int64)
    else:
        ids = np.asarray(raw).astype(np.int64)
    if c.hash_buckets:
        ids = np.asarray([_fp(int(v)) % c.hash_buckets for v in ids], np.int64).reshape(ids.shape)
    kept = np.ones(ids.size, bool)
    if c.xform_mode != XFORM_NONE:
        inside = np.zeros(ids.size, bool)
        for lo, hi in zip(c.xform_lo, c.xform_hi):
            inside |= (ids >= np.int64(lo)) & (ids <= np.int64(hi))
        if c.xform_mode == XFORM_SELECT:
            ids = np.where(inside, ids, np.int64(c.xform_substitute))
        else:
            kept = inside
    return ids, kept


def row_offsets(c: ColumnSpec, seg: np.ndarray, rows: int) -> np.ndarray:
    if c.seg_kind == SEG_CSR_I32:
        return np.asarray(seg, np.int64)
    return np.searchsorted(np.asarray(seg, np.int64), np.arange(rows + 1), side="left")


def restate(spec: PlanSpec, tables, inputs, symbols, rank: int = 0, world: int = 1):
    """(per group float32 [rows, width], bad ids) of one request, for the forms these cases use.  `tables` are the GLOBAL
    tables; a rank of a row-sharded plan adds the rows it owns (id % world == rank) and divides nothing; every rank counts
    every id that reached the lookup and is outside the vocabulary."""
    offs = spec.column_offsets()
    rows_g = {}
    for c in spec.columns:
        if c.rows_source == ROWS_FROM_SYMBOL:
            rows_g[c.concat_group] = int(symbols[c.rows_arg])
        elif c.form == FORM_GATHER:
            rows_g[c.concat_group] = int(np.asarray(inputs[c.ids_input]).size)
        elif c.form == FORM_PASSTHROUGH:
            rows_g[c.concat_group] = int(inputs[c.ids_input].shape[0])
    out = [np.zeros((rows_g[g], spec.group_width(g)), np.float32) for g in range(spec.n_groups)]
    bad = 0
    for k, c in enumerate(spec.columns):
        dst = out[c.concat_group][:, offs[k]:offs[k] + c.dim]
        if c.form == FORM_PASSTHROUGH:
            if rank == 0:
                dst[:] = inputs[c.ids_input]
            continue
        table = tables[c.table_input]
        ids, kept = lookup_ids(c, np.asarray(inputs[c.ids_input]).ravel())
        valid = (ids >= 0) & (ids < c.vocab)
        mine = kept & valid & (ids % world == rank)
        B = dst.shape[0]
        if c.form == FORM_GATHER:
            bad += int((kept & ~valid).sum())
            dst[mine] = table[ids[mine]]
        elif c.form == FORM_SEGMENT_REDUCE:
            bad += int((kept & ~valid).sum())
            o = row_offsets(c, inputs[c.seg_input], B)
            for r in range(B):
                acc = np.zeros(c.dim, np.float32)
                n = int(kept[o[r]:o[r + 1]].sum())
                with np.errstate(all="ignore"):         # (overflow and inf - inf are among the cases)
                    for i in range(int(o[r]), int(o[r + 1])):
                        if mine[i]:
                            acc = acc + table[ids[i]]
                    if c.combiner == COMBINER_MEAN and world == 1 and n > 0:
                        acc = acc / np.float32(n)
                dst[r] = acc
        else:   # ScatterNd over row ids in any order: a sequential scatter of what the filter kept; the last write wins
            seg = np.asarray(inputs[c.seg_input]).ravel()
            winner = {}
            for i in range(ids.size):
                if not kept[i]:
                    continue
                if 0 <= seg[i] < B:
                    winner[int(seg[i])] = i
                else:
                    bad += 1
            for r, i in winner.items():
                bad += int(not valid[i])
                if mine[i]:
                    dst[r] = table[ids[i]]
    return out, bad


def copy_mask(spec: PlanSpec, g: int) -> np.ndarray:
    """Elements of group g that are copies of one table row or payload (NaNs compared bit for bit)."""
    m = np.zeros(spec.group_width(g), bool)
    offs = spec.column_offsets()
    for k, c in enumerate(spec.columns):
        if c.concat_group == g and c.form != FORM_SEGMENT_REDUCE:
            m[offs[k]:offs[k] + c.dim] = True
    return m


def finalized(spec: PlanSpec, g: int, slices: np.ndarray, inputs, rows: int) -> np.ndarray:
    """Group g's slices [world, rows, width] through `aux_kernel_cases.finalize_restated`: rank-order adds, then the means'
    division by their kept counts; one-owner columns take the owner's bits."""
    import aux_kernel_cases as A
    with np.errstate(all="ignore"):
        return A.finalize_restated(group_view(spec, g), slices, kept_of_group(spec, g, inputs, rows))


def group_view(spec: PlanSpec, g: int) -> PlanSpec:
    """The columns of group g alone, for `aux_kernel_cases.finalize_restated` (which takes one group's matrix)."""
    return dataclasses.replace(spec, columns=[c for c in spec.columns if c.concat_group == g])


def kept_of_group(spec: PlanSpec, g: int, inputs, rows: int) -> dict:
    """{index in group_view(spec, g).columns: ids per row a mean divides by}"""
    out = {}
    for j, c in enumerate(group_view(spec, g).columns):
        if c.form == FORM_SEGMENT_REDUCE and c.combiner == COMBINER_MEAN:
            _, kept = lookup_ids(c, np.asarray(inputs[c.ids_input]).ravel())
            o = row_offsets(c, inputs[c.seg_input], rows)
            cs = np.concatenate([[0], np.cumsum(kept)])
            out[j] = (cs[o[1:]] - cs[o[:-1]]).astype(np.int64)
    return out


# ---- A1: id-path cells ------------------------------------------------------------------------------------------------
HASHES = (0, 1, 2, 997, 1 << 24)
MODES = ("none", "select", "filter")
INTERVALS = ("empty", "one", "adjacent", "overlap", "last_of_5", "min_x", "x_max", "all")
SUBSTITUTES = ("m1", "zero", "vm1", "v", "min", "max")
SOURCES = ("i64", "i32", "bkt")
WORLDS = (1, 2, 3)
UNHASHED_VOCAB = 10
BOUNDARIES = np.arange(UNHASHED_VOCAB - 1, dtype=np.float32)          # buckets 0..9
HASH_LEN_EDGES = {"i64": (1, 3, 4, 7, 8, 16, 17, 20), "i32": (1, 3, 4, 7, 8, 11)}   # both ends of every length branch
_MODE = {"none": XFORM_NONE, "select": XFORM_SELECT, "filter": XFORM_FILTER}


@dataclasses.dataclass(frozen=True)
class IdCell:
    src: str
    hash: int
    mode: str
    ivals: str
    sub: str
    world: int      # 1: unsharded; 2 / 3: every rank runs (rank 0 and the last one included), then the finalize
    dim: int

    @property
    def id(self) -> str:
        return f"{self.src}-h{self.hash}-{self.mode}-{self.ivals}-sub_{self.sub}-w{self.world}-d{self.dim}"

    @property
    def vocab(self) -> int:
        """Hashed columns: one row per bucket — but 900 rows for 997 buckets, so that the vocabulary check still has
        something to refuse behind the hash."""
        return UNHASHED_VOCAB if not self.hash else 900 if self.hash == 997 else self.hash

    @property
    def x(self) -> int:
        return self.vocab // 2

    def intervals(self):
        v, x = self.vocab, self.x
        return {"empty": (), "one": ((min(2, x), x),), "adjacent": ((0, x), (x + 1, max(v - 1, x + 1))),
                "overlap": ((0, x + 1), (x, v + 1)),
                "last_of_5": ((-9, -7), (v + 3, v + 4), (I64_MAX - 1, I64_MAX), (-5, -5), (min(1, v - 1), v)),
                "min_x": ((I64_MIN, x),), "x_max": ((x, I64_MAX),), "all": ((I64_MIN, I64_MAX),)}[self.ivals]

    def substitute(self) -> int:
        return {"m1": -1, "zero": 0, "vm1": self.vocab - 1, "v": self.vocab, "min": I64_MIN, "max": I64_MAX}[self.sub]


def id_cells() -> List[IdCell]:
    """Every (hash x mode) pair twice (the other id source, another world), every interval list under SELECT and under
    FILTER, every substitute, the two transforms behind Bucketize, and the INT64_MIN collisions by name: every value of
    every axis, with every reader (all four are in every cell's plan)."""
    out, j = [], 0

    def add(src, h, mode, ivals, sub, world):
        nonlocal j
        if mode == "none":
            ivals, sub = "empty", "zero"
        dim = 1 if h == 1 << 24 else (2, 1, 4)[j % 3]
        out.append(IdCell(src, h, mode, ivals, sub, world, dim))
        j += 1
    for rep in range(2):
        for h in HASHES:
            for mode in MODES:
                add(SOURCES[(j + rep) % 2], h, mode, INTERVALS[(j + 3 * rep) % 8], SUBSTITUTES[j % 6], WORLDS[(j + rep) % 3])
    for ivals in INTERVALS:
        for mode in ("select", "filter"):
            add(SOURCES[j % 2], 0, mode, ivals, SUBSTITUTES[(j + 2) % 6], WORLDS[j % 3])
    for sub in SUBSTITUTES:
        add("i64", (0, 997)[j % 2], "select", ("one", "min_x", "last_of_5")[j % 3], sub, WORLDS[j % 3])
    add("bkt", 0, "select", "one", "v", 1)
    add("bkt", 0, "filter", "adjacent", "zero", 2)
    # the collisions of a reserved "dropped" id with a legal one, unsharded and sharded
    for world in WORLDS:
        add("i64", 0, "filter", "min_x", "zero", world)
        add("i64", 0, "select", "one", "min", world)
        add("i64", 0, "select", "min_x", "m1", world)
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


def _hashed_ids(src: str) -> np.ndarray:
    """Ids whose decimal strings have every length the type can have, four per length and sign, and the digit-count edges
    10^k - 1, 10^k, 10^k + 1 in both signs, the types' extremes, 2^31 and 2^32."""
    rng = np.random.default_rng(20 + (src == "i32"))
    lo, hi = (I32_MIN, I32_MAX) if src == "i32" else (I64_MIN, I64_MAX)
    vals = [0, -1, I32_MIN, I32_MAX, lo, hi]
    if src == "i64":
        vals += [1 << 31, 1 << 32, -(1 << 31) - 1, -(1 << 32)]
    for k in range(19):
        for s in (1, -1):
            vals += [s * (10 ** k - 1), s * 10 ** k, s * (10 ** k + 1)]
            a, b = 10 ** k, min(10 ** (k + 1) - 1, hi)
            if a <= b:
                vals += [s * int(v) for v in rng.integers(a, b, 4, endpoint=True)]
    vals = [v for v in vals if lo <= v <= hi]
    return np.asarray(list(dict.fromkeys(vals)), np.int64)


def _unhashed_ids(cell: IdCell) -> np.ndarray:
    v = cell.vocab
    lo, hi = (I32_MIN, I32_MAX) if cell.src == "i32" else (I64_MIN, I64_MAX)
    vals = [0, 1, v - 1, v, -1, 3, 7, I32_MIN, I32_MAX, lo, hi, lo + 1, hi - 1, cell.substitute()]
    if cell.src == "i64":
        vals += [1 << 31, 1 << 32, (1 << 32) + 3]
    for a, b in cell.intervals():
        vals += [a - 1, a, a + 1, b - 1, b, b + 1]
    vals = [int(x) for x in vals if lo <= x <= hi]
    return np.asarray(list(dict.fromkeys(vals)) + [3, 7, 3], np.int64)


@functools.lru_cache(maxsize=8)
def _id_table(vocab: int, dim: int, identity: bool) -> np.ndarray:
    r = np.arange(vocab, dtype=np.float32)[:, None]
    if identity:
        return np.ascontiguousarray(np.broadcast_to(r, (vocab, dim)))
    return dim * r + np.arange(1, dim + 1, dtype=np.float32)[None, :]


@dataclasses.dataclass
class Case:
    spec: PlanSpec
    tables: list            # global tables (a rank's: t[rank::world])
    requests: list          # [(inputs, symbols)]


def _spread(n: int, pattern) -> np.ndarray:
    """Bag lengths of n rows holding n ids: the pattern repeated, cut where the ids run out."""
    lens = np.resize(np.asarray(pattern, np.int64), n)
    ends = np.minimum(np.cumsum(lens), n)
    ends[-1] = n
    return np.diff(np.concatenate([[0], ends]))


def _id_request(cell: IdCell, ids: np.ndarray, t: int):
    n = ids.size
    rng = np.random.default_rng(100 + t)
    dt = {"i64": np.int64, "i32": np.int32, "bkt": np.float32}[cell.src]
    a = ids.astype(dt)
    lens_sum = _spread(n, (1, 2, 0, 1, 3, 0, 1, 0, 1, 1))
    lens_mean = _spread(n, (2, 1, 1, 0, 2, 0, 1, 3, 0, 0))
    rows = rng.permutation(n).astype(np.int32)
    rows[5::7] = rows[4::7][:rows[5::7].size]          # two writes to one row: the later id wins (if the filter keeps it)
    if n > 12:
        rows[3], rows[11] = -1, n                      # rows ScatterNd drops
    inputs = [a, a.copy(), np.concatenate([[0], np.cumsum(lens_sum)]).astype(np.int32),
              a[::-1].copy(), np.repeat(np.arange(n, dtype=np.int32), lens_mean),
              np.roll(a, 5), rows]
    return inputs, np.asarray([n], np.int32)


@functools.lru_cache(maxsize=4)
def id_case(cell: IdCell) -> Case:
    v, d = cell.vocab, cell.dim
    xf = dict(xform_mode=_MODE[cell.mode], hash_buckets=cell.hash)
    if cell.mode != "none":
        iv = cell.intervals()
        xf.update(xform_lo=tuple(a for a, _ in iv), xform_hi=tuple(b for _, b in iv), xform_substitute=cell.substitute())
    src = {"i64": IDS_I64, "i32": IDS_I32, "bkt": IDS_F32_BUCKETIZE}[cell.src]
    bnd = BOUNDARIES if cell.src == "bkt" else None
    e = 8 if cell.src == "i64" else 4
    cols = [ColumnSpec(FORM_GATHER, d, v, COMBINER_NONE, src, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, bnd, 0, 0, **xf),
            ColumnSpec(FORM_SEGMENT_REDUCE, d, v, COMBINER_SUM, src, 0, 1, 2, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, bnd, 1, 0, **xf),
            ColumnSpec(FORM_SEGMENT_REDUCE, d, v, COMBINER_MEAN, src, 0, 3, 4, SEG_IDS_I32, 1, ROWS_FROM_SYMBOL, 0, bnd, 1, 1, **xf),
            ColumnSpec(FORM_GATHER_SCATTER, d, v, COMBINER_NONE, src, 0, 5, 6, SEG_IDS_I32, 1, ROWS_FROM_SYMBOL, 0, bnd, 1, 2, **xf)]
    spec = PlanSpec(cols, [1] * 7, [e, e, 4, e, 4, e, 4], 1, n_groups=2, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    if cell.src == "bkt":
        ids = np.asarray([-1.0, -0.0, 0.0, 0.5, 1.0, 3.999, 4.0, 7.0, 7.5, 8.0, 8.5, 100.0, np.inf, -np.inf, 2.5, 6.0, 5.0, 1.5],
                         np.float32)
    else:
        ids = _hashed_ids(cell.src) if cell.hash else _unhashed_ids(cell)
    first = _id_request(cell, ids, 0)
    requests = [first, _id_request(cell, np.roll(ids[::-1], 3)[:max(ids.size - 2, 1)], 1), first]
    return Case(spec, [_id_table(v, d, bool(cell.hash))], requests)


def min_collision_case():
    """The request of the first INT64_MIN collision, by hand: vocab 10, row r = [2r+1, 2r+2], one mean column over CSR, bags
    [INT64_MIN, 3] and [7, 3], FILTER [INT64_MIN, 5].  INT64_MIN is inside the interval: it reaches the lookup, reads zeros,
    counts in the mean and as a bad id -> row 0 = [3.5, 4.0], bad == 1; 7 is dropped -> row 1 = [7.0, 8.0]."""
    col = ColumnSpec(FORM_SEGMENT_REDUCE, 2, 10, COMBINER_MEAN, IDS_I64, 0, 0, 1, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 0, 0,
                     xform_mode=XFORM_FILTER, xform_lo=(I64_MIN,), xform_hi=(5,))
    spec = PlanSpec([col], [1, 1], [8, 4], 1, n_groups=1, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    inputs = [np.asarray([I64_MIN, 3, 7, 3], np.int64), np.asarray([0, 2, 4], np.int32)]
    want = np.asarray([[3.5, 4.0], [7.0, 8.0]], np.float32)
    return spec, [_id_table(10, 2, False)], inputs, np.asarray([2], np.int32), want, 1


# ---- A2: sharded ids at and beyond 2^31 and 2^32 ----------------------------------------------------------------------
BIG_VOCAB = (1 << 32) + (1 << 16)
BIG_WORLD = 3


def big_rows(rank: int) -> int:
    return (BIG_VOCAB - rank + BIG_WORLD - 1) // BIG_WORLD


@functools.lru_cache(maxsize=1)
def big_case():
    """One plan (a gather column and a pooled sum over one table of BIG_VOCAB rows x 1 float, world 3), its requests, and
    per rank the rows to write into the zero-filled table: `true` {local row: value} of the ids the rank owns and `decoy`
    {local row: value} where a wrong split of some id would read — (id mod 2^32) / world (a truncated id, which is also
    the 32-bit division) and id / world +- 1.  Values are k + 0.5 for small k (true, positive; decoys, negative): distinct,
    and their sums exact in float32 in any order."""
    rng = np.random.default_rng(77)
    W, V = BIG_WORLD, BIG_VOCAB
    around = [(1 << 31) + d for d in range(-2, 3)] + [(1 << 32) + d for d in range(-2, 3)] + [V - 1, V, V + 1, -1, 0, 1, 2, 5]
    for c in ((1 << 31) - 1, 1 << 31, 1 << 32, V - 1):
        m = c - c % W
        around += [m - W, m, m + W]
    ids = np.asarray(list(dict.fromkeys(around)) + [int(x) for x in rng.integers(0, V, 40)]
                     + [int(x) for x in rng.integers(1 << 32, V, 12)], np.int64)
    valid = [int(i) for i in dict.fromkeys(ids.tolist()) if 0 <= i < V]
    value = {i: np.float32(k + 1.5) for k, i in enumerate(valid)}
    true = [{i // W: value[i] for i in valid if i % W == r} for r in range(W)]
    decoy = [dict() for _ in range(W)]
    k = 0
    for i in valid:
        for r in range(W):
            for row in ((i % (1 << 32)) // W, i // W - 1, i // W + 1):
                if 0 <= row < big_rows(r) and row not in true[r] and row not in decoy[r]:
                    decoy[r][row] = np.float32(-(k + 1.5))
                    k += 1
    cols = [ColumnSpec(FORM_GATHER, 1, V, COMBINER_NONE, IDS_I64, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 0),
            ColumnSpec(FORM_SEGMENT_REDUCE, 1, V, COMBINER_SUM, IDS_I64, 0, 1, 2, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 1, 0)]
    spec = PlanSpec(cols, [1, 1, 1], [8, 8, 4], 1, n_groups=2, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()

    def request(a):
        lens = _spread(a.size, (1, 3, 0, 2, 5, 1))
        return [a, a[::-1].copy(), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)], np.asarray([a.size], np.int32)
    first = request(ids)
    return spec, [first, request(np.roll(ids, 7)[:-3]), first], value, true, decoy


def big_expected(value: dict, inputs, rank: int, world: int):
    """([gather [n, 1], sums [rows, 1]], bad ids) of one rank (world 1: the unsharded answer), from the id -> value map."""
    def val(i):
        return value[i] if i in value and i % world == rank else np.float32(0.0)
    g = np.asarray([[val(int(i))] for i in inputs[0]], np.float32)
    o = inputs[2]
    s = np.zeros((o.size - 1, 1), np.float32)
    for r in range(o.size - 1):
        acc = np.float32(0.0)
        for i in inputs[1][o[r]:o[r + 1]]:
            acc = acc + val(int(i))
        s[r, 0] = acc
    bad = sum(int(not 0 <= int(i) < BIG_VOCAB) for a in inputs[:2] for i in a)
    return [g, s], bad


# ---- A3: pooled specials ----------------------------------------------------------------------------------------------
def _f(u: int) -> np.float32:
    return np.uint32(u).view(np.float32)


FLT_MAX = np.finfo(np.float32).max
NAN_PAYLOAD = _f(0x7FC01234)
SUB_MAX, SUB_MIN, MIN_NORMAL = _f(0x007FFFFF), _f(0x00000001), _f(0x00800000)
SP_VOCAB = 40
N_ORDINARY = 16
# whole rows of the special tables (the same row numbers in every table); 25 / 26: magnitude 2^-140
ROW_INF, ROW_NINF, ROW_NAN, ROW_NEG0, ROW_FMAX, ROW_NFMAX, ROW_SUBMAX, ROW_SUBMIN, ROW_MINNORM, ROW_T140A, ROW_T140B = range(16, 27)
ROW_FMAX2 = 37            # a second +FLT_MAX row, on another rank than ROW_FMAX under world 2 and world 3
SINGLE_FIRST = 27         # rows 27..34: ordinary rows with one element each of the eight specials below
SINGLES = (np.float32(np.inf), np.float32(-np.inf), NAN_PAYLOAD, np.float32(-0.0), FLT_MAX, -FLT_MAX, SUB_MAX, SUB_MIN)
DROPPED_ID, OOV_IDS = 1000, (-1, SP_VOCAB, SP_VOCAB + 1, I32_MAX)
BAG_LENS = (1, 4, 5, 10, 11, 17)
LONG_BAG = 400            # > 384 ids: the fair-share rounds
OUTCOMES = ("neg0_single", "neg0_only", "inf_among_finite", "inf_minus_inf", "nan_first", "nan_middle", "nan_last",
            "fmax_order", "fmax_cross_rank", "subnormal_sum", "subnormal_quotient", "oov_only", "all_filtered",
            "single_elements", "ordinary")
NAN_OUTCOMES = ("inf_minus_inf", "nan_first", "nan_middle", "nan_last")
# which outcome a bag gets: position in this schedule; the four NaN outcomes once each in 44
_SCHEDULE = tuple(o for rep in range(4) for o in OUTCOMES if o not in NAN_OUTCOMES) + NAN_OUTCOMES


def special_table(dim: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((SP_VOCAB, dim)).astype(np.float32)
    for row, v in ((ROW_INF, np.inf), (ROW_NINF, -np.inf), (ROW_NAN, NAN_PAYLOAD), (ROW_NEG0, -0.0), (ROW_FMAX, FLT_MAX),
                   (ROW_NFMAX, -FLT_MAX), (ROW_SUBMAX, SUB_MAX), (ROW_SUBMIN, SUB_MIN), (ROW_MINNORM, MIN_NORMAL),
                   (ROW_FMAX2, FLT_MAX)):
        t[row] = v
    e = np.arange(dim)
    t[ROW_T140A] = ((1 + 2 * (e % 4)) * 2.0 ** -140).astype(np.float32)
    t[ROW_T140B] = (-(3 + 2 * (e % 3)) * 2.0 ** -140).astype(np.float32)
    for j, v in enumerate(SINGLES):
        t[SINGLE_FIRST + j, (seed + j) % dim] = v
    return t


def _bag(outcome: str, L: int, filtered: bool, salt: int) -> List[int]:
    """The ids of one bag of L ids (some outcomes need a minimum) that produces `outcome`.  Padding is the -0.0 row (x + -0.0
    is x for every x) and, in filtered columns, every other pad an id the filter drops (it changes the mean's divisor)."""
    def pad(n, at=0):
        return [DROPPED_ID if filtered and (at + i) % 2 else ROW_NEG0 for i in range(n)]

    def ordinary(n):
        return [(salt + 5 * i) % N_ORDINARY for i in range(n)]

    def put(core, n):
        n = max(n, len(core))
        k = (salt % (n - len(core) + 1))
        return pad(k) + core + pad(n - len(core) - k, k)
    if outcome == "neg0_single":
        return [ROW_NEG0]
    if outcome == "neg0_only":
        return [ROW_NEG0] * L
    if outcome == "inf_among_finite":
        b = ordinary(max(L, 2))
        b[salt % len(b)] = (ROW_INF, ROW_NINF)[salt % 2]
        return b
    if outcome == "inf_minus_inf":
        b = ordinary(max(L, 2))
        b[0], b[-1] = ((ROW_INF, ROW_NINF), (ROW_NINF, ROW_INF))[salt % 2]
        return b
    if outcome.startswith("nan_"):
        b = ordinary(max(L, 3))
        b[{"nan_first": 0, "nan_middle": len(b) // 2, "nan_last": len(b) - 1}[outcome]] = ROW_NAN
        return b
    if outcome == "fmax_order":          # (FLT_MAX + FLT_MAX) - FLT_MAX = +inf; FLT_MAX - FLT_MAX + FLT_MAX would be FLT_MAX
        return put([ROW_FMAX, ROW_FMAX, ROW_NFMAX], L)
    if outcome == "fmax_cross_rank":     # one FLT_MAX per rank: the overflow happens in the finalize's add
        return put([ROW_FMAX, ROW_FMAX2], L)
    if outcome == "subnormal_sum":       # every add exact, the sum below 2^-126; rows 25 and 26 lie on different ranks
        return put([ROW_T140A, ROW_T140B, ROW_SUBMIN, ROW_T140A], L)
    if outcome == "subnormal_quotient":  # 2^-126 / n, n not a power of two: a rounded subnormal quotient (means)
        n = L if L & (L - 1) else L + 1 + (L == 1)
        return [ROW_NEG0] * (salt % n) + [ROW_MINNORM] + [ROW_NEG0] * (n - 1 - salt % n)
    if outcome == "oov_only":
        return [OOV_IDS[(salt + i) % len(OOV_IDS)] for i in range(L)]
    if outcome == "all_filtered":        # (columns without a filter: ids outside the vocabulary)
        return [DROPPED_ID + i for i in range(L)]
    if outcome == "single_elements":
        b = ordinary(L)                  # one row with one special element among ordinary rows
        b[salt % L] = SINGLE_FIRST + salt % len(SINGLES)
        return b
    return ordinary(L)


@dataclasses.dataclass(frozen=True)
class SpecialCell:
    kernel: str     # ragged | hybrid
    vec: int
    world: int

    @property
    def id(self) -> str:
        return f"{self.kernel}-V{self.vec}-w{self.world}"


def special_cells() -> List[SpecialCell]:
    return [SpecialCell(k, v, w) for k in ("ragged", "hybrid") for v in K.VECS for w in WORLDS]


@dataclasses.dataclass
class SpecialCase(Case):
    roles: list             # per column
    outcomes: list          # per request: {column: [outcome of each row's bag]}


SPECIAL_ROWS = (7, 12, 7)


@functools.lru_cache(maxsize=None)
def special_case(kernel: str, vec: int) -> SpecialCase:
    """The layout generator of kernel_variant_cases (`_layout` / `_run_slots`, variant 2: 8 spans — hybrid: 8 + 8 —, one
    group), with the special tables and built bags.  Pooled columns cycle sum / mean / filtered mean (FILTER [0, vocab + 1]:
    ids just outside the vocabulary are kept and count, DROPPED_ID.. are dropped)."""
    variant = 2
    groups = K._layout(kernel, variant)
    cols, ranks, esz, tables, roles = [], [], [], [], []

    def host(rank, e):
        ranks.append(rank)
        esz.append(e)
        return len(ranks) - 1
    n_pool = 0
    for g, runs in enumerate(groups):
        for ri, (kind, nspans, lanes64, tail) in enumerate(runs):
            for w in K._run_slots(nspans, 3 * ri + 5 * g + variant, lanes64, tail):
                dim, k = w * vec, len(cols)
                if kind == 0:
                    role = ("gather", "passthrough", "gather_filter")[k % 3]
                else:
                    role = ("sum", "mean", "mean_filter")[n_pool % 3]
                    n_pool += 1
                roles.append(role)
                if role == "passthrough":
                    i = host(2, 4)
                    cols.append(ColumnSpec(FORM_PASSTHROUGH, dim, 0, COMBINER_NONE, IDS_I32, -1, i, -1, SEG_NONE, 1,
                                           ROWS_FROM_INPUT_DIM0, i, None, g, k))
                    continue
                tables.append(special_table(dim, 1000 * vec + k))
                src = IDS_I64 if k % 2 else IDS_I32
                i = host(1, 8 if src == IDS_I64 else 4)
                xf = dict(xform_mode=XFORM_FILTER, xform_lo=(0,), xform_hi=(SP_VOCAB + 1,)) if role.endswith("_filter") else {}
                if kind == 0:
                    cols.append(ColumnSpec(FORM_GATHER, dim, SP_VOCAB, COMBINER_NONE, src, len(tables) - 1, i, -1, SEG_NONE, 1,
                                           ROWS_FROM_IDS, 0, None, g, k, **xf))
                else:
                    si = host(1, 4)
                    cols.append(ColumnSpec(FORM_SEGMENT_REDUCE, dim, SP_VOCAB, COMBINER_SUM if role == "sum" else COMBINER_MEAN,
                                           src, len(tables) - 1, i, si, SEG_CSR_I32 if k % 2 == 0 else SEG_IDS_I32, 1,
                                           ROWS_FROM_SYMBOL, g, None, g, k, **xf))
    nxt = [0] * len(groups)
    for c in cols:
        c.concat_slot = nxt[c.concat_group]
        nxt[c.concat_group] += 1
    spec = PlanSpec(cols, ranks, esz, len(tables), n_groups=len(groups), n_symbols=len(groups), flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    requests, outcomes = [], []
    for t in range(N_REQUESTS):
        if t == 2:
            requests.append(requests[0])
            outcomes.append(outcomes[0])
            continue
        B = SPECIAL_ROWS[t]
        rng = np.random.default_rng(500 + t)
        inputs, oc, j = [], {}, 0
        for k, (c, role) in enumerate(zip(cols, roles)):
            dt = np.int64 if c.id_source == IDS_I64 else np.int32
            if role == "passthrough":
                x = rng.standard_normal((B, c.dim)).astype(np.float32)
                x[::3, ::2] = np.resize(np.asarray(SINGLES, np.float32), x[::3, ::2].shape)
                inputs.append(x)
            elif c.form == FORM_GATHER:      # copies of whole special rows, ids outside the vocabulary, dropped ones
                ids = (np.arange(B) * 5 + k) % (SP_VOCAB + 2) - 1
                ids[k % B] = DROPPED_ID
                inputs.append(ids.astype(dt))
            else:
                bags, oc[k] = [], []
                for r in range(B):
                    o = _SCHEDULE[(7 * r + 3 * j + 11 * t) % len(_SCHEDULE)]
                    L, salt = BAG_LENS[(r + j + t) % len(BAG_LENS)], r + 2 * j + t
                    if r == B - 1 and j < 6:      # once inside a long bag, the special rows across the 384-id tile's end
                        o = ("fmax_order", "subnormal_quotient", "nan_middle", "subnormal_sum", "inf_among_finite", "neg0_only")[j]
                        L, salt = LONG_BAG + j, 383 - j % 2
                    if o == "all_filtered" and role != "mean_filter":
                        o = "oov_only"
                    if o == "subnormal_quotient" and role == "sum":
                        o = "subnormal_sum"
                    bag = _bag(o, L, role == "mean_filter", salt)
                    bags.append(bag)
                    oc[k].append(o)
                lens = np.asarray([len(b) for b in bags], np.int64)
                inputs.append(np.asarray([i for b in bags for i in b], dt))
                inputs.append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32) if c.seg_kind == SEG_CSR_I32
                              else np.repeat(np.arange(B, dtype=np.int32), lens))
                j += 1
        requests.append((inputs, np.asarray([B] * len(groups), np.int32)))
        outcomes.append(oc)
    return SpecialCase(spec, tables, requests, roles, outcomes)


def outcome_holds(outcome: str, role: str, want: np.ndarray) -> np.ndarray:
    """Per element of a bag's expected result [dim]: does the outcome show in it?"""
    u = bits(want)
    sub = (np.abs(want) < MIN_NORMAL) & (want != 0)
    if outcome in ("neg0_single", "neg0_only", "oov_only", "all_filtered"):
        return u == 0                                   # +0.0, all bits clear
    if outcome == "inf_among_finite":
        return np.isinf(want)
    if outcome in NAN_OUTCOMES:
        return np.isnan(want)
    if outcome in ("fmax_order", "fmax_cross_rank"):
        return want == np.inf
    if outcome == "subnormal_sum":
        return sub
    if outcome == "subnormal_quotient":                 # inexact: q * n differs from 2^-126 for every n that is not 2^k
        return sub if role != "sum" else np.zeros(want.shape, bool)
    if outcome == "single_elements":
        return ~np.isfinite(want) | (np.abs(want) > 1e30)
    return np.isfinite(want)


def outcome_counts(case: SpecialCase, results: list) -> dict:
    """{outcome: output elements of the plan's three requests in which it shows}, from per-request expected groups."""
    offs = case.spec.column_offsets()
    n = {o: 0 for o in OUTCOMES}
    for t in range(N_REQUESTS):
        for k, ocs in case.outcomes[t].items():
            c = case.spec.columns[k]
            blk = results[t][c.concat_group][:, offs[k]:offs[k] + c.dim]
            for r, o in enumerate(ocs):
                n[o] += int(outcome_holds(o, case.roles[k], blk[r]).sum())
    return n


def nan_share(case: SpecialCase, groups: list) -> float:
    """NaN elements among the pooled elements of one request's expected groups."""
    offs = case.spec.column_offsets()
    nan = tot = 0
    for k, c in enumerate(case.spec.columns):
        if c.form == FORM_SEGMENT_REDUCE:
            blk = groups[c.concat_group][:, offs[k]:offs[k] + c.dim]
            nan += int(np.isnan(blk).sum())
            tot += blk.size
    return nan / max(tot, 1)
