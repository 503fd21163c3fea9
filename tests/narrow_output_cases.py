"""Narrow output (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16): the value model restated, the cells and the edge plans
(tests/test_narrow_output_host.py on the CPU, tests/test_gpu_narrow_output.py on the GPU).  Test data only.

The value model is one sentence: a narrow element is the float32 value the float32 plan writes, rounded ONCE to
nearest-even.  So the yardstick of every GPU comparison is `narrow(oracle float32 output, dtype)` — the existing oracle run
on the float32 twin of the plan, passed through the restatement below — compared as 16-bit patterns.

`narrow` is written in integers, on purpose apart from any library cast; the CPU test holds it to torch's and NumPy's
casts on the edge list and on 10^6 random bit patterns."""
import dataclasses
import functools
from typing import List, Tuple

import numpy as np

import kernel_variant_cases as K
from recom_amd.plan import (COMBINER_MEAN, COMBINER_NONE, COMBINER_SQRTN, COMBINER_SUM, FORM_EXTERNAL, FORM_GATHER,
                            FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE, IDS_I32, IDS_I64, LAYOUT_PER_COLUMN, ROWS_FROM_GROUP,
                            ROWS_FROM_IDS, ROWS_FROM_INPUT_DIM0, ROWS_FROM_SYMBOL, SEG_CSR_I32, SEG_IDS_I32, SEG_NONE,
                            ColumnSpec, PlanSpec)

DTYPES = ("bf16", "f16")
N_REQUESTS = 3


# ---- the narrowing restatement ------------------------------------------------------------------------------------------
def _bf16_bits(u: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even on the upper half of the pattern: the carry of the rounding runs into the exponent (overflow
    gives +-inf), float32 subnormals round like every other value, NaN stays NaN (quiet, sign kept)."""
    u = u.astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def _f16_bits(u: np.ndarray) -> np.ndarray:
    """binary32 -> binary16, round-to-nearest-even, in integers: normal results re-bias the exponent and round 13 bits
    away (the carry overflows to inf from 65520 on); results below 2^-14 are the 24-bit significand shifted to units of
    2^-24, rounded to even (gradual underflow; float32 subnormals vanish)."""
    u = u.astype(np.uint64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    nan = a > 0x7F800000
    # normal range (and overflow): exponent 127 -> 15
    rn = a - np.where(a >= 0x38000000, 0x38000000, a)
    normal = np.minimum((rn + 0xFFF + ((rn >> 13) & 1)) >> 13, 0x7C00)
    # subnormal range: |x| < 2^-14
    e = a >> 23
    m = np.where(e > 0, (a & 0x7FFFFF) | 0x800000, 0)
    shift = np.minimum(126 - e.astype(np.int64), 40).astype(np.uint64)       # 2^(e - 150) / 2^-24 = 2^-(126 - e)
    shift = np.maximum(shift, 1)
    q = m >> shift
    rem = m & ((np.uint64(1) << shift) - 1)
    half = np.uint64(1) << (shift - 1)
    sub = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    out = np.where(a >= 0x38800000, normal, sub)
    out = np.where(nan, 0x7E00, out)
    return (sign | out).astype(np.uint16)


def narrow(x, dtype: str) -> np.ndarray:
    """The 16-bit patterns of float32 `x` rounded once, to nearest-even, to `dtype` ("bf16" | "f16")."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return {"bf16": _bf16_bits, "f16": _f16_bits}[dtype](u).reshape(u.shape)


def is_nan16(h: np.ndarray, dtype: str) -> np.ndarray:
    h = np.asarray(h, np.uint16)
    return (h & 0x7FFF) > (0x7F80 if dtype == "bf16" else 0x7C00)


def truncate_bf16(x) -> np.ndarray:
    """What a kernel that drops the low half instead of rounding would write."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def assert_same16(got, want32, dtype: str, what) -> float:
    """`got` (uint16 patterns) against narrow(`want32`): patterns equal wherever the expectation is not NaN, NaN where it
    is.  Returns the share of elements compared as "is NaN" (from the expectation)."""
    want = narrow(want32, dtype)
    got = np.asarray(got, np.uint16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = is_nan16(want, dtype)
    diff = np.where(nan, ~is_nan16(got, dtype), got != want)
    if diff.any():
        r, c = (int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ, first [{r}, {c}] got {int(got[r, c]):#06x} "
                             f"want {int(want[r, c]):#06x} (float32 {np.asarray(want32)[r, c]!r})")
    return float(nan.mean()) if nan.size else 0.0


def _f(u: int) -> np.float32:
    return np.asarray([u], np.uint32).view(np.float32)[0]


FLT_MAX = np.finfo(np.float32).max
# (float32 pattern, bf16 pattern, fp16 pattern): the edge list, with what the specification says of each
EDGES: Tuple[Tuple[int, int, int], ...] = (
    (0x3F808000, 0x3F80, 0x3C04),      # bf16 tie, down to even
    (0x3F818000, 0x3F82, 0x3C0C),      # bf16 tie, up to even
    (0x3F808001, 0x3F81, 0x3C04),      # just above the tie
    (0x3F807FFF, 0x3F80, 0x3C04),      # just below it
    (0x3F801000, 0x3F80, 0x3C00),      # fp16 tie (1 + 2^-11), down to even
    (0x3F803000, 0x3F80, 0x3C02),      # fp16 tie (1 + 2^-10 + 2^-11), up to even
    (0x7F7FFFFF, 0x7F80, 0x7C00),      # FLT_MAX -> inf in both
    (0xFF7FFFFF, 0xFF80, 0xFC00),
    (0x7F7F7FFF, 0x7F7F, 0x7C00),      # below the last half-ulp under 2^128: the largest bf16
    (0x7F7F8000, 0x7F80, 0x7C00),      # the tie at it: to even = inf
    (0x477FEFFF, 0x4780, 0x7BFF),      # 65519.996 -> 65504 (fp16)
    (0x477FF000, 0x4780, 0x7C00),      # 65520 -> inf (fp16)
    (0xC77FEFFF, 0xC780, 0xFBFF),
    (0xC77FF000, 0xC780, 0xFC00),
    (0x477FE000, 0x4780, 0x7BFF),      # 65504 itself
    (0x38800000, 0x3880, 0x0400),      # 2^-14: the smallest normal fp16
    (0x387FFFFF, 0x3880, 0x0400),      # just below: rounds up into it
    (0x387FC000, 0x3880, 0x03FF),      # the largest fp16 subnormal
    (0x33800000, 0x3380, 0x0001),      # 2^-24: the smallest fp16 subnormal
    (0x33000000, 0x3300, 0x0000),      # half of it: tie, to even = 0
    (0x33000001, 0x3300, 0x0001),      # just above the tie
    (0x33C00000, 0x33C0, 0x0002),      # 1.5 x 2^-24: tie, to even = 2
    (0xB3000000, 0xB300, 0x8000),      # -2^-25 -> -0.0
    (0x00800000, 0x0080, 0x0000),      # FLT_MIN: the smallest normal of float32 and bf16
    (0x007F8000, 0x0080, 0x0000),      # bf16 subnormal range: tie at the top, up to even (into the normals)
    (0x00400000, 0x0040, 0x0000),      # 2^-127: a bf16 subnormal
    (0x00010000, 0x0001, 0x0000),      # 2^-133: the smallest bf16 subnormal
    (0x00008000, 0x0000, 0x0000),      # half of it: tie, to even = 0
    (0x00008001, 0x0001, 0x0000),      # just above the tie
    (0x00018000, 0x0002, 0x0000),      # 1.5 x: tie, to even = 2
    (0x80008000, 0x8000, 0x8000),      # the negative tie: -0.0
    (0x00000001, 0x0000, 0x0000),      # the smallest float32 subnormal
    (0x80000001, 0x8000, 0x8000),
    (0x007FFFFF, 0x0080, 0x0000),      # the largest float32 subnormal
    (0x00000000, 0x0000, 0x0000),      # +-0.0
    (0x80000000, 0x8000, 0x8000),
    (0x7F800000, 0x7F80, 0x7C00),      # +-inf
    (0xFF800000, 0xFF80, 0xFC00),
    (0x3F800000, 0x3F80, 0x3C00),      # a few ordinary values
    (0xC0490FDB, 0xC049, 0xC248),
    (0x42F6E979, 0x42F7, 0x57B7),
)
NAN_EDGES = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FC01234, 0xFFFFFFFF, 0x7F80FFFF, 0x7FFF8000)   # NaN stays NaN
EDGE_VALUES = np.asarray([e[0] for e in EDGES] + list(NAN_EDGES), np.uint32).view(np.float32)


# ---- variant cells ------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class NarrowCell:
    cell: K.Cell
    dtype: str

    @property
    def id(self) -> str:
        return f"{self.cell.id}-{self.dtype}"


def variant_cells() -> List[NarrowCell]:
    """Every unsharded cell of kernel_variant_cases.cells() in both narrow dtypes."""
    return [NarrowCell(c, dt) for c in K.cells() if not c.sharded for dt in DTYPES]


def kernel_names() -> dict:
    """mangled-name fragment -> (kernel, V, R) of every instantiation the cells reach: fcp_narrow.hip holds exactly these."""
    out = {}
    for kernel, v, r, sharded in {K.instantiation(c.cell) for c in variant_cells()}:
        assert not sharded
        frag = f"fcp_{kernel}_narrow_kernelILi{v}E" + (f"Li{r}E" if kernel != "ragged" else "") + "E"
        out[frag] = (kernel, v, r)
    return out


DISCRIMINATION_KEYS = (("dense", 4, 4, 0), ("ragged", 1, 1, 3), ("hybrid", 2, 2, 2))


# ---- edge plans ---------------------------------------------------------------------------------------------------------
# Pooled outcomes: (name, the float32 addends of the bag in id order).  The SUM column adds them; the MEAN column holds the
# addends times the bag's count n (a power of two: exact, up to overflow) padded with +0.0 rows to n ids, so its quotient
# is the same value — except `neg0`, whose mean is -2^-149 / 2: a tie that rounds to the float32 -0.0.
def _pw(e: int) -> np.float32:
    return np.float32(2.0 ** e)


OUTCOMES: Tuple[Tuple[str, Tuple[np.float32, ...]], ...] = (
    ("bf16_tie_down", (np.float32(1.0), _pw(-8))),                        # 0x3F808000
    ("bf16_tie_up", (np.float32(1.0), _pw(-7), _pw(-8))),                 # 0x3F818000
    ("f16_tie_down", (np.float32(1.0), _pw(-11))),                        # 0x3F801000
    ("f16_tie_up", (np.float32(1.0), _pw(-10), _pw(-11))),                # 0x3F803000
    ("f16_below_overflow", (np.float32(65504.0), np.float32(15.99609375))),   # 0x477FEFFF -> 65504
    ("f16_overflow", (np.float32(65504.0), np.float32(16.0))),            # 65520 -> inf
    ("f16_neg_overflow", (np.float32(-65504.0), np.float32(-16.0))),
    ("f16_sub_tie_zero", (_pw(-26), _pw(-26))),                           # 2^-25: tie -> 0
    ("f16_sub_up", (_pw(-25), _pw(-26))),                                 # 1.5 x 2^-25 -> 2^-24
    ("f16_sub_tie_even", (_pw(-24), _pw(-25))),                           # 1.5 x 2^-24: tie -> 2 x 2^-24
    ("f16_sub_max", (_f(0x387FC000),)),
    ("bf16_sub_tie_zero", (_f(0x00004000), _f(0x00004000))),              # 0x00008000: tie -> 0
    ("bf16_sub_tie_even", (_f(0x00010000), _f(0x00008000))),              # 0x00018000: tie -> 2
    ("bf16_sub", (_f(0x00400000), _f(0x00010000))),                       # 0x00410000
    ("neg0", (_f(0x80000001),)),                                          # float32 subnormal: -0.0 in both; its mean: a float32 -0.0
    ("flt_max", (FLT_MAX,)),                                              # -> inf in both
    ("overflow32", (FLT_MAX, FLT_MAX)),                                   # the float32 sum is inf already
    ("pos_inf", (np.float32(np.inf), np.float32(1.0))),
    ("neg_inf", (np.float32(-np.inf), np.float32(1.0))),
    ("inf_minus_inf", (np.float32(np.inf), np.float32(-np.inf))),         # NaN
    ("ordinary", (np.float32(3.25), np.float32(-1.125), np.float32(0.3))),
)
# float32 pattern each SUM outcome must land on (the CPU test holds the oracle to it): None = NaN
OUTCOME_BITS = {"bf16_tie_down": 0x3F808000, "bf16_tie_up": 0x3F818000, "f16_tie_down": 0x3F801000, "f16_tie_up": 0x3F803000,
                "f16_below_overflow": 0x477FEFFF, "f16_overflow": 0x477FF000, "f16_neg_overflow": 0xC77FF000,
                "f16_sub_tie_zero": 0x33000000, "f16_sub_up": 0x33400000, "f16_sub_tie_even": 0x33C00000,
                "f16_sub_max": 0x387FC000, "bf16_sub_tie_zero": 0x00008000, "bf16_sub_tie_even": 0x00018000,
                "bf16_sub": 0x00410000, "neg0": 0x80000001, "flt_max": 0x7F7FFFFF, "overflow32": 0x7F800000,
                "pos_inf": 0x7F800000, "neg_inf": 0xFF800000, "inf_minus_inf": None}
EDGE_ROWS = 2 * len(OUTCOMES) + 7          # every outcome twice, rows without ids in between


@dataclasses.dataclass
class EdgeCase:
    spec: PlanSpec              # the float32 twin; `.with_out_dtype(dt)` is the plan under test
    tables: List[np.ndarray]
    requests: list              # [(inputs, symbols)]
    outcome_rows: list          # per request: {row of group 1: outcome name}
    sum_cols: Tuple[int, int]   # [begin, end) of the SUM column in group 1
    mean_cols: Tuple[int, int]


def _cyclic(n_rows: int, dim: int, shift: int) -> np.ndarray:
    idx = (np.arange(n_rows * dim) + shift) % EDGE_VALUES.size
    return EDGE_VALUES[idx].reshape(n_rows, dim).copy()


@functools.lru_cache(maxsize=None)
def edge_case(vec: int) -> EdgeCase:
    """Group 0: a GATHER and a PASSTHROUGH column carrying the edge list (the dense body).  Group 1: a pooled SUM and a
    pooled MEAN column whose bags land on the outcomes above, beside rows without ids, then a GATHER and a PASSTHROUGH
    column again (the ragged body's copy paths).  Column dims are V x {3, 5, 7, 9, 11, 13}: their gcd is V."""
    d = [vec * w for w in (3, 5, 7, 9, 11, 13)]
    ranks, esz, tables, cols = [], [], [], []

    def host(rank, e):
        ranks.append(rank)
        esz.append(e)
        return len(ranks) - 1

    def gather(dim, group, slot, src):
        vocab = -(-EDGE_VALUES.size // dim) + 2
        tables.append(_cyclic(vocab, dim, 5 * len(tables)))
        i = host(1, 8 if src == IDS_I64 else 4)
        cols.append(ColumnSpec(FORM_GATHER, dim, vocab, COMBINER_NONE, src, len(tables) - 1, i, -1, SEG_NONE, 1,
                               ROWS_FROM_IDS, 0, None, group, slot))

    def passthrough(dim, group, slot):
        i = host(2, 4)
        cols.append(ColumnSpec(FORM_PASSTHROUGH, dim, 0, COMBINER_NONE, IDS_I32, -1, i, -1, SEG_NONE, 1, ROWS_FROM_INPUT_DIM0, i,
                               None, group, slot))

    gather(d[0], 0, 0, IDS_I64)
    passthrough(d[1], 0, 1)
    # pooled tables: per outcome its addends (SUM), or its addends times the count, padded with zero rows (MEAN)
    sum_rows, mean_rows, sum_bags, mean_bags = [], [], {}, {}
    for name, addends in OUTCOMES:
        sum_bags[name] = list(range(len(sum_rows), len(sum_rows) + len(addends)))
        sum_rows += list(addends)
        n = 2 if len(addends) <= 2 else 4
        scale = np.float32(1.0) if name == "neg0" else np.float32(n)
        mean_bags[name] = list(range(len(mean_rows), len(mean_rows) + n))
        with np.errstate(over="ignore"):
            mean_rows += [np.float32(a * scale) for a in addends] + [np.float32(0.0)] * (n - len(addends))
    for dim, rows, comb, csr in ((d[2], sum_rows, COMBINER_SUM, True), (d[3], mean_rows, COMBINER_MEAN, False)):
        tables.append(np.repeat(np.asarray(rows, np.float32)[:, None], dim, axis=1))
        i = host(1, 8 if csr else 4)
        si = host(1, 4)
        cols.append(ColumnSpec(FORM_SEGMENT_REDUCE, dim, len(rows), comb, IDS_I64 if csr else IDS_I32, len(tables) - 1, i, si,
                               SEG_CSR_I32 if csr else SEG_IDS_I32, 1, ROWS_FROM_SYMBOL, 1, None, 1, len(cols) - 2))
    gather(d[4], 1, 2, IDS_I32)
    passthrough(d[5], 1, 3)
    spec = PlanSpec(cols, ranks, esz, len(tables), n_groups=2, n_symbols=2)
    spec.validate()

    requests, outcome_rows = [], []
    names = [n for n, _ in OUTCOMES]
    for t in range(N_REQUESTS):
        tt = t % 2                                      # (the third request is the first again)
        b0, b1 = 33 + 31 * tt, EDGE_ROWS + tt
        where = {}
        for j in range(2 * len(names)):
            where[j + j // 6 + tt] = names[(j + 3 * tt) % len(names)]       # (every seventh row keeps no ids)
        assert max(where) < b1 and len(where) == 2 * len(names)
        inputs = []
        for c in cols:
            if c.form == FORM_PASSTHROUGH:
                B = b0 if c.concat_group == 0 else b1
                inputs.append(_cyclic(B, c.dim, 11 + 7 * tt + c.dim))
            elif c.form == FORM_GATHER:
                B = b0 if c.concat_group == 0 else b1
                ids = (np.arange(B) * 3 + tt) % c.vocab
                inputs.append(ids.astype(np.int64 if c.id_source == IDS_I64 else np.int32))
            else:
                bags = sum_bags if c.combiner == COMBINER_SUM else mean_bags
                per_row = [bags[where[r]] if r in where else [] for r in range(b1)]
                ids = np.asarray([i for bag in per_row for i in bag], np.int64)
                lens = np.asarray([len(bag) for bag in per_row], np.int64)
                inputs.append(ids.astype(np.int64 if c.id_source == IDS_I64 else np.int32))
                if c.seg_kind == SEG_CSR_I32:
                    inputs.append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
                else:
                    inputs.append(np.repeat(np.arange(b1, dtype=np.int32), lens))
        requests.append((inputs, np.asarray([b0, b1], np.int32)))
        outcome_rows.append(where)
    offs = spec.column_offsets()
    return EdgeCase(spec, tables, requests, outcome_rows, (offs[2], offs[2] + d[2]), (offs[3], offs[3] + d[3]))


# ---- refused plans ------------------------------------------------------------------------------------------------------
def _small_spec(**kw) -> PlanSpec:
    cols = [ColumnSpec(FORM_GATHER, 8, 50, COMBINER_NONE, IDS_I64, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 0),
            ColumnSpec(FORM_SEGMENT_REDUCE, 4, 60, COMBINER_MEAN, IDS_I64, 1, 1, 2, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 0, 1)]
    return PlanSpec(cols, [1, 1, 1, 1], [8, 8, 4, 4], 2, n_groups=1, n_symbols=1, **kw)


def refused_specs() -> dict:
    """kind -> (float32 spec that the library accepts, a word its narrow twin's refusal must carry)."""
    base = _small_spec()
    ext = dataclasses.replace(base, columns=base.columns + [ColumnSpec(FORM_EXTERNAL, 4, rows_source=ROWS_FROM_GROUP, concat_slot=2)])
    w = dataclasses.replace(base, columns=[base.columns[0], dataclasses.replace(base.columns[1], weights_input=3)])
    sq = dataclasses.replace(base, columns=[base.columns[0], dataclasses.replace(base.columns[1], combiner=COMBINER_SQRTN)])
    return {"sharded": (_small_spec(shard_rank=1, shard_world=2), "shard_world"),
            "per_column": (_small_spec(layout=LAYOUT_PER_COLUMN), "FCP_LAYOUT_PER_COLUMN"),
            "external": (ext, "FCP_FORM_EXTERNAL"),
            "weighted": (w, "per-id weights"),
            "sqrtn": (sq, "FCP_COMBINER_SQRTN")}


def small_shapes(rows: int = 5, nnz: int = 9):
    """(shapes, symbols) of a request of `_small_spec`."""
    return np.asarray([rows, nnz, rows + 1, nnz], np.int32), np.asarray([rows], np.int32)


# ---- the closed form of the full-size request (tests/test_gpu_parity.py::_closed_form_check, narrowed) ------------------------
def closed_form_check16(model, req, got16: np.ndarray, dtype: str) -> None:
    """A gather is a pure copy: every output row is the closed-form table row (synth.hash_rows), rounded once."""
    from recom_amd import synth
    import fcp_oracle as O
    offs = model.spec.column_offsets()
    for k, c in enumerate(model.spec.columns):
        sl = got16[:, offs[k]:offs[k] + c.dim]
        raw = req.inputs[c.ids_input]
        if c.form == FORM_PASSTHROUGH:
            want = raw.reshape(sl.shape)
        else:
            ids = O.np_bucketize(c.boundaries, raw) if c.id_source == 2 else raw
            want = synth.hash_rows(model.tables[c.table_input].seed, ids, c.dim)
        assert np.array_equal(sl, narrow(want, dtype)), f"column {k}"
