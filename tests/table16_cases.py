"""16-bit tables (FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16): the value model restated, the cells and the small plans
(tests/test_table16_host.py on the CPU, tests/test_gpu_table16.py on the GPU).  Test data only.

The value model is one sentence: a 16-bit table element widens to float32 EXACTLY, so a plan with 16-bit tables computes,
bit for bit, what the float32 plan computes on the widened tables.  The yardstick of every GPU comparison is therefore the
existing oracle run on `widen(tables)` with the plan's float32 twin; no rounding happens anywhere and nothing is compared
with a tolerance.  Rule: bit patterns equal wherever the expectation is not NaN, NaN where it is.

`widen` is written in integers, on purpose apart from any library cast; the CPU test holds it to torch's and NumPy's casts
on all 65 536 patterns of each dtype."""
import dataclasses
import functools
from typing import List

import numpy as np

import kernel_variant_cases as K
import narrow_output_cases as N
from recom_amd.plan import (COMBINER_NONE, COMBINER_SQRTN, COMBINER_SUM, FLAG_COUNT_BAD_IDS, FORM_EXTERNAL, FORM_GATHER,
                            FORM_GATHER_SCATTER, FORM_SEGMENT_REDUCE, IDS_I32, IDS_I64, ROWS_FROM_GROUP, ROWS_FROM_IDS, ROWS_FROM_SYMBOL, SEG_CSR_I32,
                            SEG_NONE, XFORM_FILTER, XFORM_SELECT, ColumnSpec, PlanSpec)

DTYPES = ("bf16", "f16")


# ---- the widening restatement -------------------------------------------------------------------------------------------
def _widen_bf16(h: np.ndarray) -> np.ndarray:
    """bf16 is the upper half of the float32 pattern."""
    return h.astype(np.uint32) << 16


def _widen_f16(h: np.ndarray) -> np.ndarray:
    """binary16 -> binary32 in integers: normal values re-bias the exponent (15 -> 127) and move the 10 fraction bits to
    the top of the 23; inf / NaN keep their fraction bits there; a subnormal m x 2^-24 (m in 1..1023) is normalised — its
    leading one at bit p becomes the hidden bit of 2^(p - 24)."""
    h = h.astype(np.uint32)
    sign = (h & 0x8000) << 16
    e = (h >> 10) & 0x1F
    m = h & 0x3FF
    normal = ((e + 112) << 23) | (m << 13)
    special = 0x7F800000 | (m << 13)
    p = np.zeros_like(m)                                  # position of the leading one of m (m > 0)
    for bit in range(1, 10):
        p = np.where(m >> bit, bit, p)
    sub = np.where(m > 0, ((p + 103) << 23) | ((m << (23 - p)) & 0x7FFFFF), 0)
    return sign | np.where(e == 31, special, np.where(e == 0, sub, normal)).astype(np.uint32)


def widen(bits16, dtype: str) -> np.ndarray:
    """float32 array of the 16-bit patterns `bits16` of `dtype` ("bf16" | "f16"), exact."""
    h = np.ascontiguousarray(bits16, np.uint16)
    return {"bf16": _widen_bf16, "f16": _widen_f16}[dtype](h).astype(np.uint32).view(np.float32).reshape(h.shape)


def assert_same_bits(got, want, what) -> int:
    """float32 `got` against the oracle's float32 `want`: patterns equal wherever the expectation is not NaN, NaN where it
    is.  Returns the number of elements compared as "is NaN" (from the expectation)."""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    diff = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    if diff.any():
        idx = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ, first {idx} got "
                             f"{int(got.view(np.uint32)[idx]):#010x} want {int(want.view(np.uint32)[idx]):#010x}")
    return int(nan.sum())


# ---- variant cells ------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Tab16Cell:
    cell: K.Cell
    dtype: str

    @property
    def id(self) -> str:
        return f"{self.cell.id}-tab{self.dtype}"


def variant_cells() -> List[Tab16Cell]:
    """Every unsharded cell of kernel_variant_cases.cells() in both table dtypes."""
    return [Tab16Cell(c, dt) for c in K.cells() if not c.sharded for dt in DTYPES]


def kernel_names() -> dict:
    """mangled-name fragment -> (kernel, V, R) of every instantiation the cells reach: fcp_tables16.hip holds exactly these."""
    out = {}
    for kernel, v, r, sharded in {K.instantiation(c.cell) for c in variant_cells()}:
        assert not sharded
        frag = f"fcp_{kernel}_tab16_kernelILi{v}E" + (f"Li{r}E" if kernel != "ragged" else "") + "E"
        out[frag] = (kernel, v, r)
    return out


@functools.lru_cache(maxsize=None)
def case_tables(key, dtype: str):
    """(16-bit patterns, their widened float32 form) of the tables of the variant case `key`: the case's float32 tables
    rounded to `dtype` with the narrow-output restatement."""
    bits = [N.narrow(t, dtype) for t in K.build_case(*key).tables]
    return bits, [widen(b, dtype) for b in bits]


@functools.lru_cache(maxsize=None)
def case_expectation(key, dtype: str, t: int):
    """The oracle on the widened tables with the float32 twin: (groups, bad ids) of request t.  Computed once per
    (case, dtype, request) and shared by the cells that differ only in store policy and wide rows."""
    import fcp_oracle
    from recom_amd.ops import concat_inputs
    case = K.build_case(*key)
    inputs, symbols = case.requests[t]
    blob, offsets, shapes = concat_inputs(inputs)
    want, bad = fcp_oracle.COracle().process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, case_tables(key, dtype)[1],
                                                             symbols)
    for w in want:
        w.setflags(write=False)
    return want, bad


# ---- every pattern --------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PatternCase:
    spec: PlanSpec          # float32 twin
    bits: np.ndarray        # uint16 [65536 / V, V]: every pattern once
    inputs: list
    symbols: np.ndarray


@functools.lru_cache(maxsize=None)
def pattern_case(vec: int) -> PatternCase:
    """One table holding all 65 536 bit patterns once (dim = V, vocab = 65 536 / V), read once through a GATHER column
    (group 0: a span without pooled columns, the dense body) and once as bags of exactly one id through a pooled SUM
    column (group 1: the ragged body).  The ids are a fixed permutation of the rows."""
    vocab = 65536 // vec
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(vocab, vec)
    rng = np.random.default_rng(160 + vec)
    cols = [ColumnSpec(FORM_GATHER, vec, vocab, COMBINER_NONE, IDS_I32, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 0),
            ColumnSpec(FORM_SEGMENT_REDUCE, vec, vocab, COMBINER_SUM, IDS_I64, 0, 1, 2, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 1, 0)]
    spec = PlanSpec(cols, [1, 1, 1], [4, 8, 4], 1, n_groups=2, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    inputs = [rng.permutation(vocab).astype(np.int32), rng.permutation(vocab).astype(np.int64), np.arange(vocab + 1, dtype=np.int32)]
    return PatternCase(spec, bits, inputs, np.asarray([vocab], np.int32))


def nan_patterns(dtype: str) -> np.ndarray:
    """bool[65536]: which 16-bit patterns are NaN — from the patterns themselves."""
    h = np.arange(65536, dtype=np.uint32)
    return (h & 0x7FFF) > (0x7F80 if dtype == "bf16" else 0x7C00)


# ---- copies and limits ------------------------------------------------------------------------------------------------------
def mixed_spec(layout=None):
    """(model, float32 twin spec): synth.model_mixed — GATHER by int64 / int32 ids and by bucketized floats, pooled sums and
    means in three segment encodings, GATHER_SCATTER with its row ids in any order, PASSTHROUGH, BATCH_COL_REDUCTION — with
    an EXTERNAL slot at the end of group 0 (CONCAT only) and FCP_FLAG_COUNT_BAD_IDS."""
    from recom_amd import synth
    from recom_amd.plan import LAYOUT_PER_COLUMN
    m = synth.model_mixed(batch=37, vocab=211)
    cols = list(m.spec.columns)
    if layout != LAYOUT_PER_COLUMN:
        top = max(c.concat_slot for c in cols if c.concat_group == 0) + 1
        cols.append(ColumnSpec(FORM_EXTERNAL, 4, rows_source=ROWS_FROM_GROUP, concat_group=0, concat_slot=top))
    spec = dataclasses.replace(m.spec, columns=cols, flags=FLAG_COUNT_BAD_IDS, **({} if layout is None else {"layout": layout}))
    spec.validate()
    return m, spec


def with_bad_ids(inputs, spec: PlanSpec, seed: int):
    """The request with some ids of every lookup column replaced by out-of-vocabulary and negative ones."""
    rng = np.random.default_rng(seed)
    out = [np.array(a, copy=True) for a in inputs]
    for c in spec.columns:
        if c.form not in (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER) or c.id_source not in (IDS_I32, IDS_I64):
            continue
        ids = out[c.ids_input].reshape(-1)
        if ids.size:
            hit = rng.random(ids.size) < 0.1
            ids[hit] = rng.choice(np.asarray([-1, -7, c.vocab, c.vocab + 3], ids.dtype), int(hit.sum()))
    return out


def xform_spec() -> PlanSpec:
    """FILTER, SELECT and hashed ids in front of 16-bit lookups: a filtered mean, a SELECT gather and a hashed sum."""
    from recom_amd.plan import COMBINER_MEAN
    cols = [ColumnSpec(FORM_SEGMENT_REDUCE, 6, 40, COMBINER_MEAN, IDS_I64, 0, 0, 1, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 0, 0,
                       xform_mode=XFORM_FILTER, xform_lo=(3, 30), xform_hi=(20, 35)),
            ColumnSpec(FORM_GATHER, 10, 50, COMBINER_NONE, IDS_I32, 1, 2, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 1,
                       xform_mode=XFORM_SELECT, xform_lo=(-1,), xform_hi=(52,), xform_substitute=7),
            ColumnSpec(FORM_SEGMENT_REDUCE, 4, 31, COMBINER_SUM, IDS_I64, 2, 3, 4, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 0, 2,
                       hash_buckets=31)]
    spec = PlanSpec(cols, [1, 1, 1, 1, 1], [8, 4, 4, 8, 4], 3, n_groups=1, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    return spec


def xform_request(rows: int = 29, seed: int = 5):
    rng = np.random.default_rng(seed)
    lens0, lens2 = rng.integers(0, 9, rows), rng.integers(0, 5, rows)
    inputs = [rng.integers(-2, 44, int(lens0.sum())).astype(np.int64), np.concatenate([[0], np.cumsum(lens0)]).astype(np.int32),
              rng.integers(-3, 55, rows).astype(np.int32),
              rng.integers(-10 ** 12, 10 ** 12, int(lens2.sum())).astype(np.int64), np.concatenate([[0], np.cumsum(lens2)]).astype(np.int32)]
    return inputs, np.asarray([rows], np.int32)


def random_bits(shape, dtype: str, seed: int) -> np.ndarray:
    """Finite, ordinary 16-bit table contents: standard normals rounded to `dtype`."""
    return N.narrow(np.random.default_rng(seed).standard_normal(shape).astype(np.float32), dtype)


# ---- refused plans ----------------------------------------------------------------------------------------------------------
def refused_specs() -> dict:
    """kind -> (float32 spec that the library accepts, extra flag bits of the refused twin besides the table bit, a word
    the refusal must carry)."""
    from recom_amd.plan import FLAG_OUT_BF16, FLAG_OUT_F16
    base = N._small_spec()
    w = dataclasses.replace(base, columns=[base.columns[0], dataclasses.replace(base.columns[1], weights_input=3)])
    sq = dataclasses.replace(base, columns=[base.columns[0], dataclasses.replace(base.columns[1], combiner=COMBINER_SQRTN)])
    return {"out_bf16": (base, FLAG_OUT_BF16, "narrow output"),
            "out_f16": (base, FLAG_OUT_F16, "narrow output"),
            "sharded": (N._small_spec(shard_rank=1, shard_world=2), 0, "shard_world"),
            "weighted": (w, 0, "per-id weights"),
            "sqrtn": (sq, 0, "FCP_COMBINER_SQRTN")}


# ---- the closed form of the full-size request -------------------------------------------------------------------------------
def closed_form_check(model, req, got: np.ndarray, dtype: str) -> None:
    """A gather is a pure copy: every output row is the closed-form table row (synth.hash_rows) rounded once to the table
    dtype — what the table holds — and widened."""
    from recom_amd import synth
    import fcp_oracle as O
    offs = model.spec.column_offsets()
    for k, c in enumerate(model.spec.columns):
        sl = got[:, offs[k]:offs[k] + c.dim]
        raw = req.inputs[c.ids_input]
        ids = O.np_bucketize(c.boundaries, raw) if c.id_source == 2 else raw
        want = widen(N.narrow(synth.hash_rows(model.tables[c.table_input].seed, ids, c.dim), dtype), dtype)
        assert np.array_equal(sl.view(np.uint32), want.view(np.uint32)), f"column {k}"
