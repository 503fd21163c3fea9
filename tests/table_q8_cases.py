"""8-bit row-quantised tables (FCP_FLAG_TABLES_Q8): the value model restated, the cells and the small plans
(tests/test_table_q8_host.py on the CPU, tests/test_gpu_table_q8.py on the GPU).  Test data only.

The value model is one sentence: an element of a q8 table dequantises to the float32 value fma(float(code), scale, bias) —
the product exact, the sum rounded once to nearest-even — and the plan then computes, bit for bit, what the float32 plan
computes on the dequantised tables.  The yardstick of every GPU comparison is therefore the existing oracle run on
`dequantize(tables)` with the plan's float32 twin; nothing is compared with a tolerance.  Rule: bit patterns equal wherever
the expectation is not NaN, NaN where it is.

`dequantize` is synth.dequantize_q8; the CPU test holds it to quantized::embedding_bag_byte_unpack on arbitrary bytes and to
rational arithmetic (`fma_exact`, below) on the edge list and on random triples.  `two_roundings` is the OTHER reading of
"code * scale + bias" — a rounded product, then a rounded sum — which a kernel that left the fma to chance could compute;
tables are DRAWN (random codes, scales and biases), not quantised, and the two readings differ on 22-23 % of such elements, so
every comparison tells them apart."""
import dataclasses
import functools
import zlib
from fractions import Fraction
from typing import List

import numpy as np

import kernel_variant_cases as K
import narrow_output_cases as N
import table16_cases as T16
from recom_amd import synth
from recom_amd.plan import (COMBINER_NONE, COMBINER_SQRTN, COMBINER_SUM, FLAG_COUNT_BAD_IDS, FORM_GATHER, FORM_SEGMENT_REDUCE,
                            IDS_I32, IDS_I64, ROWS_FROM_IDS, ROWS_FROM_SYMBOL, SEG_CSR_I32, SEG_NONE, ColumnSpec, PlanSpec)

FLT_MAX = float(np.finfo(np.float32).max)
SUBNORMAL = float(np.float32(2.0 ** -149) * np.float32(12345))

assert_same_bits = T16.assert_same_bits          # (got, want, what): bits where the expectation is not NaN, NaN where it is
mixed_spec, with_bad_ids = T16.mixed_spec, T16.with_bad_ids
xform_spec, xform_request = T16.xform_spec, T16.xform_request


# ---- the format and the value model ----------------------------------------------------------------------------------------
def pack(codes: np.ndarray, scale: np.ndarray, bias: np.ndarray) -> np.ndarray:
    """uint8 [vocab, dim + 8]: codes, then the float32 scale, then the float32 bias, both little-endian."""
    codes = np.ascontiguousarray(codes, np.uint8)
    vocab, dim = codes.shape
    out = np.empty((vocab, dim + 8), np.uint8)
    out[:, :dim] = codes
    out[:, dim:dim + 4] = np.ascontiguousarray(scale, "<f4").view(np.uint8).reshape(vocab, 4)
    out[:, dim + 4:] = np.ascontiguousarray(bias, "<f4").view(np.uint8).reshape(vocab, 4)
    return out


def dequantize(table: np.ndarray) -> np.ndarray:
    """float32 [vocab, dim]: fma(float(code), scale, bias), rounded once."""
    return synth.dequantize_q8(table)


def two_roundings(table: np.ndarray) -> np.ndarray:
    """float32 [vocab, dim]: the product rounded to float32, then the sum rounded to float32 — NOT the value model."""
    codes, scale, bias = synth.q8_fields(table)
    with np.errstate(all="ignore"):
        return (codes.astype(np.float32) * scale[:, None] + bias[:, None]).astype(np.float32)


def draw_table(vocab: int, dim: int, seed: int) -> np.ndarray:
    """Random codes, scale = exp(N(-5, 2)), bias = N(0, 1): finite, no NaN, and rows of dim 1 are not degenerate."""
    rng = np.random.default_rng(seed)
    return pack(rng.integers(0, 256, (vocab, dim)), np.exp(rng.normal(-5, 2, vocab)).astype(np.float32),
                rng.normal(0, 1, vocab).astype(np.float32))


def _round_to_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the rational x != 0, ties to even, overflow to infinity: in integers."""
    sign, a = (-1.0 if x < 0 else 1.0), abs(x)
    n, d = a.numerator, a.denominator
    e = n.bit_length() - d.bit_length()                     # 2^e <= a < 2^(e + 1) after the correction below
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1
    q = max(e, -126) - 23                                   # exponent of the last place (subnormals: fixed)
    scaled = a / Fraction(2) ** q
    m = scaled.numerator // scaled.denominator
    rem = scaled - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    with np.errstate(over="ignore"):
        return np.float32(sign * float(m) * 2.0 ** q)       # (m <= 2^24: exact in float64; 2^128 casts to infinity)


def fma_exact(code: int, scale: np.float32, bias: np.float32) -> np.float32:
    """fma(float(code), scale, bias) by rational arithmetic and IEEE's rules for the values rationals do not hold."""
    s, b = float(scale), float(bias)
    if np.isnan(s) or np.isnan(b) or (np.isinf(s) and code == 0):
        return np.float32(np.nan)
    if np.isinf(s):
        p = s                                               # code > 0
        return np.float32(np.nan) if np.isinf(b) and (b > 0) != (p > 0) else np.float32(p)
    if np.isinf(b):
        return np.float32(b)
    x = Fraction(code) * Fraction(s) + Fraction(b)
    if x == 0:      # an exact zero: the sign both terms share, +0.0 otherwise (round to nearest)
        p_neg = np.signbit(np.float32(s))                   # code >= 0: the product has the scale's sign
        return np.float32(-0.0) if (p_neg and np.signbit(np.float32(b))) else np.float32(0.0)
    return _round_to_f32(x)


def edge_pairs() -> List[tuple]:
    """(scale, bias) pairs: every edge scale with every edge bias, then rows for the named cases."""
    scales = [0.0, -0.0, -0.0371, 0.0123, SUBNORMAL, -SUBNORMAL, FLT_MAX, np.inf, -np.inf, np.nan, 2.0 ** -24, 1.0]
    biases = [0.0, -0.0, SUBNORMAL, -SUBNORMAL, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan, 1.0, -0.731]
    return [(np.float32(s), np.float32(b)) for s in scales for b in biases]


def edge_triples():
    """(codes, scales, biases), flat: all 256 codes against every edge pair, products that overflow alone but not fused,
    and results on float32 ties (1 + k * 2^-24 for odd k lies halfway between two neighbours of 1)."""
    pairs = edge_pairs()
    codes = np.tile(np.arange(256, dtype=np.int64), len(pairs))
    scales = np.repeat(np.asarray([p[0] for p in pairs], np.float32), 256)
    biases = np.repeat(np.asarray([p[1] for p in pairs], np.float32), 256)
    extra = [(2, FLT_MAX, -FLT_MAX), (3, FLT_MAX, -FLT_MAX), (255, FLT_MAX / 200, -FLT_MAX / 4), (2, -FLT_MAX, FLT_MAX),
             (1, 2.0 ** -24, 1.0), (3, 2.0 ** -24, 1.0), (5, 2.0 ** -24, 1.0), (255, 2.0 ** -24, 1.0), (1, 2.0 ** -25, -1.0),
             (3, 2.0 ** -25, -1.0), (1, 2.0 ** -150, 0.0), (3, 2.0 ** -150, 2.0 ** -149), (129, 2.0 ** -31, 2.0 ** -8)]
    codes = np.concatenate([codes, [e[0] for e in extra]])
    scales = np.concatenate([scales, np.asarray([e[1] for e in extra], np.float32)])
    biases = np.concatenate([biases, np.asarray([e[2] for e in extra], np.float32)])
    return codes, scales, biases


# ---- variant cells ------------------------------------------------------------------------------------------------------
def variant_cells() -> List[K.Cell]:
    """Every unsharded cell of kernel_variant_cases.cells(), on q8 tables."""
    return [c for c in K.cells() if not c.sharded]


def cell_id(cell: K.Cell) -> str:
    return f"{cell.id}-tabq8"


def kernel_names() -> dict:
    """mangled-name fragment -> (kernel, V, R) of every instantiation the cells reach: fcp_tables_q8.hip holds exactly these."""
    out = {}
    for kernel, v, r, sharded in {K.instantiation(c) for c in variant_cells()}:
        assert not sharded
        frag = f"fcp_{kernel}_tabq8_kernelILi{v}E" + (f"Li{r}E" if kernel != "ragged" else "") + "E"
        out[frag] = (kernel, v, r)
    return out


@functools.lru_cache(maxsize=None)
def case_tables(key):
    """(q8 tables, their dequantised float32 form) of the variant case `key`: tables of the case's shapes, drawn."""
    seed = zlib.crc32(repr(key).encode())
    q8 = [draw_table(t.shape[0], t.shape[1], seed + i) for i, t in enumerate(K.build_case(*key).tables)]
    return q8, [dequantize(t) for t in q8]


def _oracle(key, tables, t: int):
    import fcp_oracle
    from recom_amd.ops import concat_inputs
    case = K.build_case(*key)
    inputs, symbols = case.requests[t]
    blob, offsets, shapes = concat_inputs(inputs)
    want, bad = fcp_oracle.COracle().process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, tables, symbols)
    for w in want:
        w.setflags(write=False)
    return want, bad


@functools.lru_cache(maxsize=None)
def case_expectation(key, t: int):
    """The oracle on the dequantised tables with the float32 twin: (groups, bad ids) of request t.  Computed once per
    (case, request) and shared by the cells that differ only in store policy and wide rows."""
    return _oracle(key, case_tables(key)[1], t)


def case_expectation_on(key, tables, t: int):
    """The oracle with the float32 twin on other tables of the case's shapes (not cached)."""
    return _oracle(key, tables, t)


def case_expectation_two_roundings(key, t: int):
    """The same with the tables dequantised the other way: what the expectation must NOT be confused with."""
    return _oracle(key, [two_roundings(q) for q in case_tables(key)[0]], t)


# ---- rows that are no slot-multiples of 16 bytes, with the edge list in them ------------------------------------------------
MISALIGNED_DIMS = {1: 3, 2: 6, 4: 12}           # V -> dim: 11-, 14- and 20-byte rows


@dataclasses.dataclass
class EdgeCase:
    spec: PlanSpec          # float32 twin
    table: np.ndarray       # uint8 [vocab, dim + 8]
    inputs: list
    symbols: np.ndarray


@functools.lru_cache(maxsize=None)
def edge_case(vec: int) -> EdgeCase:
    """One table of dim MISALIGNED_DIMS[vec] whose rows carry the edge pairs (each with codes that walk through all 256
    values) and the named triples, read once through a GATHER column (group 0: the dense body) and once as bags of exactly
    one id through a pooled SUM column (group 1: the ragged body).  More than 512 rows: rows straddle 128-byte lines and,
    at 11 to 20 bytes each, a 4 KiB page."""
    dim = MISALIGNED_DIMS[vec]
    pairs = edge_pairs()
    reps = -(-600 // len(pairs))
    scale = np.asarray([p[0] for p in pairs] * reps, np.float32)
    bias = np.asarray([p[1] for p in pairs] * reps, np.float32)
    vocab = scale.size
    codes = ((np.arange(vocab)[:, None] * 29 + np.arange(dim)[None, :] * 37) % 256).astype(np.uint8)
    named_c, named_s, named_b = (a[256 * len(pairs):] for a in edge_triples())
    codes = np.concatenate([codes, np.repeat(named_c[:, None], dim, 1).astype(np.uint8)])
    scale, bias = np.concatenate([scale, named_s]), np.concatenate([bias, named_b])
    vocab = scale.size
    assert vocab >= 512 and vocab * (dim + 8) > 4096
    rng = np.random.default_rng(80 + vec)
    cols = [ColumnSpec(FORM_GATHER, dim, vocab, COMBINER_NONE, IDS_I32, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 0),
            ColumnSpec(FORM_SEGMENT_REDUCE, dim, vocab, COMBINER_SUM, IDS_I64, 0, 1, 2, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 1, 0)]
    spec = PlanSpec(cols, [1, 1, 1], [4, 8, 4], 1, n_groups=2, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    inputs = [rng.permutation(vocab).astype(np.int32), rng.permutation(vocab).astype(np.int64), np.arange(vocab + 1, dtype=np.int32)]
    return EdgeCase(spec, pack(codes, scale, bias), inputs, np.asarray([vocab], np.int32))


# ---- the wide-rows decision from the q8 stride ------------------------------------------------------------------------------
WIDE_VOCAB, WIDE_DIM = 480_000_000, 1           # vocab * dim < 2^32 - 3 <= vocab * (dim + 8): 4.32 GB


def wide_rows_spec() -> PlanSpec:
    cols = [ColumnSpec(FORM_GATHER, WIDE_DIM, WIDE_VOCAB, COMBINER_NONE, IDS_I64, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 0)]
    spec = PlanSpec(cols, [1], [8], 1, n_groups=1, n_symbols=0, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    return spec


WIDE_ROWS = [0, (1 << 32) // 9 - 1, (1 << 32) // 9, (1 << 32) // 9 + 1, WIDE_VOCAB - 1]


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


def shard_spec() -> PlanSpec:
    """BASELINE's SHARD: 4000 columns x 1 M rows, dims cycling 8 / 16 / 32 / 64 (480 GB of float32 tables)."""
    return synth.model_s2(columns=4000, vocab=1_000_000, batch=4).spec
