"""fcp_table_convert (recom_amd/csrc/fcp_convert.hip): the value model restated and the rows the tests convert
(tests/test_table_convert_host.py on the CPU, tests/test_gpu_table_convert*.py on the GPU).  Test data only.

float32 -> q8 is `quantize_ref` (synth.quantize_q8): the header's sentence in NumPy float32 arithmetic, every operation rounded once.  The CPU
test holds it to quantized::embedding_bag_byte_prepack byte for byte on the families and on the edge list below; the GPU test
then compares the kernel's bytes with it.  The other three directions have their restatements already: synth.dequantize_q8
(q8 -> float32), narrow_output_cases.narrow / torch's .to() (float32 -> 16-bit), table16_cases.widen (16-bit -> float32)."""
import functools

import numpy as np

from recom_amd import synth

FLT_MAX = float(np.finfo(np.float32).max)
KINDS = {"f32": 0, "bf16": 1, "f16": 2, "q8": 3}              # FCP_TAB_*

# The quantiser keeps kQSlots = 4 slots of V elements per lane of a 64-lane group in registers: dims above 64 * 4 * V are
# read a second time (fcp_convert.hip).
Q_SLOTS = 4
REGISTER_CAP = {v: 64 * Q_SLOTS * v for v in (1, 2, 4)}        # 256, 512, 1024
# every lane-group size on both sides of its edge, the register cap crossed in each V, V = 1, 2, 4 all occurring
QUANT_DIMS = (1, 2, 3, 4, 5, 7, 8, 12, 16, 20, 31, 32, 33, 64, 68, 128, 252, 256, 260, 1000, 1001,
              REGISTER_CAP[4] + 4, REGISTER_CAP[2] + 2, REGISTER_CAP[1] + 1, 255, 258, 510)
QUANT_ROWS = (1, 2, 63, 64, 65, 257, 1000)


def vec_of(dim: int) -> int:
    return 4 if dim % 4 == 0 else 2 if dim % 2 == 0 else 1


def group_of(dim: int) -> int:
    """Lanes that share a row in the quantiser: 1 for dims <= 4, else the power of two holding dim / V slots, at most 64."""
    if dim <= 4:
        return 1
    g = 1
    while g < dim // vec_of(dim) and g < 64:
        g <<= 1
    return g


# ---- float32 -> q8 -------------------------------------------------------------------------------------------------------
def quantize_ref(x: np.ndarray) -> np.ndarray:
    """uint8 [rows, dim + 8] of float32 [rows, dim] with finite rows: synth.quantize_q8 — per row, in float32 with every
    operation rounded once, mn = min, mx = max, R = mx - mn, scale = R / 255, inv = 255 / (R + 1e-8),
    code = rint((x - mn) * inv) to even; the codes, then scale, then mn."""
    return synth.quantize_q8(x)


def error_bound(x: np.ndarray) -> np.ndarray:
    """float64 [rows]: the bound on |dequantised - x| of a row with R > 0 (test_table_convert_host.py derives it):
    0.5 * scale + 1e-8 + 2^-22 * max(|mn|, |mx|)."""
    x = np.ascontiguousarray(x, np.float32)
    mn, mx = x.min(axis=1), x.max(axis=1)
    scale = ((mx - mn).astype(np.float32) / np.float32(255.0)).astype(np.float64)
    return 0.5 * scale + 1e-8 + 2.0 ** -22 * np.maximum(np.abs(mn), np.abs(mx)).astype(np.float64)


# ---- row families ------------------------------------------------------------------------------------------------------
def family_rows(dim: int, rows: int, seed: int) -> np.ndarray:
    """`rows` rows of width `dim`, the five families in turn: Gaussian values, values near 5 with a 1e-3 spread, small
    integers (ties, repeated values), magnitudes of 1e30, constant rows (R = 0: scale 0, codes 0)."""
    rng = np.random.default_rng(seed * 7919 + dim)
    out = np.empty((rows, dim), np.float32)
    for r in range(rows):
        f = r % 5
        if f == 0:
            out[r] = rng.standard_normal(dim)
        elif f == 1:
            out[r] = 5.0 + 1e-3 * rng.standard_normal(dim)
        elif f == 2:
            out[r] = rng.integers(-3, 4, dim)
        elif f == 3:
            out[r] = 1e30 * rng.standard_normal(dim)
        else:
            out[r] = (0.0, -1.5, 3.25e-5, 7e20, -2.0 ** -130)[(r // 5) % 5]
    return out


def _fill(dim: int, lo: float, hi: float, inner, lo_at_end: bool = False) -> np.ndarray:
    """One row: lo and hi at the first and the last element (or the other way round), `inner` cycled in between.  dim 1
    holds lo alone, dim 2 lo and hi."""
    row = np.empty(dim, np.float32)
    inner = np.asarray(inner, np.float32)
    if dim > 2:
        row[1:-1] = inner[np.arange(dim - 2) % len(inner)]
    row[0], row[-1] = (hi, lo) if lo_at_end else (lo, hi)
    if dim == 1:
        row[0] = lo
    return row


@functools.lru_cache(maxsize=None)
def edge_rows(dim: int) -> np.ndarray:
    """The hand-made edge list at width `dim`:
      * a tie at every half-integer code: rows with mn = 0, mx = 255 (scale 1, inv 1) whose other elements walk through
        k + 0.5, k = 0 .. 254 — rint goes to the even neighbour;
      * min / max at the first and at the last element, both ways round;
      * R subnormal (every code 0: inv = 255 / 1e-8 cannot lift a subnormal to 0.5), R on both sides of the 1e-8 in the
        denominator, where inv is far from 255 / R;
      * R near FLT_MAX / 2 and just below FLT_MAX: nothing overflows."""
    rows = []
    ties = np.arange(255, dtype=np.float32) + np.float32(0.5)
    per_row = max(dim - 2, 1)
    for s in range(0, 255 if dim > 2 else 1, per_row):
        rows.append(_fill(dim, 0.0, 255.0, np.roll(ties, -s)))
    rng = np.random.default_rng(4000 + dim)
    g = np.clip(rng.standard_normal(max(dim, 3)), -2.5, 2.5)
    rows.append(_fill(dim, -3.0, 3.0, g))
    rows.append(_fill(dim, -3.0, 3.0, g, lo_at_end=True))
    rows.append(_fill(dim, 2.0, 1027.0, 2.0 + 1025.0 * rng.random(max(dim, 3)), lo_at_end=True))
    sub = np.float32(2.0 ** -149)
    rows.append(_fill(dim, 0.0, float(sub * 1000), sub * rng.integers(0, 1001, max(dim, 3)).astype(np.float32)))
    rows.append(_fill(dim, float(-sub * 7), float(sub * 3), sub * rng.integers(-7, 4, max(dim, 3)).astype(np.float32)))
    for r in (0.5e-8, 0.9e-8, 1.0e-8, 1.1e-8, 2e-8, 1e-7):
        rows.append(_fill(dim, 0.0, r, r * rng.random(max(dim, 3))))
        rows.append(_fill(dim, 1.0, 1.0 + 16 * r, 1.0 + 16 * r * rng.random(max(dim, 3)), lo_at_end=True))
    for lo, hi in ((-FLT_MAX / 4, FLT_MAX / 4), (0.0, FLT_MAX / 2), (-FLT_MAX / 2, FLT_MAX * 0.49), (-FLT_MAX, -FLT_MAX / 2),
                   (FLT_MAX / 2, FLT_MAX)):
        rows.append(_fill(dim, lo, hi, lo + (hi - lo) * rng.random(max(dim, 3))))
    out = np.stack(rows).astype(np.float32)
    assert np.isfinite(out).all() and np.isfinite(out.max(axis=1) - out.min(axis=1)).all()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def quant_rows(dim: int, rows: int = max(QUANT_ROWS)) -> np.ndarray:
    """float32 [rows, dim]: the edge list (at most a third of the rows) and the families, shuffled with a fixed seed so that a
    prefix of any length holds both."""
    edges = edge_rows(dim)[:rows // 3]
    fam = family_rows(dim, rows - len(edges), 1)
    out = np.concatenate([edges, fam])[np.random.default_rng(dim).permutation(rows)]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def quant_expectation(dim: int) -> np.ndarray:
    """quantize_ref(quant_rows(dim)): computed once per dim, shared by every row count (rows are independent)."""
    out = quantize_ref(quant_rows(dim))
    out.setflags(write=False)
    return out


# ---- 64-bit offsets: a closed form on the device ---------------------------------------------------------------------------
BIG_ROWS, BIG_DIM = (1 << 24) + 3, 64           # 4.29 GB of float32, 1.21 GB of q8


def big_rows_numpy(rows: np.ndarray) -> np.ndarray:
    """float32 [len(rows), BIG_DIM]: element e of row r is ((r * 131 + e * 31) mod 1021 - 510) / 64 — exact in float32, so the
    device fills the table with the same integers (big_rows_torch) and the same division by a power of two."""
    r = np.asarray(rows, np.int64)[:, None]
    e = np.arange(BIG_DIM, dtype=np.int64)[None, :]
    return (((r * 131 + e * 31) % 1021 - 510).astype(np.float32) / np.float32(64.0)).astype(np.float32)


def big_rows_torch(torch, device):
    out = torch.empty((BIG_ROWS, BIG_DIM), dtype=torch.float32, device=device)
    e = torch.arange(BIG_DIM, device=device, dtype=torch.int64)[None, :]
    chunk = 1 << 20
    for s in range(0, BIG_ROWS, chunk):
        r = torch.arange(s, min(s + chunk, BIG_ROWS), device=device, dtype=torch.int64)[:, None]
        out[s:s + chunk] = ((r * 131 + e * 31) % 1021 - 510).to(torch.float32) / 64.0
    return out
