"""fcp_outputs_compare: the value model restated in NumPy, the edge matrix and the calling helpers of
tests/test_outputs_compare_host.py (CPU) and tests/test_zzz_gpu_outputs_compare.py (GPU).  Test data only.

The restatement is the header's value model, one line per sentence: 16-bit sides widened exactly (table16_cases.widen, the
helper the 16-bit table and narrow-output tests use), `differ` as inequality of the float32 patterns, a pair finite when
neither element is NaN or +-inf, e = b - a one float32 subtraction, the squares as float64 products, np.sum in float64, the
maxima in float32.  The device adds the same non-negative float64 terms in another order: each of the two sums is within
n * 2^-53 of the exact sum, relative, so the two are within n * 2^-52 of each other (fcp_table_audit.hip derives it); with one
finite pair there is one term and the sums are equal."""
import ctypes as C
import functools

import numpy as np

import narrow_output_cases as N
import table16_cases as T16

KINDS = ("f32", "bf16", "f16")                 # index = FCP_OUT_*
KIND_PAIRS = [(a, b) for a in KINDS for b in KINDS]
ELEM_BYTES = {"f32": 4, "bf16": 2, "f16": 2}
RECORD = np.dtype([("elems", "<i8"), ("differ", "<i8"), ("nonfinite", "<i8"), ("first_differ_row", "<i8"),
                   ("sum_sq_ref", "<f8"), ("sum_sq_err", "<f8"), ("max_abs_err", "<f4"), ("max_abs_ref", "<f4"),
                   ("reserved", "<i8")])
FIELDS = ("elems", "differ", "nonfinite", "first_differ_row", "sum_sq_ref", "sum_sq_err", "max_abs_err", "max_abs_ref", "reserved")
EXACT_FIELDS = ("elems", "differ", "nonfinite", "first_differ_row", "max_abs_err", "max_abs_ref", "reserved")
TARGET_BLOCKS, MAX_TILES = 4096, 64


def tiles_per_column(n_columns: int) -> int:
    """T, the header's function of n_columns alone"""
    return 1 if n_columns <= 0 else min(MAX_TILES, max(1, -(-TARGET_BLOCKS // n_columns)))


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def encode(x32, kind: str) -> np.ndarray:
    """float32 values as elements of `kind`: float32 itself, or the 16-bit patterns of the values rounded once"""
    x32 = np.ascontiguousarray(x32, np.float32)
    return x32 if kind == "f32" else N.narrow(x32, kind)


def widened(elems, kind: str) -> np.ndarray:
    """float32 [rows, dim] of a column's elements: float32 as they are, 16-bit patterns widened exactly"""
    return np.ascontiguousarray(elems, np.float32) if kind == "f32" else T16.widen(elems, kind)


def restate_column(a_elems, kind_a: str, b_elems, kind_b: str) -> np.ndarray:
    """one RECORD: what fcp_outputs_compare writes for a column whose sides hold these elements"""
    a, b = widened(a_elems, kind_a), widened(b_elems, kind_b)
    assert a.shape == b.shape and a.ndim == 2
    r = np.zeros((), RECORD)
    differ = a.view(np.uint32) != b.view(np.uint32)
    finite = np.isfinite(a) & np.isfinite(b)
    with np.errstate(all="ignore"):
        e = (b - a).astype(np.float32)                       # one float32 subtraction
        ef, af = e[finite].astype(np.float64), a[finite].astype(np.float64)
        r["sum_sq_err"] = np.sum(ef * ef, dtype=np.float64)
        r["sum_sq_ref"] = np.sum(af * af, dtype=np.float64)
    r["elems"] = a.size
    r["differ"] = int(differ.sum())
    r["nonfinite"] = int((~finite).sum())
    rows = np.flatnonzero(differ.any(axis=1)) if a.size else np.zeros(0, np.int64)
    r["first_differ_row"] = int(rows[0]) if rows.size else -1
    r["max_abs_err"] = np.abs(e[finite]).max() if finite.any() else 0.0
    r["max_abs_ref"] = np.abs(a[finite]).max() if finite.any() else 0.0
    return r


def restate_total(columns: np.ndarray) -> np.ndarray:
    """the record of all columns together, folded from the column records"""
    r = np.zeros((), RECORD)
    r["first_differ_row"] = -1
    if len(columns):
        for f in ("elems", "differ", "nonfinite"):
            r[f] = int(columns[f].sum())
        with np.errstate(all="ignore"):
            for f in ("sum_sq_ref", "sum_sq_err"):
                r[f] = np.sum(columns[f], dtype=np.float64)
        for f in ("max_abs_err", "max_abs_ref"):
            r[f] = columns[f].max()
        first = columns["first_differ_row"][columns["first_differ_row"] >= 0]
        r["first_differ_row"] = int(first.min()) if first.size else -1
    return r


def restate(sides_a, kind_a: str, sides_b, kind_b: str) -> np.ndarray:
    """RECORD [n + 1] of n columns given as two lists of element arrays"""
    cols = np.array([restate_column(a, kind_a, b, kind_b) for a, b in zip(sides_a, sides_b)], RECORD).reshape(-1)
    return np.concatenate([cols, restate_total(cols).reshape(1)])


def assert_records(got: np.ndarray, want: np.ndarray, what, finite_pairs=None) -> None:
    """`got` against the restatement: counts, first rows and maxima bit for bit; the two sums within elems * 2^-52, relative
    (equal where a sum is 0 or not finite, and where the column has one finite pair)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in EXACT_FIELDS:
        g, w = got[f], want[f]
        same = g.view(np.uint32) == w.view(np.uint32) if g.dtype == np.float32 else g == w
        if not np.all(same):
            k = int(np.flatnonzero(~same)[0])
            raise AssertionError(f"{what}: field {f} of record {k}: got {g[k]!r}, want {w[k]!r}")
    for f in ("sum_sq_ref", "sum_sq_err"):
        g, w = got[f], want[f]
        bound = np.maximum(want["elems"], 1).astype(np.float64) * 2.0 ** -52
        with np.errstate(all="ignore"):
            ok = np.where(np.isfinite(w) & (w != 0), np.abs(g - w) <= bound * np.abs(w), g == w)
        if finite_pairs is not None:
            one = np.asarray(finite_pairs) == 1
            ok = ok & (~one | (g == w))
        if not np.all(ok):
            k = int(np.flatnonzero(~ok)[0])
            raise AssertionError(f"{what}: {f} of record {k}: got {g[k]!r}, want {w[k]!r}, bound {bound[k]:.3e} relative")


# ---- the edge matrix ----------------------------------------------------------------------------------------------------------
DIMS = (1, 2, 3, 4, 5, 8, 20, 63, 64, 65, 128)
ROWS = (0, 1, 2, 63, 64, 65, 257)
LAYOUTS = ("packed", "padded", "group")        # stride = dim, stride = dim + 1, stride = a group's width
SPECIALS = ("one_bit", "zeros", "nan_one_side", "equal_nans", "infs", "denormals", "largest", "equal_column")
INJECTED = SPECIALS[:-1]                       # the pairs a column carries at its corners; "equal_column" is a whole column


def is_equal_column(index: int) -> bool:
    return index % 9 == 8


def corner_special(index: int, corner: int) -> str:
    """what column `index` holds at corner 0..3 (first row / last row x first element / last element); index // 7 joins in
    because the row counts have period 7 in the column list: every row count meets every special"""
    return INJECTED[(index + index // 7 + corner) % len(INJECTED)]


MIN_DENORMAL = {"f32": 0x00000001, "bf16": 0x0001, "f16": 0x0001}
LARGEST = {"f32": 0x7F7FFFFF, "bf16": 0x7F7F, "f16": 0x7BFF}


def _value(bits: int, kind: str) -> np.float32:
    """the float32 value of one element pattern of `kind`"""
    if kind == "f32":
        return np.asarray([bits], np.uint32).view(np.float32)[0]
    return T16.widen(np.asarray([bits], np.uint16), kind)[0]


def special_pair(name: str, kind_a: str, kind_b: str, flip: bool):
    """(a, b) as float32 values, each exact in its side's kind; `flip` picks the mirrored form"""
    one, zero, nan, inf = np.float32(1.0), np.float32(0.0), np.float32(np.nan), np.float32(np.inf)
    if name == "one_bit":       # 1.0 against 1.0 with the lowest bit of b's element flipped
        b1 = int(encode([1.0], kind_b).view(np.uint32 if kind_b == "f32" else np.uint16)[0]) ^ 1
        return one, _value(b1, kind_b)
    if name == "zeros":
        return (-zero, zero) if flip else (zero, -zero)
    if name == "nan_one_side":
        return (one, nan) if flip else (nan, one)
    if name == "equal_nans":    # 0x7FC00000 on both sides, whatever the kinds (bf16 0x7FC0 and fp16 0x7E00 widen to it)
        return nan, nan
    if name == "infs":
        return (inf, -inf) if flip else (inf, inf)
    if name == "denormals":
        return _value(MIN_DENORMAL[kind_a], kind_a), _value(3 * MIN_DENORMAL[kind_b], kind_b)
    if name == "largest":       # e = b - a reaches the largest finite value of a kind: e * e up to 2^256 in float64
        return (_value(LARGEST[kind_a], kind_a), zero) if flip else (zero, _value(LARGEST[kind_b], kind_b))
    raise KeyError(name)


def edge_columns():
    """[(rows, dim, layout of side A)]: every dim x rows x layout, and two columns that span more than T and more than 2 T row
    tiles at the T of this column count (dim 1: 256 rows per tile; dim 128 on 4-byte loads: 2 rows per tile)."""
    cols = [(r, d, lay) for lay in LAYOUTS for d in DIMS for r in ROWS]
    t = tiles_per_column(len(cols) + 2)
    cols += [(t * 256 + 300, 1, "packed"), (2 * 2 * t + 701, 128, "padded")]
    assert tiles_per_column(len(cols)) == t and t > 1
    return cols


def _draw_values(rng, rows, dim, kind_a, kind_b, index):
    """float32 [rows, dim] of both sides, exact in their kinds: a drawn, b = a rounded to b's kind, a third of it perturbed;
    then the column's special pairs at its four corners"""
    a = widened(encode(rng.standard_normal((rows, dim)), kind_a), kind_a)
    noise = np.where(rng.random((rows, dim)) < 0.33, rng.standard_normal((rows, dim)) * 1e-2, 0.0)
    b = widened(encode(a + noise.astype(np.float32), kind_b), kind_b)
    if is_equal_column(index) or rows == 0:
        if kind_a != kind_b:    # values exact in every kind: eighths
            a = (np.round(a * 8) / 8).astype(np.float32)
        return a, a.copy()
    corners = [(0, 0), (0, dim - 1), (rows - 1, 0), (rows - 1, dim - 1)]
    for c, (r, j) in enumerate(corners):
        a[r, j], b[r, j] = special_pair(corner_special(index, c), kind_a, kind_b, flip=(index // len(INJECTED) + c) % 2 == 1)
    return a, b


def _place(columns, layouts, kind: str):
    """An arena for one side: [(element offset, row stride)] per column and the element count.  Packed and padded columns
    follow each other, every other one pushed to an odd element offset; the columns of the "group" layout that share a row
    count lie side by side in one matrix whose first column starts at element 1 of an odd width."""
    at, where = 8, [None] * len(columns)
    groups = {}
    for k, ((rows, dim, _), lay) in enumerate(zip(columns, layouts)):
        if lay == "group":
            groups.setdefault(rows, []).append(k)
            continue
        stride = dim if lay == "packed" else dim + 1
        at = -(-at // 4) * 4 + (k % 2)
        where[k] = (at, stride)
        at += rows * stride + 3
    for rows, ks in groups.items():
        width = 1 + sum(columns[k][1] for k in ks)
        width += 1 - width % 2
        at = -(-at // 4) * 4
        off = 1
        for k in ks:
            where[k] = (at + off, width)
            off += columns[k][1]
        at += rows * width + 3
    return where, at + 8


GAP = {"f32": 0x7FC0DEAD, "bf16": 0x7FC1, "f16": 0x7E01}   # what lies between the columns: NaN patterns no column holds


@functools.lru_cache(maxsize=None)
def edge_matrix(kind_a: str, kind_b: str):
    """dict: columns [(rows, dim)], per side the arena (NumPy array of elements), the columns' element offsets and strides and
    the element arrays, and the restated records (n + 1).  Side B's layouts are side A's rotated by one."""
    cols = edge_columns()
    rng = np.random.default_rng(KINDS.index(kind_a) * 3 + KINDS.index(kind_b))
    vals = [_draw_values(rng, r, d, kind_a, kind_b, k) for k, (r, d, _) in enumerate(cols)]
    out = {"columns": [(r, d) for r, d, _ in cols]}
    for side, kind, rot in (("a", kind_a, 0), ("b", kind_b, 1)):
        layouts = [LAYOUTS[(LAYOUTS.index(lay) + rot) % 3] for _, _, lay in cols]
        where, total = _place(cols, layouts, kind)
        dt = np.uint32 if kind == "f32" else np.uint16
        arena = np.full(total, GAP[kind], dt)
        elems = []
        for k, (r, d, _) in enumerate(cols):
            e = encode(vals[k][0 if side == "a" else 1], kind)
            elems.append(e)
            off, stride = where[k]
            view = np.lib.stride_tricks.as_strided(arena[off:], (r, d), (stride * arena.itemsize, arena.itemsize))
            view[...] = e.view(dt)
        arena.setflags(write=False)
        out[side] = {"kind": kind, "arena": arena, "where": where, "elems": elems}
    out["want"] = restate(out["a"]["elems"], kind_a, out["b"]["elems"], kind_b)
    fin = [int((np.isfinite(widened(a, kind_a)) & np.isfinite(widened(b, kind_b))).sum())
           for a, b in zip(out["a"]["elems"], out["b"]["elems"])]
    out["finite_pairs"] = np.asarray(fin + [sum(fin)])
    return out


# ---- calling the entry --------------------------------------------------------------------------------------------------------
def call(L, ptrs_a, strides_a, kind_a, ptrs_b, strides_b, kind_b, shapes, n, out, workspace, device=0, stream=0) -> int:
    """fcp_outputs_compare with host arrays built from Python sequences (None: a NULL array); kinds as names or numbers"""
    def arr(seq, ctype):
        return None if seq is None else (ctype * max(1, len(seq)))(*seq)
    ka = KINDS.index(kind_a) if isinstance(kind_a, str) else kind_a
    kb = KINDS.index(kind_b) if isinstance(kind_b, str) else kind_b
    keep = (arr(ptrs_a, C.c_void_p), arr(strides_a, C.c_int64), arr(ptrs_b, C.c_void_p), arr(strides_b, C.c_int64),
            arr(shapes, C.c_int32))
    return L.fcp_outputs_compare(keep[0], keep[1], ka, keep[2], keep[3], kb, keep[4], n, C.c_void_p(out), C.c_void_p(workspace),
                                 device, C.c_void_p(stream))
