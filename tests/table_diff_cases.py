"""fcp_table_diff (recom_amd/csrc/fcp_table_diff.hip): the value model restated in NumPy, the kernels' geometry mirrored by name,
and the change patterns of tests/test_table_diff_host.py (CPU), tests/test_gpu_table_diff.py and
tests/test_zzz_gpu_table_diff_stream.py (GPU).  Test data only.

The value model: table row row0 + i is CHANGED when the bytes fcp_table_convert's value model gives row i of the source differ,
in any byte, from the bytes stored.  The bytes come from synth.quantize_q8 (q8), narrow_output_cases.narrow (bf16 / fp16) and
a plain view (float32) — the restatements the convert tests hold the kernels to."""
import functools

import numpy as np

import narrow_output_cases as N
from recom_amd import synth

# the kernels' constants (fcp_table_diff.hip)
THREADS = 256                      # kDiffThreads
TILE = THREADS                     # kDiffTile: rows of one step of a compact block
BLOCKS = 2048                      # kDiffBlocks: the fixed grid of classify / compact
MIN_CHUNK_TILES = 4                # kDiffMinChunkTiles
MIN_CHUNK = MIN_CHUNK_TILES * TILE  # the chunk of a block while the grid is not full
FULL_PASS = BLOCKS * MIN_CHUNK     # rows the fixed grid holds at the smallest chunk; one more and the chunk grows
PARTIAL_BYTES = (BLOCKS + 1) * 32  # the blocks' records and the totals
LIMIT = 2 ** 32 - 3                # rows and table_rows stay below it
INT64_MIN = -(1 << 63)
Q_SLOTS = 4                        # kQSlots (fcp_table_walk.h): slots a lane of a 64-lane group keeps in registers

KINDS = {"f32": 0, "bf16": 1, "f16": 2, "q8": 3}   # FCP_TAB_*
COMPACT = ("bf16", "f16", "q8")
# every V, G = 1, every group size, beyond the 64-lane reach (300 = 75 slots of 4) and beyond the register cap (1028 > 64 * 4 * 4):
# the quantiser reads a q8 row's tail a second time there, and the classify kernel walks every format's tail in a loop
DIMS = (1, 2, 3, 4, 6, 62, 64, 300)
CAP_DIM = 64 * Q_SLOTS * 4 + 4
# one row, two, a wave -+ 1, one tile -+ 1, one chunk -+ 1; one full pass of the fixed grid + 1 (at dim <= 4 only)
ROW_COUNTS = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, MIN_CHUNK - 1, MIN_CHUNK, MIN_CHUNK + 1)
BIG_ROWS = FULL_PASS + 1
MAX_ROWS = max(ROW_COUNTS)


def dims_of(kind: str) -> tuple:
    return DIMS + (CAP_DIM,)


def workspace_bytes(rows: int) -> int:
    return PARTIAL_BYTES + (rows + 7) // 8 * 8


def chunk_for(rows: int) -> int:
    """rows of one block of the classify / compact grid"""
    tiles = (rows + TILE - 1) // TILE
    return max(MIN_CHUNK_TILES, (tiles + BLOCKS - 1) // BLOCKS) * TILE


def row_bytes(kind: str, dim: int) -> int:
    return {"f32": 4 * dim, "bf16": 2 * dim, "f16": 2 * dim, "q8": dim + 8}[kind]


def ref_bytes(x: np.ndarray, kind: str) -> np.ndarray:
    """uint8 [rows, row_bytes]: the bytes fcp_table_convert's value model gives the float32 rows x in format `kind`"""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "q8":
        return synth.quantize_q8(x)
    if kind == "f32":
        return x.view(np.uint8).reshape(x.shape[0], -1).copy()
    return np.ascontiguousarray(N.narrow(x, kind)).view(np.uint8).reshape(x.shape[0], -1).copy()


def diff_ref(new_bytes: np.ndarray, stored: np.ndarray, row0: int = 0):
    """(ids, report, ids_out) of the format's bytes of the new rows against the stored bytes of table rows row0 .. : `ids` int64
    [m], ascending table row indices; `report` the dict of fcp_table_diff_report_t; `ids_out` int64 [rows], -1 behind the ids."""
    assert new_bytes.shape == stored.shape and new_bytes.dtype == stored.dtype == np.uint8
    ids = (np.flatnonzero((new_bytes != stored).any(axis=1)) + row0).astype(np.int64)
    rows, m = len(stored), len(ids)
    report = {"rows": rows, "changed": m, "first_changed": int(ids[0]) if m else -1, "last_changed": int(ids[-1]) if m else -1}
    ids_out = np.full(rows, -1, np.int64)
    ids_out[:m] = ids
    return ids, report, ids_out


# ---- masters ---------------------------------------------------------------------------------------------------------------
def base_rows(rows: int, dim: int, seed: int = 0) -> np.ndarray:
    """float32 [rows, dim], four families in turn (vectorised: the big row count draws it too): Gaussian values, values near 5
    with a 1e-3 spread, small integers (ties, repeated values), constant rows (q8: R = 0, scale 0, codes 0)."""
    rng = np.random.default_rng(7000 + 131 * seed + dim)
    g = rng.standard_normal((rows, dim)).astype(np.float32)
    out = np.empty((rows, dim), np.float32)
    f = np.arange(rows) % 4
    out[f == 0] = g[f == 0]
    out[f == 1] = np.float32(5.0) + np.float32(1e-3) * g[f == 1]
    # (+ 0.0: rint gives -0.0 too, and the sign of a zero min in a q8 row with zeros of both signs is unspecified)
    out[f == 2] = np.rint(np.float32(2.0) * g[f == 2]) + np.float32(0.0)
    out[f == 3] = np.asarray([0.0, -1.5, 3.25e-5, 12.0, -2.0 ** -20], np.float32)[(np.arange(rows)[f == 3] // 4) % 5][:, None]
    return out


def grid_rows(rows: int, dim: int, seed: int = 0) -> np.ndarray:
    """float32 [rows, dim] for the QUIET pattern: whole numbers in [2, 255] between a 1 at the first and a 256 at the last
    element (dim >= 2).  Every value is exact in bf16 and fp16 (eight significant bits), non-zero, and — the row's range being
    255, scale 1 and inv 1 — sits exactly ON its q8 code, as far from a tie as a value can be; a nudge upwards of an interior
    element moves neither the row's min nor its max."""
    rng = np.random.default_rng(8000 + 131 * seed + dim)
    out = rng.integers(2, 256, (rows, dim)).astype(np.float32)
    if dim >= 2:
        out[:, 0], out[:, -1] = 1.0, 256.0
    return out


def loud(x: np.ndarray, last_element_only: bool = False, double: bool = False) -> np.ndarray:
    """every row changed so that every format sees it: + 1.0 on one element — the last, or element (row index) mod dim.  (q8:
    the element's code moves, or the row's range and with it scale or bias.)  `double`: the element times 2 instead, for
    grid_rows, whose 256 + 1 is 256 again in bf16."""
    out = np.array(x, np.float32, copy=True)
    rows, dim = out.shape
    j = np.full(rows, dim - 1) if last_element_only else np.arange(rows) % dim
    if double:
        out[np.arange(rows), j] *= np.float32(2.0)
    else:
        out[np.arange(rows), j] += np.float32(1.0)
    return out


def quiet(x: np.ndarray) -> np.ndarray:
    """every row of grid_rows perturbed in its float32 BITS and in no format's bytes: 1 .. 255 added to the bit pattern of one
    element — an interior one where the row has any (dim >= 3), so that a q8 row keeps its min and max.  The value rises by
    less than 2^-15 of itself: far below half an ulp of bf16 (2^-9) and fp16 (2^-12), and by less than 0.008 of a q8 code step."""
    out = np.array(x, np.float32, copy=True)
    rows, dim = out.shape
    i = np.arange(rows)
    j = 1 + i % (dim - 2) if dim >= 3 else i % dim
    out.view(np.uint32)[i, j] += (1 + i % 255).astype(np.uint32)
    return out


def quiet_dims(kind: str) -> tuple:
    """a q8 row of dim <= 2 has no interior element: its only values are the bias and the range"""
    return tuple(d for d in dims_of(kind) if kind != "q8" or d >= 3)


# ---- change patterns -------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "all", "first", "last", "every3", "tile_edges", "last_element", "quiet")


def mask_of(pattern: str, rows: int) -> np.ndarray:
    """bool [rows]: the rows a pattern takes from its changed variant (quiet: even rows QUIET, odd rows LOUD — see variants)"""
    i = np.arange(rows)
    if pattern == "none":
        return np.zeros(rows, bool)
    if pattern in ("all", "quiet"):
        return np.ones(rows, bool)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == rows - 1
    if pattern == "every3":
        return i % 3 == 1
    if pattern == "tile_edges":          # the last row of every tile and the first row of the next one
        return (i % TILE == TILE - 1) | ((i % TILE == 0) & (i > 0))
    if pattern == "last_element":
        return i % 2 == 0
    if pattern == "wave_edges":          # the last row of every wave and the first row of the next one: every tile's edges too
        return (i % WAVE == WAVE - 1) | ((i % WAVE == 0) & (i > 0))
    raise ValueError(pattern)


# The selection's own edges (fcp_select_compact.h serves the delta too): nothing, everything, and rows on both sides of every
# wave and tile boundary — at float32 against float32, the cheapest classify, with rows_out at V 4 / G 1 and at V 2 / G 4 —
# over the delta's size list: ROW_COUNTS, and BIG_ROWS at the V 4 dim alone.
WAVE = 64
EDGE_PATTERNS = ("none", "all", "wave_edges")
EDGE_DIMS = (4, 6)
EDGE_ROW_COUNTS = ROW_COUNTS + (BIG_ROWS,)


class Variants:
    """What every pattern of one (kind, dim) is cut from, computed ONCE at `rows` rows (rows are independent: a prefix serves
    every smaller count): the base master and its stored bytes, and the changed variants with THEIR bytes."""

    def __init__(self, kind: str, dim: int, rows: int = MAX_ROWS, seed: int = 0):
        self.kind, self.dim, self.rows = kind, dim, rows
        base, grid = base_rows(rows, dim, seed), grid_rows(rows, dim, seed)
        mixed = quiet(grid)
        odd = np.arange(rows) % 2 == 1
        mixed[odd] = loud(grid, double=True)[odd]
        self.src = {"base": base, "loud": loud(base), "last_element": loud(base, last_element_only=True), "grid": grid, "quiet": mixed}
        self.bytes = {k: ref_bytes(v, kind) for k, v in self.src.items()}
        for v in list(self.src.values()) + list(self.bytes.values()):
            v.setflags(write=False)

    def case(self, pattern: str, rows: int):
        """(base master, its stored bytes, new master, its bytes in the format) of `pattern` at `rows` rows"""
        assert rows <= self.rows
        base, changed = ("grid", "quiet") if pattern == "quiet" else ("base", "last_element" if pattern == "last_element" else "loud")
        mask = mask_of(pattern, rows)
        new = np.where(mask[:, None], self.src[changed][:rows], self.src[base][:rows])
        new_bytes = np.where(mask[:, None], self.bytes[changed][:rows], self.bytes[base][:rows])
        return self.src[base][:rows], self.bytes[base][:rows], new, new_bytes


@functools.lru_cache(maxsize=None)
def variants(kind: str, dim: int) -> Variants:
    return Variants(kind, dim)


# ---- rows whose bits matter (16-bit kinds) ---------------------------------------------------------------------------------------
def special_rows(rows: int, dim: int, seed: int = 0) -> np.ndarray:
    """float32 [rows, dim] of random bit patterns — NaNs of both signs with payloads, infinities, subnormals among them — with
    -0.0, +0.0, a quiet and a signalling NaN, +-inf and the smallest subnormal at fixed places"""
    rng = np.random.default_rng(9000 + seed)
    w = rng.integers(0, 2 ** 32, (rows, dim), dtype=np.uint64).astype(np.uint32)
    fixed = np.asarray([0x80000000, 0x00000000, 0x7FC12345, 0xFF800001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32)
    flat = w.reshape(-1)
    flat[1::5] = fixed[np.arange(len(flat[1::5])) % len(fixed)]
    return w.view(np.float32)


def special_changes(x: np.ndarray, seed: int = 0) -> np.ndarray:
    """the rows of special_rows, by row index mod 4: untouched; one element's sign flipped (-0.0 for +0.0 among them); the low
    mantissa bit of one element flipped (mostly invisible in 16 bits; a NaN's payload bit among them); a new random row"""
    rng = np.random.default_rng(9500 + seed)
    out = np.array(x, np.float32, copy=True)
    w = out.view(np.uint32)
    rows, dim = w.shape
    i = np.arange(rows)
    j = i % dim
    w[i[i % 4 == 1], j[i % 4 == 1]] ^= np.uint32(0x80000000)
    w[i[i % 4 == 2], j[i % 4 == 2]] ^= np.uint32(1)
    w[i % 4 == 3] = rng.integers(0, 2 ** 32, (int((i % 4 == 3).sum()), dim), dtype=np.uint64).astype(np.uint32)
    return out
