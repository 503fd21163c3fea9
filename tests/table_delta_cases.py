"""fcp_table_delta_distinct (recom_amd/csrc/fcp_table_delta.hip): the value model restated in NumPy, the kernels' geometry
mirrored by name, and the id patterns of tests/test_table_delta_host.py (CPU), tests/test_gpu_table_delta.py and
tests/test_zzz_gpu_table_delta_stream.py (GPU).  Test data only.

The value model: an id is inside the table when its 64-bit value, read unsigned, is below table_rows; position i wins when its
id is inside and no later position holds the same id; the winners stay in ascending position."""
import functools

import numpy as np

# the kernels' constants (fcp_table_delta.hip)
THREADS = 256                      # kDeltaThreads
TILE = THREADS                     # kDeltaTile: positions of one step of a classify / compact block
BLOCKS = 1024                      # kDeltaBlocks: the fixed grid of classify / compact
MIN_CHUNK_TILES = 4                # kDeltaMinChunkTiles
MIN_CHUNK = MIN_CHUNK_TILES * TILE  # the chunk of a block while the grid is not full
FULL_PASS = BLOCKS * MIN_CHUNK     # positions the fixed grid holds at the smallest chunk; one more and the chunk grows
INSERT_TILE = 4 * THREADS          # kDeltaInsertTile: positions of one step of an insert block
LDS_SLOTS = 2048                   # kDeltaSlots (FCP_DELTA_SLOTS): cells of an insert block's LDS table; home slot = row mod LDS_SLOTS
PROBES = 4                         # kDeltaProbes: LDS cells a row looks at before it goes to the global table
MIN_CELLS = 64                     # kDeltaMinCells
HASH_MUL = 0x9E3779B97F4A7C15      # kDeltaHashMul
PARTIAL_BYTES = (BLOCKS + 1) * 32  # the blocks' records and the totals
INT64_MIN = -(1 << 63)
LIMIT = 2 ** 32 - 3                # n and table_rows stay below it

# n: one id, two, a wave -+ 1, one tile -+ 1, one chunk -+ 1, one full pass of the fixed grid + 1
SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, MIN_CHUNK - 1, MIN_CHUNK, MIN_CHUNK + 1, FULL_PASS + 1)
BIG_ROWS = 3 * PROBES * LDS_SLOTS + 5    # more rows than the LDS table has cells: 3 * PROBES rows share every home slot; odd


def cells_for(n: int) -> int:
    """cells of the global hash table: a power of two, at least 2 n and MIN_CELLS"""
    cells = MIN_CELLS
    while cells < 2 * n:
        cells <<= 1
    return cells


def workspace_bytes(n: int) -> int:
    return PARTIAL_BYTES + 8 * cells_for(n) + (n + 7) // 8 * 8


def chunk_for(n: int) -> int:
    """positions of one block of the classify / compact grid"""
    tiles = (n + TILE - 1) // TILE
    return max(MIN_CHUNK_TILES, (tiles + BLOCKS - 1) // BLOCKS) * TILE


def home_of(rows, cells: int) -> np.ndarray:
    """home cell of each row: the top log2(cells) bits of row * HASH_MUL modulo 2^64"""
    rows = np.asarray(rows).astype(np.uint64)
    shift = np.uint64(64 - (cells.bit_length() - 1))
    with np.errstate(over="ignore"):
        return ((rows * np.uint64(HASH_MUL)) >> shift).astype(np.int64)


def distinct_ref(ids, table_rows: int):
    """(pos, report, ids_out, pos_out) of the ids (any integer dtype, 1-D; int32 widens with its sign): `pos` int64 [m], the
    winning positions in ascending order; `report` the dict {n, distinct, duplicates, skipped}; `ids_out` / `pos_out` int64 [n],
    the winners' ids / positions and -1 behind them."""
    ids = np.asarray(ids).astype(np.int64).ravel()
    n = len(ids)
    inside = ids.view(np.uint64) < np.uint64(table_rows)
    p = np.flatnonzero(inside)
    _u, first = np.unique(ids[p][::-1], return_index=True)        # the first occurrence from behind = the last
    pos = np.sort(p[len(p) - 1 - first]).astype(np.int64)
    m = len(pos)
    report = {"n": n, "distinct": m, "duplicates": len(p) - m, "skipped": n - len(p)}
    ids_out, pos_out = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    ids_out[:m], pos_out[:m] = ids[pos], pos
    return pos, report, ids_out, pos_out


def apply_ref(table_f32: np.ndarray, ids, rows: np.ndarray) -> np.ndarray:
    """the float32 master with the delta applied one position after the other; ids outside the table skipped"""
    out = np.array(table_f32, np.float32, copy=True)
    for i, r in enumerate(np.asarray(ids).astype(np.int64).tolist()):
        if 0 <= r < out.shape[0]:
            out[r] = rows[i]
    return out


# ---- id patterns ---------------------------------------------------------------------------------------------------------
PATTERNS = ("distinct", "equal", "twice_reversed", "zipf", "lds_congruent", "global_congruent", "hot_head")
REPEATING = ("equal", "twice_reversed", "zipf", "lds_congruent", "global_congruent", "hot_head")   # duplicates > 0 from n = 2 on ...
CONGRUENT_ROWS = 3 * PROBES        # distinct rows of the two congruent patterns (where the table has as many)


def global_rows(n: int) -> int:
    """rows of a table in which more than PROBES rows share one home cell of the global table a delta of n ids gets: the
    multiplicative hash deals consecutive rows out almost evenly, about table_rows / cells to a cell"""
    return max(BIG_ROWS, 8 * cells_for(n))


def table_rows_options(n: int, pattern: str) -> list:
    """the table sizes a pattern is drawn in at n ids: 1, 2, n / 2 and more rows than the LDS table has cells; besides them
    the table the pattern is FOR (global_congruent: one with chains; hot_head: one where all but the head is distinct).  A
    table of fewer than n rows cannot hold n distinct ids, so `distinct` takes, in place of the smaller ones, the table of
    exactly n rows (every row named once) and one of 2 n rows and more (hot_rows) — at least two tables at every n."""
    base = sorted({1, 2, max(n // 2, 1), BIG_ROWS})
    if pattern == "distinct":
        return sorted({r for r in base if r >= n} | {n, hot_rows(n)})
    return sorted(set(base) | {"global_congruent": {global_rows(n)}, "hot_head": {hot_rows(n)}}.get(pattern, set()))


def hot_rows(n: int) -> int:
    """rows of a table in which hot_head's ids, but for the head, are distinct"""
    return max(BIG_ROWS, 2 * n)


@functools.lru_cache(maxsize=None)
def global_congruent_rows(n: int, table_rows: int) -> np.ndarray:
    """up to CONGRUENT_ROWS rows of the table that share the home cell of row 0 in the global table a delta of n ids gets: a
    probe chain as long as there are rows (found by looking at every row of the first 8 * cells)"""
    cells, found = cells_for(n), []
    for lo in range(0, min(table_rows, 8 * cells), 1 << 22):
        cand = np.arange(lo, min(lo + (1 << 22), table_rows, 8 * cells), dtype=np.int64)
        found.append(cand[home_of(cand, cells) == 0])
    return np.concatenate(found)[:CONGRUENT_ROWS]


def draw_ids(pattern: str, n: int, table_rows: int, seed: int = 0) -> np.ndarray:
    """int64 [n], every id inside the table.
      distinct          a permutation prefix of the table (table_rows >= n): nothing repeats;
      equal             one row, the table's last: the winner is position n - 1;
      twice_reversed    n // 2 distinct rows, then the same rows in reverse order (n odd: one more row in the middle);
      zipf              numpy's Zipf(1.05) folded into the table;
      lds_congruent     rows k * LDS_SLOTS, k over CONGRUENT_ROWS values: one home slot of the LDS table, PROBES cells claimed
                        by probing, the other rows on the fall-through path;
      global_congruent  rows that share one home cell of the global table: a long probe chain there;
      hot_head          a permutation prefix with every fourth position replaced by row 0."""
    rng = np.random.default_rng(3000 + seed)
    if pattern == "distinct":
        assert table_rows >= n
        return rng.permutation(table_rows)[:n].astype(np.int64) if table_rows <= 4 * n + 1024 else \
            np.unique(rng.integers(0, table_rows, 2 * n + 64, dtype=np.int64))[:n][rng.permutation(n)]
    if pattern == "equal":
        return np.full(n, table_rows - 1, np.int64)
    if pattern == "twice_reversed":
        half = draw_ids("distinct", n // 2, max(table_rows, n // 2), seed) % table_rows
        mid = np.asarray([table_rows // 2] * (n % 2), np.int64)
        return np.concatenate([half, mid, half[::-1]]).astype(np.int64)
    if pattern == "zipf":
        return ((rng.zipf(1.05, size=n).astype(np.int64) - 1) % table_rows).astype(np.int64)
    if pattern == "lds_congruent":
        k = min(CONGRUENT_ROWS, (table_rows + LDS_SLOTS - 1) // LDS_SLOTS)
        return (rng.integers(0, k, n, dtype=np.int64) * LDS_SLOTS).astype(np.int64)
    if pattern == "global_congruent":
        rows = global_congruent_rows(n, table_rows)
        return rows[rng.integers(0, len(rows), n)].astype(np.int64)
    if pattern == "hot_head":
        ids = draw_ids("distinct", n, max(table_rows, n), seed) % table_rows
        ids[::4] = 0
        return ids.astype(np.int64)
    raise ValueError(pattern)


def outside_ids(table_rows: int) -> np.ndarray:
    """int64: the ids outside the table the issue names, each next to one inside — and every inside id also BEHIND an outside
    id whose low 32 bits are its own (2^32 + row), so that an outside id that shadowed a valid one would show"""
    last = table_rows - 1
    return np.asarray([last, 2 ** 32 + last, -1, 0, table_rows, last, 2 ** 32, INT64_MIN, 0, 2 ** 32 + last, 2 ** 63 - 1, -2 ** 31,
                       2 ** 32 + 0], np.int64)


def outside_ids32(table_rows: int) -> np.ndarray:
    """int32: negative ids (sign-extended: outside) around ids inside"""
    last = min(table_rows - 1, 2 ** 31 - 1)
    return np.asarray([last, -1, 0, -2 ** 31, last, -(last + 1), 0, -7], np.int32)


# ---- rows ----------------------------------------------------------------------------------------------------------------
ROW_DIMS = (1, 2, 3, 4, 6, 62, 64, 300)      # every V, G = 1 and the groups, and beyond one 64-lane group's reach (300 > 64 * 4)


def special_rows(n: int, dim: int, seed: int = 0) -> np.ndarray:
    """float32 [n, dim] whose bits matter: random bit patterns (NaN payloads of both signs, subnormals, infinities among them)
    with -0.0, a quiet and a signalling NaN with payloads, and the smallest subnormal at fixed places; row i's first word is
    also different from every other row's, so a row copied from the wrong position shows."""
    rng = np.random.default_rng(4000 + seed)
    w = rng.integers(0, 2 ** 32, (n, dim), dtype=np.uint64).astype(np.uint32)
    fixed = np.asarray([0x80000000, 0x7FC12345, 0xFF800001, 0x00000001, 0x807FFFFF], np.uint32)
    flat = w.reshape(-1)
    flat[1::7] = fixed[np.arange(len(flat[1::7])) % len(fixed)]
    if dim >= 2:                 # (dim 1 keeps the fixed words; its random words tell the rows apart)
        w[:, 0] = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2 ** 32)).astype(np.uint32)
    return w.view(np.float32)
