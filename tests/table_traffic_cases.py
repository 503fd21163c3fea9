"""fcp_table_count_ids / fcp_table_audit_weighted (recom_amd/csrc/fcp_table_traffic.hip, fcp_table_audit.hip): the value models
restated, the kernel's constants, and the id streams of tests/test_table_traffic_host.py (CPU) and
tests/test_gpu_table_traffic.py (GPU).  Test data only.

Counting is np.bincount modulo 2^32 over the ids inside [0, table_rows), the others counted as skipped.  The weighted audit is
table_audit_cases.aggregate with the three kinds of sums replaced by sum_r w_r * (row r's float64 sum), from the same per-row
`sq` and `sse` (table_audit_cases.row_stats); every field that decides admissibility is the unweighted aggregate's."""
import numpy as np

import table_audit_cases as TA

# the kernel's constants (fcp_table_traffic.hip)
GRID_BLOCKS = 256                  # kCountBlocks: the fixed grid
BLOCK_THREADS = 1024               # kCountThreads
IDS_PER_THREAD = 4                 # kIdsPerThread
TILE_IDS = BLOCK_THREADS * IDS_PER_THREAD   # kTileIds: ids of one step of a block's stride loop — a block's share of one grid pass
SLOTS = 16384                      # kCountSlots: cells of a block's LDS table; home slot = row mod SLOTS
PROBES = 4                         # kCountProbes: cells a row looks at before it goes to memory itself
INT64_MIN = -2 ** 63

# n: one id, a wave -+ 1, four waves -+ 1, a block's threads -+ 1, one block's share (a tile) -+ 1, one full pass of the grid + 1
SIZES = (1, 63, 64, 65, 255, 256, 257, BLOCK_THREADS - 1, BLOCK_THREADS, BLOCK_THREADS + 1, TILE_IDS - 1, TILE_IDS, TILE_IDS + 1,
         GRID_BLOCKS * TILE_IDS + 1)
BIG_VOCAB = 200003                 # more rows than the LDS table has cells (3 * PROBES home-slot-sharing rows fit), and odd


def count_ref(table_rows: int, ids, start=None):
    """(uint32 [table_rows], skipped): `start` (uint32, default zeros) plus the occurrences of every row among `ids` (any
    integer dtype, any shape; int32 widens with its sign), modulo 2^32; ids outside [0, table_rows) are counted as skipped."""
    ids = np.asarray(ids).astype(np.int64).ravel()
    inside = (ids >= 0) & (ids < table_rows)
    add = np.bincount(ids[inside], minlength=table_rows).astype(np.uint64)
    base = np.zeros(table_rows, np.uint64) if start is None else np.asarray(start, np.uint32).astype(np.uint64)
    return ((base + add) & np.uint64(0xFFFFFFFF)).astype(np.uint32), int((~inside).sum())


def draw_ids(pattern: str, n: int, table_rows: int, seed: int = 0) -> np.ndarray:
    """int64 [n], every id inside the table.
      equal      one row, the table's last;
      uniform    rng.integers;
      zipf       numpy's Zipf(1.05) folded into the table (synth's `--ids zipf`);
      distinct   i mod table_rows: with table_rows > n, every id another row — a block's share of more than SLOTS ids overflows
                 its LDS table, and tiles a grid pass apart share home slots (GRID_BLOCKS * TILE_IDS is a multiple of SLOTS);
      congruent  rows k * SLOTS, k cycling over 3 * PROBES values (as many as the table has): one home slot, PROBES cells
                 claimed by probing, the other rows on the fall-through path."""
    rng = np.random.default_rng(1000 + seed)
    if pattern == "equal":
        return np.full(n, table_rows - 1, np.int64)
    if pattern == "uniform":
        return rng.integers(0, table_rows, n, dtype=np.int64)
    if pattern == "zipf":
        return ((rng.zipf(1.05, size=n).astype(np.int64) - 1) % table_rows).astype(np.int64)
    if pattern == "distinct":
        return (np.arange(n, dtype=np.int64) % table_rows).astype(np.int64)
    if pattern == "congruent":
        k = min(3 * PROBES, (table_rows + SLOTS - 1) // SLOTS)
        return (rng.integers(0, k, n, dtype=np.int64) * SLOTS).astype(np.int64)
    raise ValueError(pattern)


PATTERNS = ("equal", "uniform", "zipf", "distinct", "congruent")


def outside_ids(table_rows: int) -> np.ndarray:
    """int64: the ids outside the table the issue names, each next to one inside"""
    return np.asarray([-1, 0, table_rows, table_rows - 1, 2 ** 32 + (table_rows - 1), 2 ** 32, INT64_MIN, 0, 2 ** 63 - 1, -2 ** 31], np.int64)


def weighted_aggregate(stats: dict, idx, counts) -> dict:
    """table_audit_cases.aggregate of the table whose row r is row idx[r] of the judged array, its sums weighted by counts[r]
    (uint32): numpy's float64 sum of w_r * the row's float64 sum.  The rows' sums are 0 where the audit leaves a row out."""
    idx = np.asarray(idx, np.int64)
    w = np.asarray(counts, np.uint32).astype(np.float64)
    assert w.shape == idx.shape
    out = TA.aggregate(stats, idx)
    out["sum_sq"] = float((w * stats["sq"][idx]).sum())
    for kind in TA.COMPACT:
        out[kind]["sum_sq_err"] = float((w * stats[kind]["sse"][idx]).sum())
    return out


def draw_counts(rows: int, seed: int) -> np.ndarray:
    """uint32 [rows]: random over the whole range, a third of them 0, with 2^32 - 1 and 0 at fixed places (rows >= 3)"""
    rng = np.random.default_rng(2000 + seed)
    c = rng.integers(0, 2 ** 32, rows, dtype=np.uint64).astype(np.uint32)
    c[rng.random(rows) < 1 / 3] = 0
    if rows >= 3:
        c[rows // 2], c[rows // 3] = 0xFFFFFFFF, 0
    elif rows:
        c[0] = 0xFFFFFFFF
    return c
