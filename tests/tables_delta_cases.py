"""fcp_tables_delta_distinct (recom_amd/csrc/fcp_tables_delta.hip): the deal of blocks restated in Python, with the cap the
library exports, and the entry sets of tests/test_tables_delta_host.py (CPU) and tests/test_zzz_gpu_tables_delta.py (GPU).  The
value model, the id patterns and the rows are those of the single-table entry: tests/table_delta_cases.py, imported, not
copied.  Test data only.

An ENTRY here is a dict: ids (int64 or int32 NumPy array), rows (float32 [n, dim] or None: ids only), table_rows, pos (whether
pos_out is asked for)."""
import numpy as np

import table_delta_cases as DC

DEAL_BLOCKS = 8192       # fcp_tables_delta_deal_blocks(): the lone grids of a call are scaled down when they sum past it
FIXED_LAUNCHES = 5       # upload, clear, insert, classify, fold; then one compact launch per class present


def grid_of(n: int, max_blocks: int):
    """(blocks, chunk) of n > 0 positions dealt at most max_blocks: whole tiles, at least MIN_CHUNK_TILES, no idle block"""
    tiles = (n + DC.TILE - 1) // DC.TILE
    chunk = max(DC.MIN_CHUNK_TILES, (tiles + max_blocks - 1) // max_blocks) * DC.TILE
    return (n + chunk - 1) // chunk, chunk


def lone_blocks(n: int) -> int:
    """the classify / compact grid fcp_table_delta_distinct takes for n ids"""
    return grid_of(n, DC.BLOCKS)[0] if n else 0


def deal(ns) -> list:
    """(blocks, chunk) per entry: the lone grid while those sum to DEAL_BLOCKS or less, else the grid of at most
    max(1, floor(lone * DEAL_BLOCKS / sum)) blocks; (0, 0) without ids"""
    lone = [lone_blocks(n) for n in ns]
    total = sum(lone)
    if total <= DEAL_BLOCKS:
        return [grid_of(n, DC.BLOCKS) if n else (0, 0) for n in ns]
    return [grid_of(n, max(1, b * DEAL_BLOCKS // total)) if n else (0, 0) for n, b in zip(ns, lone)]


def compact_class(entry):
    """ids only, or the (V, G) of the entry's rows (with_compact_shape)"""
    if entry["rows"] is None:
        return (0, 1)
    dim = entry["rows"].shape[1]
    vec = 4 if dim % 4 == 0 else 2 if dim % 2 == 0 else 1
    g = 1
    if dim > 4:
        while g < dim // vec and g < 64:
            g <<= 1
    return (vec, g)


def launches_of(entries) -> int:
    with_ids = [e for e in entries if len(e["ids"])]
    if not entries:
        return 0
    return FIXED_LAUNCHES + len({compact_class(e) for e in with_ids}) if with_ids else 1


def _entry(ids, rows, table_rows, pos=False):
    return {"ids": ids, "rows": rows, "table_rows": int(table_rows), "pos": bool(pos)}


def pattern_table_rows(n: int, pattern: str, pick: int) -> int:
    """a table the pattern is drawn in: the one it is FOR where it has one, else option `pick` of table_delta_cases"""
    options = DC.table_rows_options(n, pattern)
    if pattern in ("lds_congruent", "global_congruent", "hot_head"):
        return {"lds_congruent": DC.BIG_ROWS, "global_congruent": DC.global_rows(n), "hot_head": DC.hot_rows(n)}[pattern]
    return options[pick % len(options)]


# ---- 1. a mixed model ------------------------------------------------------------------------------------------------------
def mixed_model() -> list:
    """43 entries: the n of DC.SIZES without its last value, every pattern, every dim of DC.ROW_DIMS (every V, G 1 and the
    groups), a third ids only, int32 and int64 ids mixed, every third entry with pos_out; two entries without ids (one with a
    dim, one ids only) and one whose every id lies outside its table."""
    sizes = DC.SIZES[:-1]
    entries, with_rows = [], 0
    for i in range(40):
        n, pattern = sizes[i % len(sizes)], DC.PATTERNS[i % len(DC.PATTERNS)]
        table_rows = pattern_table_rows(n, pattern, i)
        ids = DC.draw_ids(pattern, n, table_rows, seed=i)
        if i % 5 == 4 and n >= 8:                                   # some ids outside, each next to one inside
            outside = DC.outside_ids(table_rows)
            ids[1:1 + min(len(outside), n - 1)] = outside[:n - 1]
        if i % 2:
            ids = np.where(ids == np.clip(ids, -2 ** 31, 2 ** 31 - 1), ids, -1).astype(np.int32)
        rows = None
        if i % 3 != 2:
            rows = DC.special_rows(n, DC.ROW_DIMS[with_rows % len(DC.ROW_DIMS)], seed=i)
            with_rows += 1
        entries.append(_entry(ids, rows, table_rows, pos=i % 3 == 0))
    entries.insert(7, _entry(np.zeros(0, np.int64), np.zeros((0, 16), np.float32), 50))
    entries.insert(29, _entry(np.zeros(0, np.int32), None, 1, pos=True))
    entries.append(_entry(np.asarray([-1, 9, 2 ** 32 + 3, DC.INT64_MIN, 10, 2 ** 63 - 1, 9, -1], np.int64), DC.special_rows(8, 4, seed=99), 9, pos=True))
    assert {len(e["ids"]) for e in entries} == set(sizes) | {0, 8}
    assert {e["rows"].shape[1] for e in entries if e["rows"] is not None and len(e["ids"])} == set(DC.ROW_DIMS)
    return entries


# ---- 2. isolation ------------------------------------------------------------------------------------------------------------
def isolation(pattern: str) -> list:
    """Two entries with the SAME id array, different tables and different rows, a third entry between them: in the smaller
    table half of the ids lie outside, so the two have different winners at different positions — and the same LDS home slots
    and the same home cells, were their tables one."""
    n = 2 * DC.MIN_CHUNK + 1                                        # three insert tiles, three classify blocks
    big = pattern_table_rows(n, pattern, 0)
    ids = DC.draw_ids(pattern, n, big, seed=7)
    small = int(np.median(ids)) + 1
    assert 0 < (ids >= small).sum() < n
    between = _entry(DC.draw_ids("zipf", 300, 97, seed=8), DC.special_rows(300, 6, seed=8), 97)
    return [_entry(ids, DC.special_rows(n, 6, seed=1), big, pos=True), between, _entry(ids.copy(), DC.special_rows(n, 6, seed=2), small, pos=True)]


# ---- 3. block edges ------------------------------------------------------------------------------------------------------------
def block_edges() -> list:
    """one entry of FULL_PASS + 1 ids (ids only, hot_head: the chunk has grown past its smallest) among 200 entries of 1 id"""
    n = DC.FULL_PASS + 1
    big = _entry(DC.draw_ids("hot_head", n, DC.hot_rows(n), seed=3), None, DC.hot_rows(n))
    small = [_entry(np.asarray([k % 5], np.int64 if k % 2 else np.int32), DC.special_rows(1, 4, seed=k) if k % 4 == 0 else None, 3 + k % 3) for k in range(200)]
    return small[:77] + [big] + small[77:]


# ---- 4. the scaled deal ------------------------------------------------------------------------------------------------------
SCALED_N = 16 * DC.MIN_CHUNK                 # 16 blocks alone
SCALED_NS = [SCALED_N] * 520                 # 8320 blocks alone, past the cap: 15 blocks each at the most


def scaled_deal() -> list:
    """520 equal entries of 16 Ki int32 ids, ids only, whose lone grids sum past DEAL_BLOCKS"""
    assert sum(lone_blocks(n) for n in SCALED_NS) > DEAL_BLOCKS
    assert all(b < lone_blocks(n) for (b, _chunk), n in zip(deal(SCALED_NS), SCALED_NS))
    out = []
    for k, n in enumerate(SCALED_NS):
        pattern = ("zipf", "hot_head", "twice_reversed", "distinct")[k % 4]
        table_rows = pattern_table_rows(n, pattern, k)
        out.append(_entry(DC.draw_ids(pattern, n, table_rows, seed=k).astype(np.int32), None, table_rows, pos=k % 7 == 0))
    return out


# ---- 5. search depth ---------------------------------------------------------------------------------------------------------
def many_small(count: int) -> list:
    """`count` entries of 1 or 2 ids: the first-block tables are as deep as the search goes"""
    rng = np.random.default_rng(count)
    out = []
    for k in range(count):
        n = 1 + k % 2
        ids = rng.integers(-1, 3, n).astype(np.int64 if k % 3 else np.int32)          # repeats and an id outside among them
        out.append(_entry(ids, DC.special_rows(n, (4, 1)[k % 2], seed=k) if k % 5 == 0 else None, 2, pos=k % 11 == 0))
    return out


# ---- 7. the chain ------------------------------------------------------------------------------------------------------------
CHAIN_KINDS = ("f32", "bf16", "f16", "q8")
CHAIN_DIMS = (1, 6, 16, 64)


def chain_model() -> list:
    """(kind, table_rows, dim, ids int64 [n], rows float32 [n, dim]) per table: every format at every dim, ids that repeat, some
    outside the table, one table without a delta"""
    rng = np.random.default_rng(77)
    out = []
    for a, kind in enumerate(CHAIN_KINDS):
        for b, dim in enumerate(CHAIN_DIMS):
            table_rows = 50 + 37 * (4 * a + b)
            n = 0 if (a, b) == (2, 1) else 200 + 61 * b + a
            ids = rng.integers(-3, table_rows + 5, n).astype(np.int64)
            rows = rng.standard_normal((n, dim)).astype(np.float32)
            out.append((kind, table_rows, dim, ids, rows))
    return out
