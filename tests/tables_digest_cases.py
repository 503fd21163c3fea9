"""fcp_tables_digest (recom_amd/csrc/fcp_tables_digest.hip, fcp_tables_digest_plan.cc): the Python restatement of the class rule
and of the deal of blocks, the entry lists, and the runners the host tests (tests/test_tables_digest_host.py) and the GPU tests
(tests/test_zzz_gpu_tables_digest.py, tests/test_zzz_gpu_tables_digest_stream.py) share.  Test data and comparisons only: the CPU
truth is table_digest_cases.digest / digest_ids, and every device value is compared for equality with it and with the
single-table entries (tables.digest / tables.digest_rows)."""
import ctypes as C
import functools

import numpy as np

import table_digest_cases as TD

KINDS = TD.KINDS
LONE_BLOCKS, DEAL_BLOCKS, BLOCK_THREADS, UNROLL = 2048, 8192, 256, 4      # the header's numbers, restated
MAX_LAUNCHES = 2 + 4 * 7 * 2                                                # an upload, one launch per (A, G, by-id), a fold
GUARD = 0x5A5A5A5A5A5A5A5A
INT64_MIN = -(1 << 63)


# ---- the rules, restated ---------------------------------------------------------------------------------------------------
def rows_per_block(kind: str, dim: int) -> int:
    return BLOCK_THREADS // TD.group_of(kind, dim)


def lone_blocks(kind: str, dim: int, count: int) -> int:
    """the grid an entry of `count` rows (ids) takes alone"""
    return min(LONE_BLOCKS, -(-count // rows_per_block(kind, dim))) if count > 0 else 0


def deal(shapes) -> list:
    """blocks per entry of [(kind, dim, count)]: the lone grids while they sum to DEAL_BLOCKS or less, else each scaled"""
    lone = [lone_blocks(kind, dim, count) for kind, dim, count in shapes]
    total = sum(lone)
    if total <= DEAL_BLOCKS:
        return lone
    return [max(1, b * DEAL_BLOCKS // total) if b else 0 for b in lone]


def align_of(address: int, kind: str, dim: int) -> int:
    """A: the largest power of two up to 8 that divides the entry's address and its row bytes"""
    rb = TD.row_bytes(kind, dim)
    return next(a for a in (8, 4, 2, 1) if address % a == 0 and rb % a == 0)


def launches(described) -> int:
    """of [(address, kind, dim, count, by_id)]: 0 for no entries, else upload + one launch per class present + fold"""
    described = list(described)
    if not described:
        return 0
    return 2 + len({(align_of(addr, kind, dim), TD.group_of(kind, dim), bool(by_id)) for addr, kind, dim, count, by_id in described if count > 0})


# ---- entries on the CPU ----------------------------------------------------------------------------------------------------
class Spec:
    """One entry before it has a device: `raw` uint8 [rows, row_bytes] are the rows back to back (ids None), or the WHOLE table
    the int64 `ids` name rows of.  `front`: bytes in front of the table inside its allocation; `slack`: rows of other bytes behind
    it inside its allocation (where an id of table_rows and just beyond would land)."""

    def __init__(self, kind, dim, raw, ids=None, row0=0, step=1, front=0, slack=0):
        self.kind, self.dim, self.ids, self.row0, self.step, self.front = kind, dim, ids, row0, step, front
        self.allocated, self.raw = raw, raw[:raw.shape[0] - slack]
        self._want = None

    @property
    def count(self) -> int:
        return int(self.raw.shape[0] if self.ids is None else self.ids.size)

    @property
    def want(self):
        """(sum, rows, skipped) from the NumPy reference, computed once"""
        if self._want is None:
            if self.ids is None:
                self._want = (TD.digest(self.raw.tobytes(), self.kind, self.dim, self.row0, self.step), int(self.raw.shape[0]), 0)
            else:
                self._want = TD.digest_ids(self.raw.tobytes(), self.kind, self.dim, self.ids, self.row0, self.step)
        return self._want


def direct(kind, dim, rows, seed, row0=0, step=1, front=0) -> Spec:
    return Spec(kind, dim, TD.draw_raw(kind, dim, rows, seed), None, row0, step, front)


def by_id(kind, dim, n, seed, row0=0, step=1, outside=(), repeat=(), table_rows=None, slack=0) -> Spec:
    """n ids of a table of n + 3 rows (row 0 and the last row among them from n == 2 on), the ids at the positions `outside`
    replaced by -1, INT64_MIN, table_rows and 2^40 in turn, those at the positions `repeat` by the id in front of them."""
    table_rows = n + 3 if table_rows is None else table_rows
    rng = np.random.default_rng([seed, n])
    ids = rng.permutation(table_rows)[:n].astype(np.int64)
    if n >= 2:
        ids[0], ids[-1] = 0, table_rows - 1
        ids[1:-1] = rng.permutation(np.arange(1, table_rows - 1))[:n - 2]
    for pos in repeat:
        ids[pos] = ids[pos - 1]
    bad = (-1, INT64_MIN, table_rows, 1 << 40)
    for j, pos in enumerate(outside):
        ids[pos] = bad[j % 4]
    return Spec(kind, dim, TD.draw_raw(kind, dim, table_rows + slack, seed), ids, row0, step, slack=slack)


@functools.lru_cache(maxsize=None)
def mixed_model():
    """40 entries: the four kinds in turn, the ten dims of TD.DIMS in turn, every third entry by id; row counts 1, one block's
    rows - 1 / + 0 / + 1, and — six entries whose lone grids alone sum past the deal's 8192 — one full unrolled pass of the
    entry's OWN (scaled) grid plus one row; empty entries first, last and twice in a row in the middle, in both modes."""
    shapes = []
    for i in range(40):
        kind, dim = KINDS[i % 4], TD.DIMS[(i + i // 20) % 10]          # (the shift: both halves pair a dim with other kinds)
        per = rows_per_block(kind, dim)
        count = 0 if i in (0, 19, 20, 39) else (1, per - 1, per, per + 1, LONE_BLOCKS * per + 1)[i % 5]
        shapes.append([kind, dim, count])
    full = [i for i, (_k, _d, count) in enumerate(shapes) if count > LONE_BLOCKS]
    blocks = deal(shapes)
    assert len(full) == 6 and all(blocks[i] < LONE_BLOCKS for i in full)
    for i in full:                                                     # (beyond the cap a lone grid stays 2048: the deal stands)
        shapes[i][2] = UNROLL * blocks[i] * rows_per_block(*shapes[i][:2]) + 1
    assert deal(shapes) == blocks and all(shapes[i][2] > LONE_BLOCKS * rows_per_block(*shapes[i][:2]) for i in full)
    out = []
    for i, (kind, dim, count) in enumerate(shapes):
        row0, step = i, 1 + i % 3
        if i % 3 == 0:
            out.append(by_id(kind, dim, count, 500 + i, row0, step, outside=(1, 2) if count >= 4 else ()))
        else:
            out.append(direct(kind, dim, count, 500 + i, row0, step))
    assert {s.kind for s in out if s.count} == set(KINDS) and {s.dim for s in out if s.count} == set(TD.DIMS)
    assert {s.ids is None for s in out if s.count} == {True, False} and {s.ids is None for s in out if not s.count} == {True, False}
    return tuple(out)


@functools.lru_cache(maxsize=None)
def scaled_deal():
    """24 bf16 entries of dim 1 with 2048 * 256 rows each (24 MB in all): alone each fills the fixed grid in ONE stride; grouped
    each gets 341 blocks and walks several trips with its own stride."""
    return tuple(direct("bf16", 1, LONE_BLOCKS * 256, 700 + i, row0=i) for i in range(24))


@functools.lru_cache(maxsize=None)
def search_depth(n_entries: int = 1500):
    """1500 entries of 1 to 3 rows, q8 of dim 8 (16-byte rows, G 2) and bf16 of dim 16 (32-byte rows, G 4) in turn: two launches
    of 750 one-block entries each — ten search steps, and every first-block value is the end of the entry in front."""
    return tuple(direct(*(("q8", 8), ("bf16", 16))[i % 2], 1 + i % 3, 1000 + i, row0=i) for i in range(n_entries))


@functools.lru_cache(maxsize=None)
def skew():
    """One entry of 300 000 rows among one-row entries of its class, in both modes."""
    out = []
    for make in (direct, by_id):
        out += [make("f16", 16, 1, 2000), make("f16", 16, 1, 2001), make("f16", 16, 300000, 2002, row0=7, step=2), make("f16", 16, 1, 2003)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def outside_ids():
    """Ids outside the table — -1, INT64_MIN, table_rows, 2^40, with table_rows inside the allocation — in some entries and none in
    others; repeated ids, which count as often as they occur; an entry of nothing but outside ids."""
    out = []
    for kind, dim in (("q8", 64), ("q8", 3), ("bf16", 6), ("f32", 64)):
        out.append(by_id(kind, dim, 257, 3000 + dim, outside=(5, 6, 64, 256), repeat=(10, 11, 200), slack=4))
        out.append(by_id(kind, dim, 65, 3100 + dim))
        out.append(by_id(kind, dim, 70, 3200 + dim, outside=(0,), repeat=(69,), slack=1))
        out.append(by_id(kind, dim, 9, 3300 + dim, outside=tuple(range(9)), slack=2))
    return tuple(out)


# ---- on the device -----------------------------------------------------------------------------------------------------------
class Item:
    """One entry as the call takes it: a device table (or row range), its kind and dim, device ids or None."""

    def __init__(self, table, kind, dim, ids=None, n=0, row0=0, step=1):
        self.table, self.kind, self.dim, self.ids, self.n, self.row0, self.step = table, kind, dim, ids, n, row0, step

    def entry(self, lib):
        return lib.TableDigestEntry(self.table.data_ptr() if self.table.numel() else None, self.ids.data_ptr() if self.ids is not None else None,
                                    int(self.table.shape[0]), self.n, self.row0, self.step, TD.KIND[self.kind], self.dim, 0)


def place(torch, spec: Spec, dev) -> Item:
    table = TD.as_table(torch, spec.allocated, spec.kind, spec.dim, dev, front=spec.front)[:spec.raw.shape[0]]
    if spec.ids is None:
        return Item(table, spec.kind, spec.dim, None, 0, spec.row0, spec.step)
    ids = torch.zeros((spec.ids.size + 1,), dtype=torch.int64, device=dev)      # (never empty: an entry of no ids keeps its mode)
    ids[:spec.ids.size].copy_(torch.from_numpy(spec.ids))
    return Item(table, spec.kind, spec.dim, ids, int(spec.ids.size), spec.row0, spec.step)


def call(torch, items, dev, stream=None, what=""):
    """fcp_tables_digest of `items` through the C ABI, TWICE, into buffers of the test's own: the guard words in front of and
    behind out[n_tables] and the workspace survive, both calls leave the same bytes, `reserved` is 0, and the launch count stays
    within its bound and is the restated rule's.  Returns ([(sum, rows, skipped)] per entry, the blocks dealt per entry)."""
    from recom_amd import lib
    L = lib.load()
    n = len(items)
    entries = (lib.TableDigestEntry * max(n, 1))(*[it.entry(lib) for it in items])
    blocks = (C.c_int32 * max(n, 1))()
    enq = int(L.fcp_tables_digest_launches(entries, n, blocks))
    assert 0 <= enq <= MAX_LAUNCHES, (what, enq, L.fcp_last_error().decode())
    assert enq == launches((it.table.data_ptr(), it.kind, it.dim, it.n if it.ids is not None else int(it.table.shape[0]), it.ids is not None)
                           for it in items), (what, enq)
    ws_words = int(L.fcp_tables_digest_workspace_bytes(n)) // 8
    results = []
    for _ in range(2):
        buf = torch.full((4 + 4 * n + 4 + ws_words + 4,), GUARD, dtype=torch.int64, device=dev)
        out, ws = buf[4:4 + 4 * n], buf[8 + 4 * n:8 + 4 * n + ws_words]
        torch.cuda.synchronize()
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
        status = L.fcp_tables_digest(entries, n, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), dev.index or 0, C.c_void_p(s))
        assert status == lib.FCP_OK, (what, L.fcp_last_error().decode())
        (torch.cuda if stream is None else stream).synchronize()
        host = buf.cpu().numpy()
        assert (host[:4] == GUARD).all() and (host[4 + 4 * n:8 + 4 * n] == GUARD).all() and (host[8 + 4 * n + ws_words:] == GUARD).all(), \
            (what, "a guard word was written")
        results.append(host[4:4 + 4 * n].copy())
    assert np.array_equal(results[0], results[1]), (what, "two calls left different bytes")
    rec = results[0].reshape(n, 4)
    assert (rec[:, 3] == 0).all(), (what, "reserved")
    return [(int(r[0]) & TD.M64, int(r[1]), int(r[2])) for r in rec], list(blocks[:n])


def run(torch, specs, dev, stream=None, what=""):
    """`specs` on the device through ONE grouped call (see `call`): every record equals the NumPy reference and what the
    single-table entry leaves for the same entry (on the same stream when one is given), entries without rows leave zeros, and
    the tables are unchanged.  Returns the blocks the call dealt."""
    from recom_amd import tables
    items = [place(torch, s, dev) for s in specs]
    got, blocks = call(torch, items, dev, stream=stream, what=what)
    assert blocks == deal([(s.kind, s.dim, s.count) for s in specs]), (what, "the deal")
    s_ = None if stream is None else stream.cuda_stream
    for k, (spec, it, g) in enumerate(zip(specs, items, got)):
        where = (what, "entry", k, spec.kind, spec.dim, spec.count, "by id" if spec.ids is not None else "rows")
        print(*where, hex(g[0]), g[1:], hex(spec.want[0]), spec.want[1:])
        assert g == spec.want, where
        if spec.count == 0:
            assert g == (0, 0, 0), where
        if spec.ids is None:
            single = (tables.digest(it.table, row0=spec.row0, row_step=spec.step, stream=s_), int(it.table.shape[0]), 0)
        else:
            single = tables.digest_rows(it.table, it.ids[:it.n], row0=spec.row0, row_step=spec.step, stream=s_)
        assert g == single, where + ("the single-table entry differs",)
        assert np.array_equal(TD.bytes_of(torch, it.table), spec.raw.reshape(-1)), where + ("the table's own bytes changed",)
    return blocks
