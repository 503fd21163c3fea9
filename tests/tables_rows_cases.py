"""fcp_tables_update_rows / fcp_tables_read_rows (recom_amd/csrc/fcp_tables_rows.hip): the entry lists and the two runners the
GPU tests share (tests/test_zzz_gpu_tables_rows.py, tests/test_zzz_gpu_tables_rows_stream.py).  Test data and comparisons only: an
entry is (kind, dim, table_rows, ids, x) — ids int64 [n], possibly outside the table, x float32 [n, dim] — and every expectation
comes from table_rows_cases.expect_bytes (the restatements) and from the single-table entries."""
import numpy as np

import table_convert_cases as TC
import table_rows_cases as R

KINDS = ("f32", "bf16", "f16", "q8")
SKIPPED_BEFORE = 7            # what every counter holds before a call: "has grown by", not "is"
OUTSIDE = (-1, R.INT64_MIN, None, 1 << 40)        # None: table_rows itself, the first row behind the table


def rows_of(dim: int, n: int, seed: int = 0) -> np.ndarray:
    """float32 [n, dim]: a prefix of TC.quant_rows (edges and families) while it lasts, TC.family_rows beyond."""
    if n <= max(TC.QUANT_ROWS):
        return np.array(TC.quant_rows(dim)[:n])
    return TC.family_rows(dim, n, 40 + seed)


def entry(kind: str, dim: int, n: int, seed: int, outside=(), table_rows=None):
    """n distinct ids of a table of n + R.SLACK_ROWS rows (row 0 and the last row among them from n == 2 on), with the ids at the
    positions `outside` replaced by the values of OUTSIDE in turn."""
    table_rows = n + R.SLACK_ROWS if table_rows is None else table_rows
    ids = R.distinct_ids(n, table_rows, seed) if n else np.zeros((0,), np.int64)
    for j, pos in enumerate(outside):
        bad = OUTSIDE[j % len(OUTSIDE)]
        ids[pos] = table_rows if bad is None else bad
    return kind, dim, table_rows, ids, rows_of(dim, n, seed)


def inside(e) -> np.ndarray:
    _kind, _dim, table_rows, ids, _x = e
    return (ids >= 0) & (ids < table_rows)


def mixed_model():
    """40 entries: the four kinds in turn, dims of every V (and of G 1 to 64, the register cap crossed), n on both sides of a wave
    and of a block; empty entries first, last, and two in a row in the middle."""
    dims = (1, 2, 3, 4, 5, 12, 64, 260, TC.REGISTER_CAP[4] + 4)
    ns = (0, 1, 63, 64, 65, 257)
    out = []
    for i in range(40):
        n = 0 if i in (0, 19, 20, 39) else ns[(5 * i + i // 6) % 6]
        out.append(entry(KINDS[i % 4], dims[i % 9], n, 100 + i))
    assert sum(1 for e in out if len(e[3]) == 0) >= 4 and {e[0] for e in out if len(e[3])} == set(KINDS)
    assert {len(e[3]) for e in out} == set(ns) and {e[1] for e in out if len(e[3])} == set(dims)
    return out


def block_edges():
    """Entries whose threads are exactly one block of 256, and one block -/+ one row, next to each other in their class: the q8
    front (n * G) at G 1, 8, 16, 64 and the streaming front (n * dim / V) at 1, 8 and 16 slots per row, V 4, 2, 1."""
    out = []
    for dim, per_block in ((3, 256), (5, 32), (64, 16), (260, 4)):
        assert 256 // TC.group_of(dim) == per_block
        out += [entry("q8", dim, n, 300 + dim + n) for n in (per_block, per_block - 1, per_block + 1, 2 * per_block)]
    for kind, dim, per_block in (("bf16", 4, 256), ("f16", 2, 256), ("f32", 1, 256), ("bf16", 64, 16), ("f32", 32, 32)):
        assert 256 // (dim // TC.vec_of(dim)) == per_block
        out += [entry(kind, dim, n, 400 + dim + n) for n in (per_block, per_block - 1, per_block + 1, 2 * per_block)]
    return out


def search_depth(n_entries: int = 1500):
    """1500 entries of 1 to 3 rows, q8 and bf16 in turn, dim 8: two launches of 750 one-block pieces each — ten search steps, and
    every first-block value is the end of the piece in front."""
    return [entry(("q8", "bf16")[i % 2], 8, 1 + i % 3, 1000 + i) for i in range(n_entries)]


def skew():
    """One entry of 5000 rows beside entries of one row, in both fronts: the grid is the sum of the entries' blocks."""
    out = []
    for kind in ("q8", "f16"):
        out += [entry(kind, 16, 1, 2000), entry(kind, 16, 1, 2001), entry(kind, 16, 5000, 2002), entry(kind, 16, 1, 2003)]
    return out


def outside_ids():
    """Ids outside the table — -1, INT64_MIN, table_rows, 2^40 — in some entries and none in others, per front; an entry of
    nothing but outside ids; a counter per entry."""
    out = []
    for kind, dim in (("q8", 64), ("q8", 3), ("bf16", 6), ("f32", 64)):
        out.append(entry(kind, dim, 257, 3000 + dim, outside=(5, 6, 64, 256)))
        out.append(entry(kind, dim, 65, 3100 + dim))
        out.append(entry(kind, dim, 70, 3200 + dim, outside=(0,)))
        out.append(entry(kind, dim, 9, 3300 + dim, outside=tuple(range(9))))
    return out


def run_update(torch, entries, dev, stream=None, with_skipped=True, what=""):
    """One grouped update of `entries` into poisoned tables, and per-table tables.update_rows into poisoned twins (the same stream
    when one is given).  Every buffer — the rows behind each table included — equals the CPU expectation and its twin byte for
    byte; skipped[k] has grown by entry k's outside ids, exactly, and is untouched where there are none.  Returns the tables."""
    from recom_amd import tables
    bufs, tabs, twin_bufs, twins, d_ids, d_x = [], [], [], [], [], []
    for kind, dim, table_rows, ids, x in entries:
        b, t = R.poisoned(torch, kind, dim, table_rows, dev)
        tb, tt = R.poisoned(torch, kind, dim, table_rows, dev)
        bufs.append(b), tabs.append(t), twin_bufs.append(tb), twins.append(tt)
        d_ids.append(torch.from_numpy(ids).to(dev)), d_x.append(torch.from_numpy(np.ascontiguousarray(x)).to(dev))
    skipped = torch.full((len(entries),), SKIPPED_BEFORE, dtype=torch.int64, device=dev) if with_skipped else None
    twin_skipped = torch.full((len(entries),), SKIPPED_BEFORE, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    assert tables.update_rows_grouped(tabs, d_ids, d_x, skipped=skipped, stream=s) is tabs
    for k, (t, i, r) in enumerate(zip(twins, d_ids, d_x)):
        tables.update_rows(t, i, r, skipped=twin_skipped[k:k + 1], stream=s)
    (torch.cuda if stream is None else stream).synchronize()
    for k, e in enumerate(entries):
        kind, dim, table_rows, ids, x = e
        keep = inside(e)
        want_rows = R.expect_bytes(x, kind)[keep] if len(ids) else np.zeros((0, R.row_bytes(kind, dim)), np.uint8)
        R.check_poisoned(bufs[k], kind, dim, table_rows, ids[keep], want_rows, (what, "entry", k, kind, dim, len(ids)))
    assert torch.equal(torch.cat(bufs), torch.cat(twin_bufs)), (what, "the grouped call and the per-table calls differ")
    want = np.asarray([SKIPPED_BEFORE + int((~inside(e)).sum()) for e in entries], np.int64)
    assert (twin_skipped.cpu().numpy() == want).all(), what
    if with_skipped:
        assert (skipped.cpu().numpy() == want).all(), (what, skipped.cpu().numpy(), want)
    return tabs


def run_read(torch, entries, dev, stream=None, what=""):
    """Tables holding the rows x of each entry at its inside ids (poison elsewhere: any bytes are rows), read back by ONE grouped
    call into sentinel-backed outputs, and by per-table tables.read_rows: the same bits, +0.0 for outside ids, the element behind
    every output intact."""
    from recom_amd import tables
    tabs, d_ids, fronts, backs = [], [], [], []
    for kind, dim, table_rows, ids, x in entries:
        _b, t = R.poisoned(torch, kind, dim, table_rows, dev)
        i = torch.from_numpy(ids).to(dev)
        tables.update_rows(t, i, torch.from_numpy(np.ascontiguousarray(x)).to(dev))
        n = len(ids)
        back = torch.empty((n * dim + 1,), dtype=torch.int32, device=dev).fill_(0x5A5A5A5A).view(torch.float32)
        tabs.append(t), d_ids.append(i), backs.append(back), fronts.append(back[:n * dim].view(n, dim))
    torch.cuda.synchronize()
    s = None if stream is None else stream.cuda_stream
    got = tables.read_rows_grouped(tabs, d_ids, out=fronts, stream=s)
    assert all(g is f for g, f in zip(got, fronts))
    single = [tables.read_rows(t, i, stream=s) for t, i in zip(tabs, d_ids)]
    fresh = tables.read_rows_grouped(tabs, d_ids, stream=s)           # the allocating form
    (torch.cuda if stream is None else stream).synchronize()
    for k, e in enumerate(entries):
        kind, dim, _table_rows, ids, _x = e
        g = backs[k].cpu().numpy().view(np.uint32)
        assert g[-1] == 0x5A5A5A5A, (what, k, "the element behind the output was written")
        g = g[:-1].reshape(len(ids), dim)
        assert (g == single[k].cpu().numpy().view(np.uint32)).all(), (what, "entry", k, kind, dim)
        assert (g == fresh[k].cpu().numpy().view(np.uint32)).all() and tuple(fresh[k].shape) == (len(ids), dim)
        assert (g[~inside(e)] == 0).all(), (what, k, "a row of an outside id is not +0.0")
        if kind == "f32" and len(ids):
            assert (g[inside(e)] == np.ascontiguousarray(e[4]).view(np.uint32)[inside(e)]).all()
