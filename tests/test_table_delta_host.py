"""fcp_table_delta_distinct / fcp_table_delta_workspace_bytes without a GPU: the two names in the header, in lib.EXPORTS and in
the loaded library; the report's size; the workspace formula's properties; every FCP_ERR_INVALID_ARGUMENT in the documented
order (no device is needed for any of them); what the Python wrappers refuse; and the restatement of table_delta_cases held to a
plain dict loop, with every id pattern shown to contain what it is for.  (The kernels: tests/test_gpu_table_delta.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import table_delta_cases as D
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
INV, NODEV = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE
A = 1 << 20          # (pointers are never dereferenced on the host: plain numbers serve)


def test_header_declares_and_library_exports_the_two_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint64_t fcp_table_delta_workspace_bytes\(int64_t n\);", text)
    assert re.search(r"\bint fcp_table_delta_distinct\(const void \*row_ids, int32_t id_bytes, const float \*rows, int32_t dim, int64_t n,\s+"
                     r"int64_t table_rows,\s+int64_t \*ids_out, float \*rows_out, int64_t \*pos_out, fcp_table_delta_report_t \*report,\s+"
                     r"void \*workspace,\s+int32_t device, void \*stream\);", text)
    names = {"fcp_table_delta_workspace_bytes", "fcp_table_delta_distinct"}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names)
    # the header's surface and the mirror agree (tests/test_host.py holds the same for every entry)
    assert set(re.findall(r"\b(fcp_[a-z_0-9]+)\s*\(", text)) - {"fcp_alloc_fn"} == set(_lib.EXPORTS)
    assert C.sizeof(_lib.TableDeltaReport) == 32
    assert [f[0] for f in _lib.TableDeltaReport._fields_] == ["n", "distinct", "duplicates", "skipped"]
    assert re.search(r"\} fcp_table_delta_report_t; /\* 32 bytes \*/", text)


def test_workspace_bytes():
    """depends on n only; a multiple of 8; non-decreasing; at most 40 n + 2^20; -1 outside [0, 2^32 - 3); the mirrored formula"""
    L = _lib.load()
    ns = sorted(set([0, 1, 2, 31, 32, 33, 1000, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, D.LIMIT - 1]
                    + [2 ** k + d for k in range(3, 32) for d in (-1, 0, 1)] + list(D.SIZES)))
    last = 0
    for n in ns:
        b = int(L.fcp_table_delta_workspace_bytes(n))
        assert b == D.workspace_bytes(n), n
        assert b > 0 and b % 8 == 0 and b >= last and b <= 40 * n + 2 ** 20, (n, b)
        assert D.cells_for(n) >= 2 * n and D.cells_for(n) & (D.cells_for(n) - 1) == 0
        last = b
    for n in (-1, -2 ** 40, D.LIMIT, D.LIMIT + 1, 2 ** 32, 2 ** 62, D.INT64_MIN):
        assert int(L.fcp_table_delta_workspace_bytes(n)) == -1, n


def _distinct(row_ids, id_bytes, rows, dim, n, table_rows, ids_out, rows_out, pos_out, report, workspace, device=0):
    L = _lib.load()
    p = C.c_void_p
    status = L.fcp_table_delta_distinct(p(row_ids), id_bytes, p(rows), dim, n, table_rows, p(ids_out), p(rows_out), p(pos_out), p(report),
                                        p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def test_status_codes_arrive_in_the_stated_order():
    import torch
    #         row_ids id_bytes rows dim n table_rows ids_out rows_out pos_out report workspace
    good = (A, 8, A, 64, 3, 5, A, A, A, A, A)

    def but(**kw):
        names = ("row_ids", "id_bytes", "rows", "dim", "n", "table_rows", "ids_out", "rows_out", "pos_out", "report", "workspace")
        assert set(kw) <= set(names)
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    for args, word in ((but(n=-1), "`n`"), (but(n=D.LIMIT), "`n`"), (but(n=2 ** 40), "`n`"),
                       (but(table_rows=0), "`table_rows`"), (but(table_rows=-7), "`table_rows`"), (but(table_rows=D.LIMIT), "`table_rows`"),
                       (but(id_bytes=0), "`id_bytes`"), (but(id_bytes=2), "`id_bytes`"), (but(id_bytes=16), "`id_bytes`"), (but(id_bytes=-8), "`id_bytes`"),
                       (but(dim=0), "`dim`"), (but(dim=-3), "`dim`"), (but(dim=0, rows_out=0), "`dim`"),
                       (but(rows=0), "`rows_out` without `rows`"), (but(rows=0, dim=0), "`rows_out` without `rows`"),
                       (but(rows_out=0), "`rows_out` is null"),
                       (but(report=0), "`report`"), (but(report=0, n=0), "`report`"), (but(workspace=0), "`workspace`"), (but(workspace=0, n=0), "`workspace`"),
                       (but(row_ids=0), "`row_ids`"), (but(ids_out=0), "`ids_out`"), (but(row_ids=0, n=1, rows=0, rows_out=0), "`row_ids`"),
                       (but(row_ids=A + 4), "`row_ids`"), (but(row_ids=A + 2, id_bytes=4), "`row_ids`"), (but(row_ids=A + 12, n=0), "`row_ids`"),
                       (but(rows=A + 4), "`rows`"), (but(rows=A + 8), "`rows`"), (but(rows=A + 4, dim=62), "`rows`"), (but(rows=A + 2, dim=61), "`rows`"),
                       (but(ids_out=A + 4), "`ids_out`"), (but(ids_out=A + 4, n=0), "`ids_out`"),
                       (but(rows_out=A + 8), "`rows_out`"), (but(rows_out=A + 4, dim=6), "`rows_out`"), (but(rows_out=A + 1, dim=3), "`rows_out`"),
                       (but(pos_out=A + 4), "`pos_out`"), (but(report=A + 4), "`report`"), (but(workspace=A + 4), "`workspace`")):
        status, msg = _distinct(*args)
        assert status == INV and word in msg and msg.startswith("fcp_table_delta_distinct: "), (args, status, msg)
    # the order: n, table_rows, id_bytes, dim with rows, the rows pair, null report / workspace, null ids with n > 0, then
    # misalignment in argument order — each call is wrong in everything that follows, too
    bad = dict(n=-1, table_rows=0, id_bytes=3, dim=0, rows_out=0, report=0, workspace=0, row_ids=0, ids_out=0, pos_out=A + 4)
    order = [("n", 3, "`n`"), ("table_rows", 5, "`table_rows`"), ("id_bytes", 8, "`id_bytes`"), ("dim", 64, "`dim`"),
             ("rows_out", A + 8, "`rows_out` is null"), ("report", A + 4, "`report` is null"), ("workspace", A + 4, "`workspace` is null"),
             ("row_ids", A + 4, "`row_ids` is null"), ("ids_out", A + 4, "`ids_out` is null")]
    for name, fixed, word in order:
        assert word in _distinct(*but(**bad))[1], (name, _distinct(*but(**bad))[1])
        bad[name] = fixed
    bad["rows"] = A + 8
    for name, word in (("row_ids", "`row_ids` is not 8"), ("rows", "`rows` is not 16"), ("ids_out", "`ids_out` is not 8"),
                       ("rows_out", "`rows_out` is not 16"), ("pos_out", "`pos_out` is not 8"), ("report", "`report` is not 8"),
                       ("workspace", "`workspace` is not 8")):
        assert word in _distinct(*but(**bad))[1], (name, _distinct(*but(**bad))[1])
        bad[name] = A
    if not torch.cuda.is_available():
        assert _distinct(*but(**bad))[0] == NODEV
        # alignments that ARE enough, ids only, pos_out NULL, n == 0 (the report is written on the device), the ends of the ranges
        for args in (good, but(rows=A + 4, rows_out=A + 12, dim=61), but(rows=A + 8, rows_out=A + 8, dim=62), but(row_ids=A + 4, id_bytes=4),
                     but(rows=0, rows_out=0, dim=0), but(rows=0, rows_out=0, dim=-5), but(pos_out=0), but(n=0), but(n=0, row_ids=0, ids_out=0),
                     but(n=D.LIMIT - 1, table_rows=D.LIMIT - 1), but(n=1, table_rows=1)):
            assert _distinct(*args)[0] == NODEV, args


def test_python_wrappers_refuse_what_they_can_see():
    import torch
    from recom_amd import tables
    ids = torch.zeros((3,), dtype=torch.int64)
    for fn in (tables.delta_distinct, tables.delta_distinct_async):
        for bad in (torch.zeros((3,), dtype=torch.float32), torch.zeros((3,), dtype=torch.int16), torch.zeros((3, 1), dtype=torch.int64),
                    torch.zeros((6,), dtype=torch.int32)[::2]):
            with pytest.raises(ValueError, match=r"row_ids is a contiguous int64 or int32 \[n\] tensor"):
                fn(bad, table_rows=5)
        with pytest.raises(ValueError, match="device to device; the tensor is on cpu"):
            fn(ids, table_rows=5)
    table = torch.zeros((5, 4))
    with pytest.raises(ValueError, match="device to device"):          # the table's own refusal comes first
        tables.apply_delta(table, ids, torch.zeros((3, 4)))
    with pytest.raises(ValueError, match="no table format"):
        tables.apply_delta(torch.zeros((5, 4), dtype=torch.int32), ids, torch.zeros((3, 4)))
    r = tables.DeltaReport(4, 2, 1, 1)
    assert (r.n, r.distinct, r.duplicates, r.skipped) == (4, 2, 1, 1)
    with pytest.raises(Exception):
        r.n = 5                                                         # frozen


def _dict_loop(ids, table_rows):
    """the plain restatement: remember each row's last position"""
    last = {}
    skipped = 0
    for i, r in enumerate(int(v) for v in ids):
        if 0 <= r < table_rows:
            last[r] = i
        else:
            skipped += 1
    pos = sorted(last.values())
    n = len(ids)
    return pos, {"n": n, "distinct": len(pos), "duplicates": n - skipped - len(pos), "skipped": skipped}


def _check_ref(ids, table_rows):
    pos, report, ids_out, pos_out = D.distinct_ref(ids, table_rows)
    want_pos, want_report = _dict_loop(ids, table_rows)
    assert pos.tolist() == want_pos and report == want_report
    m, n = len(want_pos), len(ids)
    wide = np.asarray(ids).astype(np.int64)
    assert pos.dtype == ids_out.dtype == pos_out.dtype == np.int64 and ids_out.shape == pos_out.shape == (n,)
    assert ids_out[:m].tolist() == wide[want_pos].tolist() and pos_out[:m].tolist() == want_pos
    assert (ids_out[m:] == -1).all() and (pos_out[m:] == -1).all()
    assert report["n"] == report["distinct"] + report["duplicates"] + report["skipped"]
    return report


def test_the_restatement_against_a_dict_loop():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 7, 100, 3000):
        for table_rows in (1, 2, 17, 5000):
            _check_ref(rng.integers(-3, table_rows + 3, n, dtype=np.int64), table_rows)
            _check_ref(rng.integers(-3, min(table_rows + 3, 2 ** 31), n).astype(np.int32), table_rows)
    for table_rows in (1, 2, 1000, D.LIMIT - 1):
        o = D.outside_ids(table_rows)
        r = _check_ref(o, table_rows)
        assert r["skipped"] == 9 and r["distinct"] == (1 if table_rows == 1 else 2), (table_rows, r)
        r = _check_ref(D.outside_ids32(table_rows), table_rows)
        assert r["skipped"] == 4 and r["distinct"] == (1 if table_rows == 1 else 2)
    # an outside id never shadows the inside id whose low 32 bits it shares: the LAST inside occurrence wins, whatever follows
    pos, _r, ids_out, _p = D.distinct_ref(np.asarray([3, 2 ** 32 + 3, -1], np.int64), 5)
    assert pos.tolist() == [0] and ids_out.tolist() == [3, -1, -1]
    # apply_ref: position order, the last write stays
    t = np.zeros((4, 2), np.float32)
    got = D.apply_ref(t, [1, 3, 1, 9, -1], np.arange(10, dtype=np.float32).reshape(5, 2))
    assert got.tolist() == [[0, 0], [4, 5], [0, 0], [2, 3]] and not t.any()


def test_every_pattern_contains_what_it_is_for():
    """duplicates where a pattern is meant to repeat and none where it is not; the winner of `equal` is the last position;
    the congruent patterns hold chains longer than the probe limit, from the mirrored constants; the sizes straddle the
    kernels' edges."""
    assert D.chunk_for(1) == D.chunk_for(D.FULL_PASS) == D.MIN_CHUNK and D.chunk_for(D.FULL_PASS + 1) == D.MIN_CHUNK + D.TILE
    assert {1, 2, 63, 64, 65, D.TILE - 1, D.TILE + 1, D.MIN_CHUNK - 1, D.MIN_CHUNK + 1, D.FULL_PASS + 1} <= set(D.SIZES)
    assert max(D.SIZES) == D.FULL_PASS + 1 and D.BIG_ROWS > D.LDS_SLOTS and D.BIG_ROWS > D.CONGRUENT_ROWS * D.LDS_SLOTS - D.LDS_SLOTS
    for n in D.SIZES:
        for pattern in D.PATTERNS:
            options = D.table_rows_options(n, pattern)
            # no case is left out: every pattern in at least two tables at every n — the four sizes the issue names, or, for
            # ids that are all distinct, every one of them that can hold n ids, the table of exactly n rows and a larger one
            assert len(options) >= 2 and len(set(options)) == len(options), (n, pattern, options)
            if pattern == "distinct":
                assert n in options and min(options) >= n and max(options) >= 2 * n
                assert {r for r in (1, 2, max(n // 2, 1), D.BIG_ROWS) if r >= n} <= set(options)
            else:
                assert {1, 2, max(n // 2, 1), D.BIG_ROWS} <= set(options)
            for table_rows in options:
                ids = D.draw_ids(pattern, n, table_rows)
                assert ids.dtype == np.int64 and ids.shape == (n,) and ids.min() >= 0 and ids.max() < table_rows, (pattern, n, table_rows)
                pos, report, _i, _p = D.distinct_ref(ids, table_rows)
                assert report["skipped"] == 0
                if pattern == "distinct":
                    assert report["duplicates"] == 0 and pos.tolist() == list(range(n))
                elif pattern == "equal":
                    assert pos.tolist() == [n - 1] and report["duplicates"] == n - 1
                elif pattern == "twice_reversed" and table_rows >= n:
                    assert report["duplicates"] == n // 2 and pos.tolist() == list(range(n // 2, n))
                if pattern in D.REPEATING and n >= D.TILE:
                    assert report["duplicates"] > 0, (pattern, n, table_rows)
        if n >= D.TILE:
            # chains longer than the probe limit: more rows on ONE home slot than the LDS table probes, and as many on one
            # home cell of the global table
            rows = np.unique(D.draw_ids("lds_congruent", n, D.BIG_ROWS))
            assert len(rows) == D.CONGRUENT_ROWS > D.PROBES and not (rows % D.LDS_SLOTS).any()
            rows = np.unique(D.draw_ids("global_congruent", n, D.global_rows(n)))
            assert len(rows) > D.PROBES and len(set(D.home_of(rows, D.cells_for(n)).tolist())) == 1, (n, rows)
            hot = D.draw_ids("hot_head", n, D.hot_rows(n))
            assert (hot == 0).sum() >= n // 4 and len(np.unique(hot)) > n // 2
    for dim in D.ROW_DIMS:
        x = D.special_rows(50, dim).view(np.uint32)
        assert len({bytes(r) for r in x}) == (50 if dim >= 2 else 48)      # (dim 1: seven fixed words, five different)
    x = D.special_rows(50, 64)
    assert np.isnan(x).any() and (x.view(np.uint32) == 0x80000000).any() and (x.view(np.uint32) == 1).any()
    assert set(D.ROW_DIMS) == {1, 2, 3, 4, 6, 62, 64, 300}
