"""fcp_table_diff / fcp_table_diff_workspace_bytes without a GPU: the two names in the header, in lib.EXPORTS and in the loaded
library; the report's size; the workspace formula's properties; every FCP_ERR_INVALID_ARGUMENT in the documented order (no
device is needed for any of them); what the Python wrappers refuse; the restatement of table_diff_cases held to a plain per-row
loop; and every change pattern shown to contain what it is for — the QUIET pattern above all: at least a quarter of its rows
differ in their float32 bits and in no byte of the format, at least a quarter in both.  (The kernels: tests/test_gpu_table_diff.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import table_diff_cases as D
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
INV, NODEV = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE
A = 1 << 20          # (pointers are never dereferenced on the host: plain numbers serve)
F32, BF16, F16, Q8 = (D.KINDS[k] for k in ("f32", "bf16", "f16", "q8"))


def test_header_declares_and_library_exports_the_two_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint64_t fcp_table_diff_workspace_bytes\(int64_t rows\);", text)
    assert re.search(r"\bint fcp_table_diff\(const void \*table, int32_t kind, int64_t table_rows, int32_t dim, const void \*src, int32_t src_kind,\s+"
                     r"int64_t row0, int64_t rows, int64_t \*ids_out, float \*rows_out, fcp_table_diff_report_t \*report,\s+"
                     r"void \*workspace, int32_t device, void \*stream\);", text)
    names = {"fcp_table_diff_workspace_bytes", "fcp_table_diff"}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names)
    # the header's surface and the mirror agree (tests/test_host.py holds the same for every entry)
    assert set(re.findall(r"\b(fcp_[a-z_0-9]+)\s*\(", text)) - {"fcp_alloc_fn"} == set(_lib.EXPORTS)
    assert C.sizeof(_lib.TableDiffReport) == 32
    assert [f[0] for f in _lib.TableDiffReport._fields_] == ["rows", "changed", "first_changed", "last_changed"]
    assert re.search(r"\} fcp_table_diff_report_t; /\* 32 bytes \*/", text)
    assert re.search(r"#define FCP_ABI_VERSION 2\b", text)          # the ABI is append-only


def test_workspace_bytes():
    """depends on rows only; a multiple of 8; non-decreasing; at most rows + 2^17 (the header's bound), one flag byte per row
    and the block records; -1 outside [0, 2^32 - 3); the mirrored formula"""
    L = _lib.load()
    ns = sorted(set([0, 1, 2, 7, 8, 9, 1000, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, D.LIMIT - 1, D.BIG_ROWS]
                    + [2 ** k + d for k in range(3, 32) for d in (-1, 0, 1)] + list(D.ROW_COUNTS)))
    last = 0
    for n in ns:
        b = int(L.fcp_table_diff_workspace_bytes(n))
        assert b == D.workspace_bytes(n), n
        assert b > 0 and b % 8 == 0 and b >= last and n + D.PARTIAL_BYTES <= b <= n + 2 ** 17, (n, b)
        last = b
    for n in (-1, -2 ** 40, D.LIMIT, D.LIMIT + 1, 2 ** 32, 2 ** 62, D.INT64_MIN):
        assert int(L.fcp_table_diff_workspace_bytes(n)) == -1, n


NAMES = ("table", "kind", "table_rows", "dim", "src", "src_kind", "row0", "rows", "ids_out", "rows_out", "report", "workspace")


def _diff(table, kind, table_rows, dim, src, src_kind, row0, rows, ids_out, rows_out, report, workspace, device=0):
    L = _lib.load()
    p = C.c_void_p
    status = L.fcp_table_diff(p(table), kind, table_rows, dim, p(src), src_kind, row0, rows, p(ids_out), p(rows_out), p(report), p(workspace),
                              device, None)
    return status, L.fcp_last_error().decode()


def test_status_codes_arrive_in_the_stated_order():
    import torch
    #       table kind table_rows dim src src_kind row0 rows ids_out rows_out report workspace
    good = (A, Q8, 9, 64, A, F32, 2, 3, A, A, A, A)

    def but(**kw):
        assert set(kw) <= set(NAMES)
        return tuple(kw.get(k, v) for k, v in zip(NAMES, good))

    for args, word in ((but(rows=-1), "`rows` is negative"), (but(rows=D.LIMIT), "`rows`"), (but(rows=2 ** 40), "`rows`"),
                       (but(table_rows=0), "`table_rows`"), (but(table_rows=-7), "`table_rows`"), (but(table_rows=D.LIMIT), "`table_rows`"),
                       (but(row0=-1), "`row0` is negative"), (but(row0=7), "`row0`"), (but(row0=9, rows=1), "`row0`"), (but(row0=0, rows=10), "`row0`"),
                       (but(row0=10, rows=0), "`row0`"), (but(row0=2 ** 62, rows=2 ** 31), "`row0`"),
                       (but(dim=0), "`dim`"), (but(dim=-3), "`dim`"),
                       (but(kind=-1), "`kind`"), (but(kind=4), "`kind`"), (but(kind=5, src_kind=5), "`kind`"),
                       (but(src_kind=BF16), "`src_kind`"), (but(src_kind=-1), "`src_kind`"), (but(kind=BF16, src_kind=F16), "`src_kind`"),
                       (but(kind=F32, src_kind=Q8), "`src_kind`"),
                       (but(src_kind=Q8), "`rows_out`"), (but(kind=BF16, src_kind=BF16), "`rows_out`"), (but(kind=F16, src_kind=F16, rows=0), "`rows_out`"),
                       (but(report=0), "`report` is null"), (but(report=0, rows=0), "`report` is null"),
                       (but(workspace=0), "`workspace` is null"), (but(workspace=0, rows=0), "`workspace` is null"),
                       (but(table=0), "`table` is null"), (but(src=0), "`src` is null"), (but(ids_out=0), "`ids_out` is null"),
                       (but(table=A + 2), "`table` is not 4"), (but(table=A + 8, kind=F32), "`table` is not 16"),
                       (but(table=A + 4, kind=BF16), "`table` is not 8"), (but(table=A + 2, kind=F16, dim=6), "`table` is not 4"),
                       (but(table=A + 1, kind=BF16, dim=3), "`table` is not 2"), (but(table=A + 1, dim=3), "`table` is not 4"),
                       (but(src=A + 8), "`src` is not 16"), (but(src=A + 4, dim=62), "`src` is not 8"), (but(src=A + 2, dim=61), "`src` is not 4"),
                       (but(src=A + 2, src_kind=Q8, rows_out=0), "`src` is not 4"), (but(src=A + 4, kind=BF16, src_kind=BF16, rows_out=0), "`src` is not 8"),
                       (but(ids_out=A + 4), "`ids_out` is not 8"), (but(ids_out=A + 4, rows=0), "`ids_out` is not 8"),
                       (but(rows_out=A + 8), "`rows_out` is not 16"), (but(rows_out=A + 4, dim=6), "`rows_out` is not 8"),
                       (but(rows_out=A + 1, dim=3), "`rows_out` is not 4"),
                       (but(report=A + 4), "`report` is not 8"), (but(workspace=A + 4), "`workspace` is not 8")):
        status, msg = _diff(*args)
        assert status == INV and word in msg and msg.startswith("fcp_table_diff: "), (args, status, msg)
    # the order: rows, table_rows, row0, dim, kind, src_kind, rows_out with a compact source, null report / workspace, null
    # table / src / ids_out with rows > 0, then misalignment in argument order — each call is wrong in everything that follows, too
    # (one repair at a time, and the message names what is wrong FIRST among what is left)
    bad = dict(rows=-1, table_rows=0, row0=-1, dim=0, kind=7, src_kind=9, report=0, workspace=0, table=0, src=0, ids_out=0, rows_out=A + 4)
    assert "`rows` is negative" in _diff(*but(**bad))[1]
    for name, repaired, word in (("rows", 3, "`table_rows`"), ("table_rows", 9, "`row0` is negative"), ("row0", 7, "`row0` + rows"),
                                 ("row0", 2, "`dim`"), ("dim", 64, "`kind`"), ("kind", Q8, "`src_kind`"),
                                 ("src_kind", Q8, "`rows_out` with a q8 source"), ("src_kind", F32, "`report` is null"),
                                 ("report", A + 4, "`workspace` is null"), ("workspace", A + 4, "`table` is null"), ("table", A + 2, "`src` is null"),
                                 ("src", A + 8, "`ids_out` is null"), ("ids_out", A + 4, "`table` is not 4"), ("table", A, "`src` is not 16"),
                                 ("src", A, "`ids_out` is not 8"), ("ids_out", A, "`rows_out` is not 16"), ("rows_out", A, "`report` is not 8"),
                                 ("report", A, "`workspace` is not 8")):
        bad[name] = repaired
        assert word in _diff(*but(**bad))[1], (name, repaired, word, _diff(*but(**bad))[1])
    bad["workspace"] = A
    if not torch.cuda.is_available():
        assert _diff(*but(**bad))[0] == NODEV
        # alignments that ARE enough, ids only, replicas, rows == 0 (the report is written on the device), the ends of the ranges
        for args in (good, but(rows_out=0), but(kind=F32), but(kind=BF16), but(kind=F16), but(kind=F32, src_kind=F32, rows_out=A),
                     but(src_kind=Q8, rows_out=0, src=A + 4), but(kind=BF16, src_kind=BF16, rows_out=0, src=A + 8),
                     but(kind=F16, src_kind=F16, rows_out=0, dim=61, src=A + 2, table=A + 2), but(dim=61, src=A + 4, rows_out=A + 12, table=A + 4),
                     but(dim=62, src=A + 8, rows_out=A + 8), but(rows=0), but(rows=0, table=0, src=0, ids_out=0), but(rows=0, row0=9),
                     but(row0=6), but(row0=0, rows=9), but(table_rows=D.LIMIT - 1, rows=D.LIMIT - 1, row0=0), but(table_rows=1, rows=1, row0=0)):
            assert _diff(*args)[0] == NODEV, args


def test_python_wrappers_refuse_what_they_can_see():
    import torch
    from recom_amd import tables
    table, src = torch.zeros((5, 4)), torch.zeros((3, 4))
    for fn in (tables.diff, tables.diff_async):
        with pytest.raises(ValueError, match="table: .*device to device"):          # the table's own refusal comes first
            fn(table, src)
        with pytest.raises(ValueError, match="no table format"):
            fn(torch.zeros((5, 4), dtype=torch.int32), src)
        with pytest.raises(ValueError, match="contiguous 2-D"):
            fn(torch.zeros((5, 8))[:, ::2], src)
    for fn in (tables.diff_from_host, tables.sync_from_host):
        with pytest.raises(ValueError, match=r"takes a float32 \[rows, dim\] tensor on the host"):
            fn(table, torch.zeros((5, 4), dtype=torch.float64))
        with pytest.raises(ValueError, match=r"takes a float32 \[rows, dim\] tensor on the host"):
            fn(table, torch.zeros((20,)))
        with pytest.raises(ValueError, match="chunk_rows must be positive"):
            fn(table, torch.zeros((5, 4)), chunk_rows=0)
        with pytest.raises(ValueError, match="device to device"):                   # a host table: the table's own refusal
            fn(table, torch.zeros((5, 4)))
    r = tables.DiffReport(4, 2, 1, 3)
    assert (r.rows, r.changed, r.first_changed, r.last_changed) == (4, 2, 1, 3)
    with pytest.raises(Exception):
        r.rows = 5                                                                  # frozen


def _row_loop(new_bytes, stored, row0):
    """the plain restatement: one row after the other, one byte after the other"""
    ids = []
    for i in range(len(stored)):
        if any(int(a) != int(b) for a, b in zip(new_bytes[i], stored[i])):
            ids.append(row0 + i)
    return ids


def test_the_restatement_against_a_row_loop():
    rng = np.random.default_rng(11)
    for rows, width, row0 in ((0, 4, 0), (1, 1, 0), (1, 3, 9), (7, 12, 0), (200, 9, 1000), (64, 72, 2 ** 31)):
        stored = rng.integers(0, 256, (rows, width)).astype(np.uint8)
        new = stored.copy()
        hit = rng.random(rows) < 0.4
        at = rng.integers(0, width, rows)
        new[np.flatnonzero(hit), at[hit]] ^= np.uint8(1 << 3)
        ids, report, ids_out = D.diff_ref(new, stored, row0)
        want = _row_loop(new, stored, row0)
        assert ids.tolist() == want == (np.flatnonzero(hit) + row0).tolist() and ids.dtype == ids_out.dtype == np.int64
        m = len(want)
        assert ids_out.shape == (rows,) and ids_out[:m].tolist() == want and (ids_out[m:] == -1).all()
        assert report == {"rows": rows, "changed": m, "first_changed": want[0] if m else -1, "last_changed": want[-1] if m else -1}
    # bits, not values: -0.0 differs from +0.0, two NaNs with equal bits do not, two NaNs with different payloads do
    x = np.asarray([[0.0, 1.0], [np.nan, 2.0], [np.nan, 3.0]], np.float32)
    y = x.copy()
    y[0, 0] = -0.0
    y.view(np.uint32)[2, 0] ^= 1
    assert D.diff_ref(D.ref_bytes(y, "f32"), D.ref_bytes(x, "f32"))[0].tolist() == [0, 2]
    # the bytes are those of the formats: their sizes, the q8 tail, one rounding to 16 bits
    x = np.asarray([[1.0, 2.0, 4.0]], np.float32)
    assert [D.ref_bytes(x, k).shape[1] for k in ("f32", "bf16", "f16", "q8")] == [D.row_bytes(k, 3) for k in ("f32", "bf16", "f16", "q8")] == [12, 6, 6, 11]
    assert D.ref_bytes(x, "q8")[0].tolist() == [0, 85, 255] + list(np.float32(3.0 / 255.0).tobytes()) + list(np.float32(1.0).tobytes())
    assert D.ref_bytes(x, "bf16").view(np.uint16)[0].tolist() == [0x3F80, 0x4000, 0x4080]
    assert D.ref_bytes(x, "f16").view(np.uint16)[0].tolist() == [0x3C00, 0x4000, 0x4400]


def test_the_geometry_and_the_sizes():
    assert D.chunk_for(1) == D.chunk_for(D.FULL_PASS) == D.MIN_CHUNK and D.chunk_for(D.BIG_ROWS) == D.MIN_CHUNK + D.TILE
    assert {1, 2, 63, 64, 65, D.TILE - 1, D.TILE + 1, D.MIN_CHUNK - 1, D.MIN_CHUNK + 1} <= set(D.ROW_COUNTS) and D.BIG_ROWS == D.FULL_PASS + 1
    assert set(D.DIMS) == {1, 2, 3, 4, 6, 62, 64, 300} and all(D.dims_of(k) == D.DIMS + (1028,) for k in D.KINDS) and 1028 > 64 * D.Q_SLOTS * 4
    assert 300 // 4 > 64                    # beyond one 64-lane group's reach
    assert set(D.quiet_dims("q8")) == set(D.dims_of("q8")) - {1, 2} and D.quiet_dims("f16") == D.dims_of("f16")


def test_the_selection_s_edge_cells_stand_on_the_delta_s_sizes():
    """the edge cells of tests/test_gpu_table_diff.py: the size list of tests/table_delta_cases.py in this grid's terms, and a
    mixed pattern with a changed row on both sides of every wave boundary — every tile boundary is one"""
    assert set(D.EDGE_ROW_COUNTS) == {1, 2, 63, 64, 65, D.TILE - 1, D.TILE, D.TILE + 1, D.MIN_CHUNK - 1, D.MIN_CHUNK, D.MIN_CHUNK + 1,
                                      D.FULL_PASS + 1}
    assert D.EDGE_PATTERNS == ("none", "all", "wave_edges") and D.TILE % D.WAVE == 0
    for rows in D.ROW_COUNTS:
        mask = D.mask_of("wave_edges", rows)
        for edge in range(D.WAVE, rows, D.WAVE):
            assert mask[edge - 1] and mask[edge]
        assert mask.sum() == rows // D.WAVE + (rows - 1) // D.WAVE and not mask[0] and (rows < 3 or not mask[1:D.WAVE - 1].any())
        assert (D.mask_of("tile_edges", rows) <= mask).all()
    assert D.EDGE_DIMS == (4, 6)        # float32 rows copied by V 4 / G 1 and by V 2 / G 4, as the delta's sweep copies them


@pytest.mark.parametrize("kind", tuple(D.KINDS))
def test_every_pattern_contains_what_it_is_for(kind):
    """From the reference alone: the rows a pattern means to change are the rows whose bytes change in every format, nothing
    else does; `none` hands over the stored master; `last_element` differs from it in the last element only."""
    for dim in D.dims_of(kind):
        v = D.variants(kind, dim)
        for rows in D.ROW_COUNTS:
            for pattern in D.PATTERNS:
                if pattern == "quiet":
                    continue
                base, stored, new, new_bytes = v.case(pattern, rows)
                assert (D.ref_bytes(new, kind) == new_bytes).all() and (D.ref_bytes(base, kind) == stored).all()
                ids, report, _o = D.diff_ref(new_bytes, stored)
                want = np.flatnonzero(D.mask_of(pattern, rows))
                assert ids.tolist() == want.tolist(), (kind, dim, rows, pattern)
                differ = (new.view(np.uint32) != base.view(np.uint32))
                assert (differ.any(axis=1) == D.mask_of(pattern, rows)).all() and differ.sum() == len(want)
                if pattern == "last_element":
                    assert differ[:, -1].sum() == len(want)
                if pattern == "none":
                    assert report["changed"] == 0 and report["first_changed"] == -1
                if pattern == "all":
                    assert report["changed"] == rows and (report["first_changed"], report["last_changed"]) == (0, rows - 1)
                if pattern == "tile_edges" and rows > D.TILE:
                    assert {D.TILE - 1, D.TILE} <= set(ids.tolist())


@pytest.mark.parametrize("kind", tuple(D.KINDS))
def test_the_quiet_pattern_is_quiet_and_loud(kind):
    """The condition on the QUIET pattern, from the reference alone: every row differs from the stored master in its float32
    bits; for the compact formats at least 25 % of the rows are QUIET — the format's bytes are equal — and at least 25 % are
    LOUD, in every dim and at every row count from 2 on (one row cannot be both).  A float32 table sees every row."""
    for dim in D.quiet_dims(kind):
        v = D.variants(kind, dim)
        for rows in D.ROW_COUNTS:
            if rows < 2:
                continue
            base, stored, new, new_bytes = v.case("quiet", rows)
            assert (D.ref_bytes(new, kind) == new_bytes).all() and (D.ref_bytes(base, kind) == stored).all()
            bits_differ = (new.view(np.uint32) != base.view(np.uint32)).any(axis=1)
            assert bits_differ.all()
            ids, report, _o = D.diff_ref(new_bytes, stored)
            changed = np.zeros(rows, bool)
            changed[ids] = True
            if kind == "f32":
                assert changed.all()
                continue
            quiet_rows, loud_rows = (bits_differ & ~changed).sum(), changed.sum()
            assert 4 * quiet_rows >= rows and 4 * loud_rows >= rows, (kind, dim, rows, quiet_rows, loud_rows)
            assert (changed == (np.arange(rows) % 2 == 1)).all(), (kind, dim, rows)      # interleaved: even rows QUIET, odd rows LOUD


def test_the_special_rows_hold_what_they_are_for():
    x = D.special_rows(200, 6)
    w = x.view(np.uint32)
    assert np.isnan(x).any() and np.isinf(x).any() and (w == 0x80000000).any() and (w == 0).any() and (w == 1).any()
    y = D.special_changes(x)
    d = (y.view(np.uint32) != w).any(axis=1)
    assert (d == (np.arange(200) % 4 != 0)).all()
    for kind in ("bf16", "f16"):
        ids = D.diff_ref(D.ref_bytes(y, kind), D.ref_bytes(x, kind))[0]
        # sign flips and new rows show in 16 bits; most low-bit flips do not
        assert set(np.flatnonzero(np.arange(200) % 4 == 1).tolist()) <= set(ids.tolist()) and 100 <= len(ids) < 150
