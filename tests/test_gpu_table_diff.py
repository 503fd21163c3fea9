"""fcp_table_diff on the GPU (recom_amd/csrc/fcp_table_diff.hip) against the NumPy restatement of tests/table_diff_cases.py: the
tables are built with tables.convert from a base master, and ids_out, rows_out[:m] (as 32-bit patterns), the -1 tail and the
report are EQUAL to diff_ref's for every format, at every dim where the kernels take another V or G, at every row count where
they take another path, for every change pattern — the QUIET one among them, whose float32 rows differ and whose bytes in the
format do not.  Guards around every output stay untouched, rows >= m of rows_out keep their poison, inputs are only read.
16-bit rows whose bits matter are held to the composition the entry replaces (convert into a temporary, a torch byte compare);
a replica of the table's own format gives the same ids and refuses rows_out; the workspace's content and a second run change
nothing.

(The references on themselves, and every pattern shown to contain what it is for: tests/test_table_diff_host.py.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import table_diff_cases as D

pytestmark = pytest.mark.gpu

GUARD = 64           # bytes of 0x5A in front of and behind every output (a multiple of every alignment asked for)
POISON = 0x5A


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _guarded(torch, nbytes, dev, fill=POISON):
    buf = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev)
    if fill != POISON:
        buf[GUARD:GUARD + nbytes] = fill
    return buf


def _table_of(torch, master, kind, dev):
    """the device table of `kind` tables.convert writes from the float32 master (float32: the master itself)"""
    from recom_amd import tables
    t = torch.from_numpy(np.array(master, np.float32)).to(dev)          # (a copy: the cases are read-only)
    return t if kind == "f32" else tables.convert(t, kind)


def _bytes_of(torch, t):
    return t.cpu().contiguous().view(torch.uint8).numpy().reshape(t.shape[0], -1)


def _run(torch, table, kind, dim, src, src_kind="f32", row0=0, with_rows=True, ws_fill=0xC3):
    """One call of the C entry on guarded, poisoned outputs; `table` and `src` are device tensors.  Returns the raw bytes of
    every output buffer, guards included."""
    from recom_amd import lib
    L = lib.load()
    dev = table.device
    rows = int(src.shape[0])
    need = int(L.fcp_table_diff_workspace_bytes(rows))
    assert need == D.workspace_bytes(rows)
    before = (_bytes_of(torch, table), _bytes_of(torch, src)) if rows <= D.MAX_ROWS else None
    bufs = {"ids_out": _guarded(torch, 8 * rows, dev), "report": _guarded(torch, 32, dev), "workspace": _guarded(torch, need, dev, ws_fill)}
    if with_rows:
        bufs["rows_out"] = _guarded(torch, 4 * rows * dim, dev)
    ptr = lambda name: C.c_void_p(bufs[name].data_ptr() + GUARD) if name in bufs else None   # noqa: E731
    status = L.fcp_table_diff(C.c_void_p(table.data_ptr()), D.KINDS[kind], int(table.shape[0]), dim, C.c_void_p(src.data_ptr()),
                              D.KINDS[src_kind], row0, rows, ptr("ids_out"), ptr("rows_out"), ptr("report"), ptr("workspace"), 0,
                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    lib.check(status, "fcp_table_diff")
    torch.cuda.synchronize()
    # (of the workspace only the guards come back: its content means nothing)
    out = {k: (torch.cat([v[:GUARD], v[-GUARD:]]) if k == "workspace" else v).cpu().numpy() for k, v in bufs.items()}
    if before is not None:                                                               # inputs are only read
        assert (_bytes_of(torch, table) == before[0]).all() and (_bytes_of(torch, src) == before[1]).all()
    return out


def _payload(raw, dtype=np.uint8):
    return raw[GUARD:len(raw) - GUARD].view(dtype)


def _check(out, want, new, what, row0=0):
    """every output against diff_ref's (ids, report, ids_out), every guard, the poison behind the changed rows; `new`: the
    float32 source rows, whose row i is the candidate for table row row0 + i (None: ids only)"""
    ids, report, ids_out = want
    m, rows = len(ids), report["rows"]
    for name, raw in out.items():
        assert (raw[:GUARD] == POISON).all() and (raw[len(raw) - GUARD:] == POISON).all(), (what, name, "guard")
    got = _payload(out["report"], np.int64)
    assert got.tolist() == [report["rows"], report["changed"], report["first_changed"], report["last_changed"]], (what, got, report)
    got = _payload(out["ids_out"], np.int64)
    assert (got == ids_out).all(), (what, "ids_out", np.flatnonzero(got != ids_out)[:5], got[:5], ids_out[:5], m)
    if "rows_out" in out:
        dim = new.shape[1]
        got = _payload(out["rows_out"], np.uint32).reshape(rows, dim)
        bad = np.flatnonzero((got[:m] != new.view(np.uint32)[ids - row0]).any(axis=1))
        assert bad.size == 0, (what, "rows_out", bad[:5], m)
        assert (_payload(out["rows_out"])[4 * dim * m:] == POISON).all(), (what, "rows behind the changed ones were touched")
    return report


CASES = [(kind, dim) for kind in D.KINDS for dim in D.dims_of(kind)]


@pytest.mark.parametrize("kind,dim", CASES)
def test_equal_to_the_restatement(torch_cuda, kind, dim):
    """Every row count and every change pattern of one format and dim, with rows_out: the table is tables.convert of the base
    master (checked once against the reference's bytes), the source the pattern's new master."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    v = D.variants(kind, dim)
    for name in ("base", "grid"):
        assert (_bytes_of(torch, _table_of(torch, v.src[name], kind, dev)) == v.bytes[name]).all(), (kind, dim, name, "tables.convert")
    ran = 0
    for rows in D.ROW_COUNTS:
        tables_of = {name: _table_of(torch, v.src[name][:rows], kind, dev) for name in ("base", "grid")}
        for pattern in D.PATTERNS:
            _base, stored, new, new_bytes = v.case(pattern, rows)
            want = D.diff_ref(new_bytes, stored)
            out = _run(torch, tables_of["grid" if pattern == "quiet" else "base"], kind, dim, torch.from_numpy(new).to(dev))
            report = _check(out, want, new, {"kind": kind, "dim": dim, "rows": rows, "pattern": pattern})
            ran += 1
            if pattern == "none":
                # nothing changed: ids_out all -1, rows_out untouched (its poison), first_changed -1
                assert report["changed"] == 0 and report["first_changed"] == -1 and report["last_changed"] == -1
                assert (_payload(out["ids_out"], np.int64) == -1).all() and (_payload(out["rows_out"]) == POISON).all()
            if pattern == "all":
                assert report["changed"] == rows
            if pattern == "quiet" and kind != "f32" and rows >= 2 and dim in D.quiet_dims(kind):
                assert report["changed"] == rows // 2           # the odd rows: LOUD; the even rows' float32 bits differ and are not reported
    assert ran == len(D.ROW_COUNTS) * len(D.PATTERNS)


@pytest.mark.parametrize("dim", (1, 2, 3, 4))
@pytest.mark.parametrize("kind", tuple(D.KINDS))
def test_one_full_pass_of_the_grid_and_one_row(torch_cuda, kind, dim):
    """FULL_PASS + 1 rows: the chunk of a block grows by a tile and the last block holds what is left.  Every third row
    changed, and the last."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    rows = D.BIG_ROWS
    assert D.chunk_for(rows) > D.chunk_for(rows - 1)
    base = D.base_rows(rows, dim, seed=3)
    mask = D.mask_of("every3", rows) | D.mask_of("last", rows)
    new = np.where(mask[:, None], D.loud(base), base)
    want = D.diff_ref(D.ref_bytes(new, kind), D.ref_bytes(base, kind))
    assert want[0].tolist() == np.flatnonzero(mask).tolist()
    out = _run(torch, _table_of(torch, base, kind, dev), kind, dim, torch.from_numpy(new).to(dev))
    report = _check(out, want, new, {"kind": kind, "dim": dim, "rows": rows})
    assert report["last_changed"] == rows - 1 and report["first_changed"] == 1


@functools.lru_cache(maxsize=None)
def _edge_rows(dim):
    """(base, loud(base)) float32 at the largest row count an edge cell of `dim` takes, read-only: a prefix serves every count"""
    rows = D.BIG_ROWS if dim == 4 else D.MAX_ROWS
    base = D.base_rows(rows, dim, seed=11)
    changed = D.loud(base)
    base.setflags(write=False)
    changed.setflags(write=False)
    return base, changed


@pytest.mark.parametrize("pattern", D.EDGE_PATTERNS)
def test_the_selection_s_edges(torch_cuda, pattern):
    """What fcp_table_delta_distinct's size sweep holds the shared compact body to, held to it through this entry: nothing
    changed, every row changed, and changed rows on both sides of every wave and tile boundary, at one row, two, a wave -+ 1, a
    tile -+ 1, a chunk -+ 1 and one full pass of the fixed grid + 1; float32 against float32, rows_out by V 4 / G 1 (dim 4)
    and by V 2 / G 4 (dim 6; not at the full pass)."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    for dim in D.EDGE_DIMS:
        base, changed = _edge_rows(dim)
        for rows in D.EDGE_ROW_COUNTS:
            if rows > len(base):
                continue
            mask = D.mask_of(pattern, rows)
            new = np.where(mask[:, None], changed[:rows], base[:rows])
            want = D.diff_ref(D.ref_bytes(new, "f32"), D.ref_bytes(base[:rows], "f32"))
            assert want[0].tolist() == np.flatnonzero(mask).tolist()
            out = _run(torch, _table_of(torch, base[:rows], "f32", dev), "f32", dim, torch.from_numpy(new).to(dev))
            report = _check(out, want, new, {"dim": dim, "rows": rows, "pattern": pattern})
            assert report["changed"] == {"none": 0, "all": rows, "wave_edges": rows // D.WAVE + (rows - 1) // D.WAVE}[pattern]
    assert D.BIG_ROWS in D.EDGE_ROW_COUNTS and D.chunk_for(D.BIG_ROWS) > D.chunk_for(D.BIG_ROWS - 1)


@pytest.mark.parametrize("kind", tuple(D.KINDS))
def test_row0_against_a_larger_table(torch_cuda, kind):
    """row0 > 0: the source holds the candidates of a run of rows inside a table larger than the call's chunk; the rows outside
    the run differ from the source and are not reported.  The run's end at the table's last row, too."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    for dim in (3, 6, 64):
        table_rows = D.MIN_CHUNK + 301
        master = D.base_rows(table_rows, dim, seed=5)
        stored_all = D.ref_bytes(master, kind)
        table = _table_of(torch, master, kind, dev)
        for row0, rows in ((517, 300), (table_rows - 65, 65), (1, D.MIN_CHUNK + 1), (table_rows - 1, 1), (0, table_rows)):
            mask = D.mask_of("every3", rows) | D.mask_of("first", rows)
            new = np.where(mask[:, None], D.loud(master[row0:row0 + rows]), master[row0:row0 + rows])
            want = D.diff_ref(D.ref_bytes(new, kind), stored_all[row0:row0 + rows], row0)
            assert want[0].tolist() == (np.flatnonzero(mask) + row0).tolist() and want[1]["first_changed"] == row0
            # the table's rows 0 .. rows - 1 are not the source's: an entry that forgot row0 would report them
            assert rows in (1, table_rows) or (D.ref_bytes(new, kind) != stored_all[:rows]).any(axis=1).sum() > len(want[0])
            out = _run(torch, table, kind, dim, torch.from_numpy(new).to(dev), row0=row0)
            _check(out, want, new, {"kind": kind, "dim": dim, "rows": rows, "row0": row0}, row0=row0)


@pytest.mark.parametrize("dim", (1, 6, 64, 300))
@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_rows_whose_bits_matter_against_the_composition(torch_cuda, kind, dim):
    """16-bit rows with NaNs (payloads, both signs), +-inf, -0.0 and subnormals: the ids are those of the composition the entry
    replaces — fcp_table_convert of the new rows into a temporary on the device, then a torch byte compare.  (A NaN's 16-bit
    payload is the library's own choice: only the library can say whether the stored bytes change.)"""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    rows = D.MIN_CHUNK + 77
    base = D.special_rows(rows, dim, seed=dim)
    new = D.special_changes(base, seed=dim)
    table = _table_of(torch, base, kind, dev)
    d_new = torch.from_numpy(new).to(dev)
    temporary = tables.convert(d_new, kind)
    changed = (temporary.view(torch.int16) != table.view(torch.int16)).any(dim=1)
    want_ids = torch.nonzero(changed).view(-1).cpu().numpy().astype(np.int64)
    assert 0 < len(want_ids) < rows and set(np.flatnonzero(np.arange(rows) % 4 == 0).tolist()).isdisjoint(want_ids.tolist())
    ids_out = np.full(rows, -1, np.int64)
    ids_out[:len(want_ids)] = want_ids
    report = {"rows": rows, "changed": len(want_ids), "first_changed": int(want_ids[0]), "last_changed": int(want_ids[-1])}
    out = _run(torch, table, kind, dim, d_new)
    _check(out, (want_ids, report, ids_out), new, {"kind": kind, "dim": dim, "specials": True})
    # float32 against float32: a compare of bits — -0.0 differs from +0.0, equal NaNs do not, a payload bit does
    want = D.diff_ref(D.ref_bytes(new, "f32"), D.ref_bytes(base, "f32"))
    assert want[0].tolist() == np.flatnonzero(np.arange(rows) % 4 != 0).tolist()
    _check(_run(torch, torch.from_numpy(base).to(dev), "f32", dim, d_new), want, new, {"kind": "f32", "dim": dim, "specials": True})


@pytest.mark.parametrize("kind", D.COMPACT)
def test_a_replica_of_the_same_format(torch_cuda, kind):
    """src_kind == kind: the rows of another replica, compared byte for byte — the ids of the master's diff; ids only, and a
    rows_out is refused by the entry and by the wrapper."""
    torch = torch_cuda
    from recom_amd import lib, tables
    dev = torch.device("cuda", 0)
    for dim in (1, 3, 6, 64, 300, D.CAP_DIM):
        v = D.variants(kind, dim)
        for rows, pattern in ((D.MIN_CHUNK, "none"), (1, "all"), (65, "every3"), (D.TILE + 1, "tile_edges"), (D.MIN_CHUNK + 1, "quiet"),
                              (D.MIN_CHUNK + 1, "last_element")):
            _base, stored, new, new_bytes = v.case(pattern, rows)
            want = D.diff_ref(new_bytes, stored)
            table = _table_of(torch, v.src["grid" if pattern == "quiet" else "base"][:rows], kind, dev)
            replica = _table_of(torch, new, kind, dev)
            out = _run(torch, table, kind, dim, replica, src_kind=kind, with_rows=False)
            assert "rows_out" not in out
            _check(out, want, None, {"kind": kind, "dim": dim, "rows": rows, "pattern": pattern, "replica": True})
    got_ids, got_rows, got_report = tables.diff(table, replica, want_rows=False)
    assert got_rows is None and got_ids.cpu().numpy().tolist() == want[0].tolist() and got_report == tables.DiffReport(**want[1])
    with pytest.raises(ValueError, match="replica gives ids only"):
        tables.diff(table, replica)
    L = lib.load()
    scratch = torch.zeros((1 << 16,), dtype=torch.int64, device=dev)
    p = C.c_void_p(scratch.data_ptr())
    status = L.fcp_table_diff(C.c_void_p(table.data_ptr()), D.KINDS[kind], rows, dim, C.c_void_p(replica.data_ptr()), D.KINDS[kind], 0, rows,
                              p, p, p, p, 0, None)
    assert status == lib.FCP_ERR_INVALID_ARGUMENT and "`rows_out`" in L.fcp_last_error().decode()
    # float32 is its own replica: the two modes coincide, and rows_out is allowed
    v = D.variants("f32", 6)
    _base, stored, new, new_bytes = v.case("every3", 300)
    out = _run(torch, _table_of(torch, v.src["base"][:300], "f32", dev), "f32", 6, torch.from_numpy(new).to(dev), src_kind="f32")
    _check(out, D.diff_ref(new_bytes, stored), new, "f32 replica")


@pytest.mark.parametrize("kind", tuple(D.KINDS))
def test_ids_only_and_no_rows_at_all(torch_cuda, kind):
    torch = torch_cuda
    from recom_amd import lib
    dev = torch.device("cuda", 0)
    dim = 62
    v = D.variants(kind, dim)
    for rows, pattern in ((1, "none"), (64, "all"), (D.MIN_CHUNK + 1, "every3"), (D.MIN_CHUNK + 1, "quiet")):
        _base, stored, new, new_bytes = v.case(pattern, rows)
        table = _table_of(torch, v.src["grid" if pattern == "quiet" else "base"][:rows], kind, dev)
        out = _run(torch, table, kind, dim, torch.from_numpy(new).to(dev), with_rows=False)
        assert set(out) == {"ids_out", "report", "workspace"}
        _check(out, D.diff_ref(new_bytes, stored), None, (kind, rows, pattern, "ids only"))
    # rows == 0: the report is written, nothing else is touched; null table, src and ids_out are accepted
    L = lib.load()
    report = torch.full((4,), 7, dtype=torch.int64, device=dev)
    ws = torch.empty((int(L.fcp_table_diff_workspace_bytes(0)) // 8,), dtype=torch.int64, device=dev)
    lib.check(L.fcp_table_diff(None, D.KINDS[kind], 5, dim, None, D.KINDS["f32"], 5, 0, None, None, C.c_void_p(report.data_ptr()),
                               C.c_void_p(ws.data_ptr()), 0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "fcp_table_diff")
    torch.cuda.synchronize()
    assert report.cpu().tolist() == [0, 0, -1, -1]


@pytest.mark.parametrize("kind", tuple(D.KINDS))
def test_the_workspace_and_a_second_run_change_nothing(torch_cuda, kind):
    """the same call with the workspace pre-filled with 0xFF, with 0x00, and once more: identical bytes in every output"""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    dim, rows = 6, 3 * D.MIN_CHUNK + 5
    base = D.base_rows(rows, dim, seed=9)
    mask = D.mask_of("every3", rows) | D.mask_of("tile_edges", rows)
    new = np.where(mask[:, None], D.loud(base), base)
    table, d_new = _table_of(torch, base, kind, dev), torch.from_numpy(new).to(dev)
    runs = [_run(torch, table, kind, dim, d_new, ws_fill=fill) for fill in (0xFF, 0x00, 0x00)]
    _check(runs[0], D.diff_ref(D.ref_bytes(new, kind), D.ref_bytes(base, kind)), new, (kind, "workspace"))
    for other in runs[1:]:
        for name in ("ids_out", "rows_out", "report"):
            assert (runs[0][name] == other[name]).all(), (kind, name)


def test_the_wrappers(torch_cuda):
    """tables.diff slices at m and returns a DiffReport; the async form returns the padded tensors; row0; what the wrappers
    refuse of device tensors"""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    kind, dim, rows, row0 = "q8", 20, 700, 41
    master = D.base_rows(row0 + rows + 9, dim, seed=2)
    mask = D.mask_of("every3", rows)
    new = np.where(mask[:, None], D.loud(master[row0:row0 + rows]), master[row0:row0 + rows])
    ids, report, ids_out = D.diff_ref(D.ref_bytes(new, kind), D.ref_bytes(master, kind)[row0:row0 + rows], row0)
    m = len(ids)
    table, d_new = _table_of(torch, master, kind, dev), torch.from_numpy(new).to(dev)
    got_ids, got_rows, got_report = tables.diff(table, d_new, row0=row0)
    assert got_report == tables.DiffReport(**report) and got_ids.cpu().numpy().tolist() == ids.tolist()
    assert got_rows.shape == (m, dim) and (got_rows.cpu().numpy().view(np.uint32) == new.view(np.uint32)[ids - row0]).all()
    got_ids, got_rows, got_report = tables.diff(table, d_new, row0=row0, want_rows=False)
    assert got_rows is None and got_ids.cpu().numpy().tolist() == ids.tolist() and got_report.changed == m
    a_ids, a_rows, a_report = tables.diff_async(table, d_new, row0=row0)
    torch.cuda.synchronize()
    assert a_ids.shape == (rows,) and a_rows.shape == (rows, dim) and (a_ids.cpu().numpy() == ids_out).all()
    assert a_report.cpu().tolist() == [rows, m, report["first_changed"], report["last_changed"]]
    with pytest.raises(ValueError, match="do not lie in a table of 750 rows"):
        tables.diff(table, d_new, row0=row0 + 10)
    with pytest.raises(ValueError, match="src has rows of dim 19"):
        tables.diff(table, d_new[:, :19].contiguous())
    with pytest.raises(ValueError, match="compared with a float32 master or a q8 replica"):
        tables.diff(table, d_new.to(torch.bfloat16), want_rows=False)
    with pytest.raises(ValueError, match="src: .*device to device"):
        tables.diff(table, torch.from_numpy(new))
