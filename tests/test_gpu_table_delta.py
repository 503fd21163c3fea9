"""fcp_table_delta_distinct on the GPU (recom_amd/csrc/fcp_table_delta.hip) against the NumPy restatement of
tests/table_delta_cases.py: ids_out, pos_out, rows_out[:m] (as 32-bit patterns) and the report are EQUAL to distinct_ref's for
int64 and int32 ids at every size where the kernels take another path, for every id pattern and table size; ids outside the
table are skipped and shadow nothing; guards around every output stay untouched, rows >= m of rows_out keep their poison, the
tails are -1; rows are copied as bits at every V and G; the workspace's content and a second run change nothing; an already
distinct delta comes back as it went in; and tables.apply_delta leaves a table of every format byte for byte what
tables.convert writes from the sequentially updated master, with the digest kept.

Every kernel here gets well-formed memory: only id VALUES are adversarial.  (The references on themselves, and every pattern
shown to contain what it is for: tests/test_table_delta_host.py.)"""
import ctypes as C

import numpy as np
import pytest

import table_convert_cases as TC
import table_delta_cases as D
import table_rows_cases as R

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


def _run(torch, ids, rows, table_rows, with_pos=True, ws_fill=0xC3):
    """One call of the C entry on guarded, poisoned outputs.  Returns the raw bytes of every output buffer, guards included."""
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    n = len(ids)
    d_ids = torch.from_numpy(ids).to(dev)
    d_rows = torch.from_numpy(rows).to(dev) if rows is not None else None
    dim = rows.shape[1] if rows is not None else -9       # (ids only: dim is not read)
    need = int(L.fcp_table_delta_workspace_bytes(n))
    assert need == D.workspace_bytes(n)
    bufs = {"ids_out": _guarded(torch, 8 * n, dev), "report": _guarded(torch, 32, dev), "workspace": _guarded(torch, need, dev, ws_fill)}
    if with_pos:
        bufs["pos_out"] = _guarded(torch, 8 * n, dev)
    if rows is not None:
        bufs["rows_out"] = _guarded(torch, rows.nbytes, dev)
    ptr = lambda name: C.c_void_p(bufs[name].data_ptr() + GUARD) if name in bufs else None   # noqa: E731
    status = L.fcp_table_delta_distinct(C.c_void_p(d_ids.data_ptr()), ids.itemsize, C.c_void_p(d_rows.data_ptr()) if rows is not None else None,
                                        dim, n, table_rows, ptr("ids_out"), ptr("rows_out"), ptr("pos_out"), ptr("report"), ptr("workspace"),
                                        0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    lib.check(status, "fcp_table_delta_distinct")
    torch.cuda.synchronize()
    # (of the workspace only the guards come back: its content means nothing)
    out = {k: (torch.cat([v[:GUARD], v[-GUARD:]]) if k == "workspace" else v).cpu().numpy() for k, v in bufs.items()}
    assert (d_ids.cpu().numpy() == ids).all()                                             # inputs are only read
    if rows is not None:
        assert (d_rows.cpu().numpy().view(np.uint32) == rows.view(np.uint32)).all()
    return out


def _payload(raw, dtype=np.uint8):
    return raw[GUARD:len(raw) - GUARD].view(dtype)


def _check(out, ids, rows, table_rows, what):
    """every output against distinct_ref, every guard, the poison behind the winners' rows"""
    pos, report, ids_out, pos_out = D.distinct_ref(ids, table_rows)
    m = len(pos)
    for name, raw in out.items():
        assert (raw[:GUARD] == POISON).all() and (raw[len(raw) - GUARD:] == POISON).all(), (what, name, "guard")
    got = _payload(out["report"], np.int64)
    assert got.tolist() == [report["n"], report["distinct"], report["duplicates"], report["skipped"]], (what, got, report)
    got = _payload(out["ids_out"], np.int64)
    assert (got == ids_out).all(), (what, "ids_out", np.flatnonzero(got != ids_out)[:5], m)
    if "pos_out" in out:
        got = _payload(out["pos_out"], np.int64)
        assert (got == pos_out).all(), (what, "pos_out", np.flatnonzero(got != pos_out)[:5], m)
    if rows is not None:
        dim = rows.shape[1]
        got = _payload(out["rows_out"], np.uint32).reshape(len(ids), dim)
        bad = np.flatnonzero((got[:m] != rows.view(np.uint32)[pos]).any(axis=1))
        assert bad.size == 0, (what, "rows_out", bad[:5], m)
        assert (_payload(out["rows_out"])[4 * dim * m:] == POISON).all(), (what, "rows behind the winners were touched")
    return report


SWEEP_DIMS = {np.int64: 4, np.int32: 6}      # rows of the size sweep: V 4 with G 1 beside int64 ids, V 2 with G 4 beside int32 ids


@pytest.mark.parametrize("pattern", D.PATTERNS)
@pytest.mark.parametrize("n", D.SIZES)
def test_equal_to_the_restatement(torch_cuda, n, pattern):
    """int64 and int32 ids WITH rows and pos_out, in every table size of table_delta_cases.table_rows_options (1, 2, n / 2, more
    rows than LDS cells; the global pattern also in the table its chains need, the hot head also in one where everything but
    the head is distinct, all-distinct ids in tables of n rows and more): ids_out, pos_out, rows_out[:m] and the report."""
    ran = 0
    for table_rows in D.table_rows_options(n, pattern):
        ids = D.draw_ids(pattern, n, table_rows)
        for dtype, dim in SWEEP_DIMS.items():
            what = (pattern, n, table_rows, np.dtype(dtype).name)
            typed = ids.astype(dtype)
            rows = D.special_rows(n, dim, 7)
            report = _check(_run(torch_cuda, typed, rows, table_rows), typed, rows, table_rows, what)
            ran += 1
            if pattern == "equal":
                assert report["distinct"] == 1
            if pattern == "distinct":
                assert report["duplicates"] == 0 and report["distinct"] == n
    assert ran >= 2 * 2, (n, pattern, ran)       # no case may run nothing: at least two tables, both id types


@pytest.mark.parametrize("table_rows", (1, 2, 1000, D.LIMIT - 1))
def test_ids_outside_the_table(torch_cuda, table_rows):
    """-1, table_rows, 2^32 + a valid row, INT64_MIN and negative int32 ids: counted in skipped, never winners, and no valid
    id is shadowed by one — alone, and spread over more than one block's chunk of ids inside the table."""
    rng = np.random.default_rng(table_rows % 1000)
    for o in (D.outside_ids(table_rows), D.outside_ids32(table_rows)):
        report = _check(_run(torch_cuda, o, None, table_rows), o, None, table_rows, ("outside", table_rows, o.dtype))
        assert report["skipped"] == (9 if o.dtype == np.int64 else 4) and report["distinct"] == min(table_rows, 2)
        n = 2 * D.MIN_CHUNK + 77
        ids = rng.integers(0, min(table_rows, 2 ** 31 - 1), n).astype(o.dtype)
        at = rng.permutation(n)[:40 * len(o)]
        ids[at] = np.tile(o, 40)
        rows = D.special_rows(n, 4, 1)
        report = _check(_run(torch_cuda, ids, rows, table_rows), ids, rows, table_rows, ("outside in a crowd", table_rows, o.dtype))
        assert report["skipped"] == 40 * (9 if o.dtype == np.int64 else 4)


@pytest.mark.parametrize("dim", D.ROW_DIMS)
def test_rows_are_copied_as_bits(torch_cuda, dim):
    """every V (dims 1, 2, 3, 4, 6, 62, 64, 300), G = 1, the groups and beyond a 64-lane group's reach: NaN payloads, -0.0,
    subnormals and random words arrive as they left, at the winners' ranks; rows behind them keep the poison; with and
    without pos_out."""
    assert TC.vec_of(dim) in (1, 2, 4)
    for n, pattern, table_rows in ((1, "equal", 7), (65, "hot_head", 40), (D.TILE + 1, "zipf", D.BIG_ROWS), (D.MIN_CHUNK + 1, "twice_reversed", D.BIG_ROWS),
                                   (2 * D.MIN_CHUNK + 3, "distinct", D.BIG_ROWS)):
        ids = D.draw_ids(pattern, n, table_rows)
        rows = D.special_rows(n, dim, n)
        for with_pos in (True, False):
            _check(_run(torch_cuda, ids, rows, table_rows, with_pos=with_pos), ids, rows, table_rows, (dim, n, pattern, with_pos))


def test_ids_only_without_pos_and_no_ids_at_all(torch_cuda):
    torch = torch_cuda
    for n in (1, 64, D.MIN_CHUNK + 1):
        ids = D.draw_ids("zipf", n, 50)
        out = _run(torch, ids, None, 50, with_pos=False)
        assert set(out) == {"ids_out", "report", "workspace"}
        _check(out, ids, None, 50, ("ids only, no pos", n))
    # n == 0: the report is written, nothing else is touched; null ids are accepted
    empty = np.zeros(0, np.int64)
    out = _run(torch, empty, None, 5)
    assert _check(out, empty, None, 5, "n == 0") == {"n": 0, "distinct": 0, "duplicates": 0, "skipped": 0}
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    report = torch.full((4,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty((int(L.fcp_table_delta_workspace_bytes(0)) // 8,), dtype=torch.int64, device=dev)
    lib.check(L.fcp_table_delta_distinct(None, 4, None, 0, 0, 1, None, None, None, C.c_void_p(report.data_ptr()), C.c_void_p(ws.data_ptr()), 0,
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "fcp_table_delta_distinct")
    torch.cuda.synchronize()
    assert report.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("pattern", ("zipf", "global_congruent", "hot_head"))
def test_the_workspace_and_a_second_run_change_nothing(torch_cuda, pattern):
    """the same call with the workspace pre-filled with 0x00, with 0xFF, and once more: identical bytes in every output"""
    n, dim = 3 * D.MIN_CHUNK + 5, 6
    table_rows = D.global_rows(n)
    ids = D.draw_ids(pattern, n, table_rows)
    ids[::97] = -1
    rows = D.special_rows(n, dim, 2)
    runs = [_run(torch_cuda, ids, rows, table_rows, ws_fill=fill) for fill in (0x00, 0xFF, 0xFF)]
    _check(runs[0], ids, rows, table_rows, pattern)
    for other in runs[1:]:
        for name in ("ids_out", "pos_out", "rows_out", "report"):
            assert (runs[0][name] == other[name]).all(), (pattern, name)


@pytest.mark.parametrize("n", (1, D.TILE + 1, 2 * D.MIN_CHUNK + 1))
def test_an_already_distinct_delta_comes_out_as_it_went_in(torch_cuda, n):
    table_rows, dim = D.BIG_ROWS, 64
    ids = D.draw_ids("distinct", n, table_rows)
    rows = D.special_rows(n, dim, 3)
    out = _run(torch_cuda, ids, rows, table_rows)
    report = _check(out, ids, rows, table_rows, ("distinct", n))
    assert report == {"n": n, "distinct": n, "duplicates": 0, "skipped": 0}
    assert (_payload(out["ids_out"], np.int64) == ids).all() and (_payload(out["pos_out"], np.int64) == np.arange(n)).all()
    assert _payload(out["rows_out"]).tobytes() == rows.tobytes()


def test_the_wrappers(torch_cuda):
    """tables.delta_distinct slices at m and returns a DeltaReport; the async form returns the padded tensors; int32 ids"""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    n, table_rows, dim = 1500, 300, 6
    ids = D.draw_ids("zipf", n, table_rows)
    ids[::50] = table_rows + 3
    rows = D.special_rows(n, dim, 4)
    pos, report, ids_out, pos_out = D.distinct_ref(ids, table_rows)
    m = len(pos)
    for dtype in (np.int64, np.int32):
        d_ids, d_rows = torch.from_numpy(ids.astype(dtype)).to(dev), torch.from_numpy(rows).to(dev)
        got_ids, got_rows, got_report, got_pos = tables.delta_distinct(d_ids, d_rows, table_rows=table_rows, pos=True)
        assert got_report == tables.DeltaReport(**report)
        assert got_ids.cpu().numpy().tolist() == ids_out[:m].tolist() and got_pos.cpu().numpy().tolist() == pos.tolist()
        assert (got_rows.cpu().numpy().view(np.uint32) == rows.view(np.uint32)[pos]).all() and got_rows.shape == (m, dim)
        got_ids, got_rows, got_report = tables.delta_distinct(d_ids, table_rows=table_rows)
        assert got_rows is None and got_ids.cpu().numpy().tolist() == ids_out[:m].tolist() and got_report.distinct == m
        a_ids, a_rows, a_report = tables.delta_distinct_async(d_ids, d_rows, table_rows=table_rows)
        torch.cuda.synchronize()
        assert a_ids.shape == (n,) and a_rows.shape == (n, dim) and (a_ids.cpu().numpy() == ids_out).all()
        assert a_report.cpu().tolist() == [n, m, report["duplicates"], report["skipped"]]
    with pytest.raises(ValueError, match="rows has 3 rows, row_ids names 1500"):
        tables.delta_distinct(d_ids, d_rows[:3], table_rows=table_rows)
    with pytest.raises(ValueError, match="table_rows= is needed"):
        tables.delta_distinct(d_ids)


def _table_of(torch, master, kind, dev):
    """the device table of `kind` tables.convert writes from the float32 master (float32: the master itself)"""
    from recom_amd import tables
    t = torch.from_numpy(master).to(dev)
    return t if kind == "f32" else tables.convert(t, kind)


@pytest.mark.parametrize("kind", ("f32", "bf16", "f16", "q8"))
def test_apply_delta_end_to_end(torch_cuda, kind):
    """A delta with repeated ids (and ids outside the table) through tables.apply_delta: the table is, byte for byte, what
    tables.convert writes from the master that apply_ref updated one position after the other; the returned digest is
    tables.digest of the result; `skipped` receives the delta's own outside ids only.  (The same delta through plain
    update_rows_tracked is not asserted: its bytes are unspecified.)"""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    dim, table_rows, n = 20, 700, 2 * D.MIN_CHUNK + 9
    master = TC.family_rows(dim, table_rows, 5)
    rows = TC.family_rows(dim, n, 6)
    ids = D.draw_ids("zipf", n, table_rows, seed=1)
    ids[5::41] = D.outside_ids(table_rows)[np.arange(len(ids[5::41])) % 13]
    _pos, report, _i, _p = D.distinct_ref(ids, table_rows)
    assert report["duplicates"] > 100 and report["skipped"] > 10 and 100 < report["distinct"] < table_rows
    want = R.expect_bytes(D.apply_ref(master, ids, rows), kind)
    for dtype in (np.int64, np.int32):
        typed = ids if dtype == np.int64 else np.where((ids >= -2 ** 31) & (ids < 2 ** 31), ids, -5).astype(np.int32)
        table = _table_of(torch, master, kind, dev)
        assert (table.cpu().view(torch.uint8).numpy().reshape(table_rows, -1) == R.expect_bytes(master, kind)).all()
        before = tables.digest(table)
        skipped = torch.full((1,), 1000, dtype=torch.int64, device=dev)
        got_report, after = tables.apply_delta(table, torch.from_numpy(typed).to(dev), torch.from_numpy(rows).to(dev), digest=before, skipped=skipped)
        assert got_report == tables.DeltaReport(**report)
        got = table.cpu().view(torch.uint8).numpy().reshape(table_rows, -1)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (kind, bad[:5])
        assert after == tables.digest(table) and after != before
        assert int(skipped.cpu()[0]) == 1000 + report["skipped"]
        assert after == tables.digest_host(want, kind, dim=dim)
    # without a digest: the report alone
    table = _table_of(torch, master, kind, dev)
    assert tables.apply_delta(table, torch.from_numpy(ids).to(dev), torch.from_numpy(rows).to(dev)) == tables.DeltaReport(**report)
    assert (table.cpu().view(torch.uint8).numpy().reshape(table_rows, -1) == want).all()
