"""fcp_tables_delta_distinct on the GPU (recom_amd/csrc/fcp_tables_delta.hip): a model's delta made distinct in ONE call.  Two
oracles apply to every case: the single-table tables.delta_distinct_async of each entry, byte for byte (ids, pos, rows < m,
report), and distinct_ref of tests/table_delta_cases.py.  Entries with rows get a rows_out filled with a sentinel, and rows >= m
must still hold it; every call starts from a workspace filled with 0xFF.  The entry sets: tests/tables_delta_cases.py."""
import ctypes as C

import numpy as np
import pytest

import table_delta_cases as DC
import tables_delta_cases as GC

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


class Call:
    """One fcp_tables_delta_distinct call over `entries` (tests/tables_delta_cases.py): the device inputs, sentinel-filled
    outputs, and the C entry array."""

    def __init__(self, torch, entries):
        from recom_amd import lib
        self.torch, self.entries, self.L = torch, entries, lib.load()
        self.dev = torch.device("cuda", 0)
        self.ids = [torch.from_numpy(e["ids"]).to(self.dev) for e in entries]
        self.rows = [torch.from_numpy(e["rows"]).to(self.dev) if e["rows"] is not None else None for e in entries]
        ns = [len(e["ids"]) for e in entries]
        self.need = int(self.L.fcp_tables_delta_workspace_bytes((C.c_int64 * max(len(ns), 1))(*ns), len(ns)))
        assert self.need > 0 and self.need % 8 == 0
        self.fresh_outputs()

    def fresh_outputs(self):
        torch, dev = self.torch, self.dev
        fill = lambda n: torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)      # noqa: E731
        self.ids_out = [fill(8 * len(e["ids"])) for e in self.entries]
        self.pos_out = [fill(8 * len(e["ids"])) if e["pos"] else None for e in self.entries]
        self.rows_out = [fill(e["rows"].nbytes) if e["rows"] is not None else None for e in self.entries]
        self.reports = fill(32 * max(len(self.entries), 1))
        ptr = lambda t, n: t.data_ptr() if t is not None and n else None                # noqa: E731
        self.array = (lib_entry() * max(len(self.entries), 1))()
        for k, e in enumerate(self.entries):
            n = len(e["ids"])
            with_rows = e["rows"] is not None and n > 0
            self.array[k] = lib_entry()(ptr(self.ids[k], n), ptr(self.rows[k], with_rows), ptr(self.ids_out[k], n), ptr(self.rows_out[k], with_rows),
                                        ptr(self.pos_out[k], n), e["table_rows"], n, e["ids"].itemsize, e["rows"].shape[1] if e["rows"] is not None else 0)

    def workspace(self, fill=0xFF):
        return self.torch.full((self.need,), fill, dtype=self.torch.uint8, device=self.dev)

    def enqueue(self, workspace):
        from recom_amd import lib
        stream = self.torch.cuda.current_stream(self.dev).cuda_stream
        status = self.L.fcp_tables_delta_distinct(self.array, len(self.entries), C.c_void_p(self.reports.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                                  0, C.c_void_p(stream))
        lib.check(status, "fcp_tables_delta_distinct")

    def run(self, fill=0xFF):
        ws = self.workspace(fill)
        self.enqueue(ws)
        self.torch.cuda.synchronize()
        return self.outputs()

    def outputs(self):
        """the raw bytes of every output, per entry: (ids_out, pos_out or None, rows_out or None, report)"""
        reports = self.reports.cpu().numpy()
        host = lambda t: t.cpu().numpy() if t is not None else None                      # noqa: E731
        return [(host(self.ids_out[k]), host(self.pos_out[k]), host(self.rows_out[k]), reports[32 * k:32 * k + 32]) for k in range(len(self.entries))]

    def launches(self):
        return int(self.L.fcp_tables_delta_launches(self.array, len(self.entries)))

    def grid(self):
        blocks = (C.c_int32 * max(len(self.entries), 1))()
        return int(self.L.fcp_tables_delta_grid(self.array, len(self.entries), blocks)), list(blocks)[:len(self.entries)]


def lib_entry():
    from recom_amd import lib
    return lib.TableDeltaEntry


def check(call, outs, what):
    """every entry against the single-table call, byte for byte, and against distinct_ref; the sentinel behind the winners' rows"""
    from recom_amd import tables
    torch = call.torch
    for k, (e, (ids_raw, pos_raw, rows_raw, report_raw)) in enumerate(zip(call.entries, outs)):
        n = len(e["ids"])
        tag = (what, k, n, e["table_rows"])
        got_report = report_raw.view(np.int64).tolist()
        pos, report, ids_ref, pos_ref = DC.distinct_ref(e["ids"], e["table_rows"])
        m = len(pos)
        assert got_report == ([report["n"], report["distinct"], report["duplicates"], report["skipped"]] if n else [0, 0, 0, 0]), (tag, got_report, report)
        assert (ids_raw.view(np.int64) == ids_ref).all(), (tag, "ids_out against distinct_ref")
        if e["pos"]:
            assert (pos_raw.view(np.int64) == pos_ref).all(), (tag, "pos_out against distinct_ref")
        if e["rows"] is not None:
            dim = e["rows"].shape[1]
            got = rows_raw.view(np.uint32).reshape(n, dim)
            assert (got[:m] == e["rows"].view(np.uint32)[pos]).all(), (tag, "rows_out against distinct_ref")
            assert (rows_raw[4 * dim * m:] == SENTINEL).all(), (tag, "rows behind the winners were touched")
        if n == 0:
            continue
        single = tables.delta_distinct_async(call.ids[k], call.rows[k], table_rows=e["table_rows"], pos=e["pos"])
        torch.cuda.synchronize()
        assert single[2].cpu().tolist() == got_report, (tag, "report against the single-table call")
        assert (single[0].cpu().numpy() == ids_raw.view(np.int64)).all(), (tag, "ids_out against the single-table call")
        if e["pos"]:
            assert (single[3].cpu().numpy() == pos_raw.view(np.int64)).all(), (tag, "pos_out against the single-table call")
        if e["rows"] is not None:
            assert (single[1][:m].cpu().numpy().view(np.uint32) == got[:m]).all(), (tag, "rows_out against the single-table call")


def test_a_mixed_model_in_one_call(torch_cuda):
    """43 entries of every size class, pattern, dim, id width and mode in one call of at most 27 launches; the Python wrapper
    returns the same bytes."""
    from recom_amd import tables
    entries = GC.mixed_model()
    call = Call(torch_cuda, entries)
    assert call.launches() == GC.launches_of(entries) <= 27
    outs = call.run()
    check(call, outs, "mixed")
    got = tables.delta_distinct_grouped(call.ids, call.rows, [e["table_rows"] for e in entries], pos=True)
    for k, ((ids, rows, report, pos), (ids_raw, _pos_raw, rows_raw, report_raw)) in enumerate(zip(got, outs)):
        n, m = len(entries[k]["ids"]), report.distinct
        assert [report.n, report.distinct, report.duplicates, report.skipped] == report_raw.view(np.int64).tolist(), k
        assert (ids.cpu().numpy() == ids_raw.view(np.int64)[:m]).all() and len(ids) == m == len(pos), k
        assert (pos.cpu().numpy() == DC.distinct_ref(entries[k]["ids"], entries[k]["table_rows"])[0]).all(), k
        if entries[k]["rows"] is not None:
            assert (rows.cpu().numpy().view(np.uint32) == rows_raw.view(np.uint32).reshape(n, entries[k]["rows"].shape[1])[:m]).all(), k
        else:
            assert rows is None


@pytest.mark.parametrize("pattern", ["lds_congruent", "global_congruent"])
def test_two_entries_with_the_same_ids_do_not_see_each_other(torch_cuda, pattern):
    """The SAME id array for two tables of different sizes, with different rows: each entry's winners are its own.  A hash table
    or an LDS row table shared between entries would hand one entry the other's positions."""
    entries = GC.isolation(pattern)
    a, b = DC.distinct_ref(entries[0]["ids"], entries[0]["table_rows"]), DC.distinct_ref(entries[2]["ids"], entries[2]["table_rows"])
    assert a[1]["skipped"] == 0 and b[1]["skipped"] > 0 and a[1]["distinct"] != b[1]["distinct"]
    call = Call(torch_cuda, entries)
    check(call, call.run(), pattern)


def test_a_full_pass_and_one_among_two_hundred_single_ids(torch_cuda):
    """The big entry keeps the single-table grid — its chunk has grown past the smallest — the small ones one block each, and the
    launch has no idle block: the grid is exactly their sum."""
    entries = GC.block_edges()
    call = Call(torch_cuda, entries)
    grid, blocks = call.grid()
    n = DC.FULL_PASS + 1
    assert DC.chunk_for(n) > DC.MIN_CHUNK
    want = [(len(e["ids"]) + DC.chunk_for(len(e["ids"])) - 1) // DC.chunk_for(len(e["ids"])) for e in entries]
    assert blocks == want == [b for b, _chunk in GC.deal([len(e["ids"]) for e in entries])]
    assert blocks[77] == (n + DC.chunk_for(n) - 1) // DC.chunk_for(n) == 820 and grid == 820 + 200
    assert call.launches() == GC.FIXED_LAUNCHES + 2                       # ids only, and dim 4
    check(call, call.run(), "block edges")


def test_a_call_whose_lone_grids_sum_past_the_cap(torch_cuda):
    entries = GC.scaled_deal()
    ns = [len(e["ids"]) for e in entries]
    assert sum(GC.lone_blocks(n) for n in ns) > GC.DEAL_BLOCKS == int(Call(torch_cuda, entries[:1]).L.fcp_tables_delta_deal_blocks())
    call = Call(torch_cuda, entries)
    grid, blocks = call.grid()
    assert blocks == [b for b, _chunk in GC.deal(ns)] and grid == sum(blocks) <= GC.DEAL_BLOCKS + len(ns)
    assert all(b < GC.lone_blocks(n) for b, n in zip(blocks, ns))
    check(call, call.run(), "scaled deal")


@pytest.mark.parametrize("count", [1025, 4097])
def test_many_small_entries(torch_cuda, count):
    entries = GC.many_small(count)
    call = Call(torch_cuda, entries)
    assert call.launches() == GC.launches_of(entries) == GC.FIXED_LAUNCHES + 3
    check(call, call.run(), f"{count} entries")


def test_two_calls_leave_the_same_bytes(torch_cuda):
    """Whatever the workspace held, and with one workspace shared by two calls on one stream."""
    entries = GC.mixed_model()[:20] + GC.isolation("lds_congruent")
    call = Call(torch_cuda, entries)
    first = call.run(fill=0xFF)
    check(call, first, "first")
    call.fresh_outputs()
    second = call.run(fill=0x00)
    other = Call(torch_cuda, list(reversed(entries)))
    shared = call.torch.full((max(call.need, other.need),), 0x3C, dtype=call.torch.uint8, device=call.dev)
    call.fresh_outputs()
    call.enqueue(shared)
    other.enqueue(shared)
    call.enqueue(shared)
    call.torch.cuda.synchronize()
    third, reversed_outs = call.outputs(), other.outputs()
    for k, (a, b, c, d) in enumerate(zip(first, second, third, reversed(reversed_outs))):
        for x, y, z, w in zip(a, b, c, d):
            assert (x is None and y is None and z is None and w is None) or ((x == y).all() and (x == z).all() and (x == w).all()), k


def test_apply_delta_grouped_is_apply_delta_per_table(torch_cuda):
    """A served model of f32, bf16, fp16 and q8 tables with dims 1, 6, 16 and 64 and a delta whose ids repeat: every table is, byte
    for byte, what per-table apply_delta leaves on a copy; the returned digests are tables.digest of the finished tables;
    `skipped` grows by the reports' skipped only."""
    from recom_amd import tables
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    model = GC.chain_model()
    rng = np.random.default_rng(5)
    served, copies, ids, rows = [], [], [], []
    for kind, table_rows, dim, ids_np, rows_np in model:
        master = torch.from_numpy(rng.standard_normal((table_rows, dim)).astype(np.float32)).to(dev)
        t = master if kind == "f32" else tables.convert(master, kind)
        served.append(t)
        copies.append(t.clone())
        ids.append(torch.from_numpy(ids_np).to(dev))
        rows.append(torch.from_numpy(rows_np).to(dev))
    before = tables.digests_grouped(served)
    skipped = torch.arange(1000, 1000 + len(model), dtype=torch.int64, device=dev)
    reports, after = tables.apply_delta_grouped(served, ids, rows, digests=before, skipped=skipped)
    assert len(reports) == len(after) == len(model)
    for k, (kind, table_rows, dim, ids_np, rows_np) in enumerate(model):
        want = tables.apply_delta(copies[k], ids[k], rows[k])
        _pos, ref, _i, _p = DC.distinct_ref(ids_np, table_rows)
        assert reports[k] == want == tables.DeltaReport(**ref), (k, kind, dim)
        assert torch.equal(served[k].view(torch.uint8), copies[k].view(torch.uint8)), (k, kind, dim)
        assert after[k] == tables.digest(served[k]), (k, kind, dim)
    assert sum(r.duplicates for r in reports) > 100 and sum(r.skipped for r in reports) > 20
    assert skipped.cpu().tolist() == [1000 + k + r.skipped for k, r in enumerate(reports)]
    # without digests: the reports alone, and the same tables once more (the delta is idempotent)
    again = tables.apply_delta_grouped(served, ids, rows)
    assert again == reports
    for k in range(len(model)):
        assert torch.equal(served[k].view(torch.uint8), copies[k].view(torch.uint8)), k
