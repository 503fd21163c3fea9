"""fcp_tables_update_rows / fcp_tables_read_rows on the GPU (kernels: recom_amd/csrc/fcp_tables_rows.hip): a whole model's delta
in one call.  Every case runs into poisoned tables with rows behind them and is compared as bytes, with no tolerance, against
the CPU expectation (table_rows_cases.expect_bytes: the restatements) AND against twin tables updated through one
tables.update_rows per entry; the runners and the entry lists are tests/tables_rows_cases.py.  The calls on a non-default stream,
behind delta_distinct, and under stream capture: tests/test_zzz_gpu_tables_rows_stream.py.

The file sorts behind tests/test_z_gpu_private_streams.py for the reason tests/test_zzz_gpu_outputs_compare.py gives.  It takes no
stream from torch's pool, yet as tests/test_gpu_tables_rows.py, in front of that file, the whole suite failed in that file's
test_supervisor_re_admits_a_demoted_caller_when_the_private_streams_win_again (the caller stayed demoted) — the very test and the
very symptom recorded there for the other entry that installs its records from a pinned ring.  Behind the private-stream tests it
disturbs nothing."""
import ctypes as C

import numpy as np
import pytest

import table_rows_cases as R
import tables_rows_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _launches(entries) -> int:
    """fcp_tables_rows_launches of an entry list (host only: the pointers are numbers)"""
    from recom_amd import lib
    arr = (lib.TableRows * max(len(entries), 1))(*[lib.TableRows(1 << 20, 1 << 20, 1 << 20, tr, len(ids), lib.TABLE_KINDS[kind], dim)
                                                  for kind, dim, tr, ids, _x in entries])
    return int(lib.load().fcp_tables_rows_launches(arr, len(entries)))


def test_mixed_model(torch_cuda):
    """40 entries over all four kinds, nine dims and six row counts, empty entries first, last and two in a row in the middle:
    one call, at most 25 launches."""
    entries = G.mixed_model()
    assert 2 <= _launches(entries) <= 25
    G.run_update(torch_cuda, entries, torch_cuda.device("cuda", 0), what="mixed model")


def test_block_edges(torch_cuda):
    """Entries of exactly one block, one block -/+ one row and two blocks, side by side in their class, in both fronts: a first
    block off by one writes a neighbour's rows or leaves rows unwritten, and either shows in the bytes."""
    G.run_update(torch_cuda, G.block_edges(), torch_cuda.device("cuda", 0), what="block edges")


def test_search_depth(torch_cuda):
    """1500 entries of 1 to 3 rows in two classes: 750 one-block pieces per launch, so every block's search runs its ten steps and
    ends at a prefix end; three launches whatever the count."""
    entries = G.search_depth()
    assert _launches(entries) == 3 == _launches(entries[:2])
    G.run_update(torch_cuda, entries, torch_cuda.device("cuda", 0), what="search depth")


def test_skew(torch_cuda):
    """One entry of 5000 rows beside entries of one row."""
    G.run_update(torch_cuda, G.skew(), torch_cuda.device("cuda", 0), what="skew")


def test_outside_ids(torch_cuda):
    """-1, INT64_MIN, table_rows and 2^40 per entry: their rows land nowhere (table_rows lies inside the allocation: a missing
    range check would overwrite poison), skipped[k] grows by exactly entry k's count and stays as it was for entries with none;
    a null `skipped` is accepted."""
    dev = torch_cuda.device("cuda", 0)
    entries = G.outside_ids()
    counts = [int((~G.inside(e)).sum()) for e in entries]
    assert set(counts) == {0, 1, 4, 9}
    G.run_update(torch_cuda, entries, dev, what="outside ids")
    G.run_update(torch_cuda, entries, dev, with_skipped=False, what="outside ids, skipped=None")


@pytest.mark.parametrize("kind,dim", (("q8", 64), ("bf16", 6)))
def test_one_table_in_two_entries(torch_cuda, kind, dim):
    """Two entries name one table with ids that are pairwise distinct together — with another table's entry between them: the
    table holds both deltas, as after two update_rows calls."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    n, table_rows = 300, 300 + R.SLACK_ROWS
    ids = R.distinct_ids(n, table_rows, 71)
    x = G.rows_of(dim, n)
    halves = (slice(0, 129), slice(129, n))
    buf, table = R.poisoned(torch, kind, dim, table_rows, dev)
    twin_buf, twin = R.poisoned(torch, kind, dim, table_rows, dev)
    other = G.entry(kind, dim, 65, 72)
    obuf, otable = R.poisoned(torch, other[0], other[1], other[2], dev)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    skipped = torch.zeros(3, dtype=torch.int64, device=dev)
    tables.update_rows_grouped([table, otable, table], [d(ids[halves[0]]), d(other[3]), d(ids[halves[1]])],
                               [d(x[halves[0]]), d(other[4]), d(x[halves[1]])], skipped=skipped)
    for h in halves:
        tables.update_rows(twin, d(ids[h]), d(x[h]))
    torch.cuda.synchronize()
    R.check_poisoned(buf, kind, dim, table_rows, ids, R.expect_bytes(x, kind), (kind, dim, "one table, two entries"))
    R.check_poisoned(obuf, other[0], other[1], other[2], other[3], R.expect_bytes(other[4], kind), (kind, dim, "the table between"))
    assert torch.equal(buf, twin_buf) and int(skipped.abs().sum().item()) == 0


def test_grouped_read(torch_cuda):
    """read_rows_grouped equals tables.read_rows per table bit for bit, over the mixed model (every kind, dim and row count, empty
    entries included), the block edges and entries with ids outside the table, whose rows are +0.0; the element behind every
    output keeps its sentinel."""
    dev = torch_cuda.device("cuda", 0)
    G.run_read(torch_cuda, G.mixed_model(), dev, what="read: mixed model")
    G.run_read(torch_cuda, G.block_edges() + G.outside_ids(), dev, what="read: block edges and outside ids")
    few = G.search_depth(600)
    G.run_read(torch_cuda, few, dev, what="read: 600 small entries")


def test_served_model(torch_cuda):
    """The two-column model (a gather, a mean-pooled column) on q8 tables: ONE grouped call applies both tables' deltas, the tables
    are the restatement's bytes, and a request enqueued behind it on the same stream, with nothing in between, reads the new
    rows: bit for bit the float32 plan on the dequantised updated tables."""
    torch = torch_cuda
    from recom_amd import tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    spec, masters, deltas, (inputs, symbols) = R.small_model()
    want_q8, want_deq = R.small_model_expected_tables(masters, deltas)
    op, op32 = FeatureColumnProcess(spec.with_table_dtype("q8"), 0), FeatureColumnProcess(spec, 0)
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    q8 = [tables.convert(torch.from_numpy(m).to(dev), "q8") for m in masters]
    d_ids = [torch.from_numpy(i).to(dev) for i, _r in deltas]
    d_rows = [torch.from_numpy(r).to(dev) for _i, r in deltas]
    ref = op32(d_blob, offsets, shapes, [torch.from_numpy(w).to(dev) for w in want_deq], symbols)
    torch.cuda.synchronize()
    tables.update_rows_grouped(q8, d_ids, d_rows)
    out = op(d_blob, offsets, shapes, q8, symbols)
    torch.cuda.synchronize()
    for t, w in zip(q8, want_q8):
        assert (t.cpu().numpy() == w).all()
    got, want = out.groups[0].cpu().numpy(), ref.groups[0].cpu().numpy()
    assert got.shape == (int(symbols[0]), 12) and not np.isnan(want).any() and np.abs(want).max() > 0
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_workspace_is_the_callers_and_may_be_shared_on_one_stream(torch_cuda):
    """The C entry with a workspace of exactly fcp_tables_rows_workspace_bytes bytes between two guard words, at an address that is
    8 but not 16 bytes aligned, used by two calls in a row on one stream: both deltas land, the guards stay."""
    torch = torch_cuda
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    entries = G.mixed_model()[:12]
    need = int(L.fcp_tables_rows_workspace_bytes(len(entries)))
    arena = torch.full((need // 8 + 3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    ws = arena.data_ptr() + 8
    assert ws % 16 == 8
    stream = torch.cuda.current_stream(dev).cuda_stream
    bufs = []
    for rep in range(2):
        tabs, ids, xs = [], [], []
        for kind, dim, table_rows, i, x in entries:
            b, t = R.poisoned(torch, kind, dim, table_rows, dev)
            bufs.append(b), tabs.append(t), ids.append(torch.from_numpy(i).to(dev)), xs.append(torch.from_numpy(np.ascontiguousarray(x)).to(dev))
        arr = (lib.TableRows * len(entries))(*[lib.TableRows(t.data_ptr(), i.data_ptr(), x.data_ptr(), e[2], len(e[3]), lib.TABLE_KINDS[e[0]], e[1])
                                              for t, i, x, e in zip(tabs, ids, xs, entries)])
        lib.check(L.fcp_tables_update_rows(arr, len(entries), None, C.c_void_p(ws), 0, C.c_void_p(stream)), "fcp_tables_update_rows")
        del arr                                                        # `entries` is read before the call returns
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        kind, dim, table_rows, i, x = entries[k % len(entries)]
        want = R.expect_bytes(x, kind) if len(i) else np.zeros((0, R.row_bytes(kind, dim)), np.uint8)
        R.check_poisoned(b, kind, dim, table_rows, i, want, ("shared workspace", k))
    a = arena.cpu().numpy()
    assert a[0] == 0x5A5A5A5A5A5A5A5A and (a[1 + need // 8:] == 0x5A5A5A5A5A5A5A5A).all(), "the call wrote outside its workspace"
