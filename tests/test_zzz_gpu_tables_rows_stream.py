"""fcp_tables_update_rows / fcp_tables_read_rows on a non-default stream, chained behind delta_distinct's padding, and under
stream capture (kernels: recom_amd/csrc/fcp_tables_rows.hip).

A file of its own that sorts behind tests/test_z_gpu_private_streams.py, for the reason
tests/test_zzz_gpu_table_convert_stream.py gives: a stream taken from torch's pool shifts which hardware queue later streams
are mapped to, the one thing the private-stream tests depend on and cannot see.  Behind them it disturbs nothing."""
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


def test_grouped_calls_on_a_non_default_stream(torch_cuda):
    """The mixed model, the outside ids and the grouped read with every call enqueued on a stream of its own and nothing but
    that stream synchronised: stream order is all there is."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    G.run_update(torch, G.mixed_model() + G.outside_ids(), dev, stream=stream, what="stream: mixed model and outside ids")
    G.run_read(torch, G.mixed_model() + G.outside_ids(), dev, stream=stream, what="stream: read")


def test_served_model_in_stream_order(torch_cuda):
    """On a non-default stream with no synchronisation in between: the grouped update of both q8 tables, the grouped read of
    the updated rows, the plan of the small model.  The results are those of the synchronised run."""
    torch = torch_cuda
    from recom_amd import synth, tables
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
    want = ref.groups[0].cpu().numpy()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        tables.update_rows_grouped(q8, d_ids, d_rows, stream=stream.cuda_stream)
        back = tables.read_rows_grouped(q8, d_ids)                      # the wrapper's default: torch's current stream
        out = op(d_blob, offsets, shapes, q8, symbols, stream=stream.cuda_stream)
    stream.synchronize()
    for t, w, b, (ids, _rows) in zip(q8, want_q8, back, deltas):
        assert (t.cpu().numpy() == w).all()
        assert (b.cpu().numpy().view(np.uint32) == synth.dequantize_q8(w[ids]).view(np.uint32)).all()
    got = out.groups[0].cpu().numpy()
    assert np.abs(want).max() > 0 and (got.view(np.uint32) == want.view(np.uint32)).all()


def test_grouped_update_behind_delta_distinct_padding(torch_cuda):
    """Deltas that repeat ids, made distinct on the device by tables.delta_distinct_async, whose padded outputs — winners in front,
    -1 behind them — go straight into ONE grouped update on the same stream with no host read: the -1 ids are skipped, and every
    table is what the rows written one after the other in position order leave."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(5)
    cases = []
    for k, (kind, dim) in enumerate((("q8", 64), ("bf16", 6), ("f32", 3), ("q8", 5), ("f16", 64))):
        table_rows, n = 90 + 7 * k, 200 + k
        ids = rng.integers(0, table_rows, n).astype(np.int64)          # repeats for certain: n > table_rows
        ids[3], ids[n - 2] = -1, table_rows + 1                         # the delta's own outside ids
        cases.append((kind, dim, table_rows, ids, G.rows_of(dim, n)))
    bufs, tabs, pads, reports = [], [], [], []
    with torch.cuda.stream(stream):
        for kind, dim, table_rows, ids, x in cases:
            b, t = R.poisoned(torch, kind, dim, table_rows, dev)
            bufs.append(b), tabs.append(t)
            ids_d, rows_d, report = tables.delta_distinct_async(torch.from_numpy(ids).to(dev), torch.from_numpy(x).to(dev),
                                                                table_rows=table_rows, stream=stream.cuda_stream)
            pads.append((ids_d, rows_d)), reports.append(report)
        skipped = torch.zeros(len(cases), dtype=torch.int64, device=dev)
        tables.update_rows_grouped(tabs, [p[0] for p in pads], [p[1] for p in pads], skipped=skipped, stream=stream.cuda_stream)
    stream.synchronize()
    for k, (kind, dim, table_rows, ids, x) in enumerate(cases):
        last = {}
        for pos, i in enumerate(ids.tolist()):
            if 0 <= i < table_rows:
                last[i] = pos
        win_ids = np.asarray(sorted(last), np.int64)
        win_rows = x[[last[i] for i in win_ids.tolist()]]
        R.check_poisoned(bufs[k], kind, dim, table_rows, win_ids, R.expect_bytes(win_rows, kind), ("behind delta_distinct", k, kind, dim))
        n, distinct, duplicates, outside = (int(v) for v in reports[k].cpu().tolist())
        assert (n, distinct, outside) == (len(ids), len(last), 2) and duplicates > 0
        assert int(skipped[k].item()) == n - distinct                  # the padding: every -1 behind the winners is skipped


def test_capturing_stream(torch_cuda):
    """A capturing stream with work to do is FCP_ERR_UNSUPPORTED — the records are installed from the host by every call, which a
    replay would not repeat — and nothing is recorded; a call with no work (n_tables == 0, or every n == 0) is FCP_OK inside
    the capture.  The capture goes on and replays."""
    torch = torch_cuda
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    kind, dim, table_rows, ids, x = G.entry("q8", 64, 65, 9)
    buf, table = R.poisoned(torch, kind, dim, table_rows, dev)
    d_ids, d_x = torch.from_numpy(ids).to(dev), torch.from_numpy(x).to(dev)
    out = torch.empty((65, dim), dtype=torch.float32, device=dev)
    ws = torch.empty((int(L.fcp_tables_rows_workspace_bytes(1)) // 8,), dtype=torch.int64, device=dev)
    counter = torch.zeros(8, dtype=torch.int64, device=dev)
    work = (lib.TableRows * 1)(lib.TableRows(table.data_ptr(), d_ids.data_ptr(), d_x.data_ptr(), table_rows, 65, lib.TABLE_KINDS[kind], dim))
    read = (lib.TableRows * 1)(lib.TableRows(table.data_ptr(), d_ids.data_ptr(), out.data_ptr(), table_rows, 65, lib.TABLE_KINDS[kind], dim))
    idle = (lib.TableRows * 1)(lib.TableRows(table.data_ptr(), d_ids.data_ptr(), d_x.data_ptr(), table_rows, 0, lib.TABLE_KINDS[kind], dim))
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    statuses = []
    with torch.cuda.graph(g, stream=s):
        p = C.c_void_p(s.cuda_stream)
        statuses.append(L.fcp_tables_update_rows(work, 1, None, C.c_void_p(ws.data_ptr()), 0, p))
        message = L.fcp_last_error().decode()
        statuses.append(L.fcp_tables_read_rows(read, 1, C.c_void_p(ws.data_ptr()), 0, p))
        statuses.append(L.fcp_tables_update_rows(None, 0, None, None, 0, p))
        statuses.append(L.fcp_tables_update_rows(idle, 1, None, C.c_void_p(ws.data_ptr()), 0, p))
        statuses.append(L.fcp_tables_read_rows(idle, 1, C.c_void_p(ws.data_ptr()), 0, p))
        counter.add_(1)                                                 # (something for the graph to hold)
    assert statuses == [lib.FCP_ERR_UNSUPPORTED, lib.FCP_ERR_UNSUPPORTED, lib.FCP_OK, lib.FCP_OK, lib.FCP_OK], statuses
    assert message.startswith("fcp_tables_update_rows: ") and "capture" in message
    g.replay()
    torch.cuda.synchronize()
    assert bool((buf == R.POISON).all()) and int(counter[0].item()) == 1
    # the same call outside the capture does the work
    lib.check(L.fcp_tables_update_rows(work, 1, None, C.c_void_p(ws.data_ptr()), 0, C.c_void_p(s.cuda_stream)), "fcp_tables_update_rows")
    s.synchronize()
    R.check_poisoned(buf, kind, dim, table_rows, ids, R.expect_bytes(x, kind), "after the capture")
