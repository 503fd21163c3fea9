"""fcp_tables_digest on a non-default stream, chained around a grouped update with one host read at the end, and under stream
capture (kernels: recom_amd/csrc/fcp_tables_digest.hip).

A file of its own that sorts behind tests/test_z_gpu_private_streams.py, for the reason
tests/test_zzz_gpu_table_convert_stream.py gives: a stream taken from torch's pool shifts which hardware queue later streams
are mapped to, the one thing the private-stream tests depend on and cannot see.  Behind them it disturbs nothing."""
import ctypes as C

import numpy as np
import pytest

import table_digest_cases as TD
import tables_digest_cases as GD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def test_on_a_side_stream_behind_fills(torch_cuda):
    """The call is ordered on the stream it is given: tables filled on a side stream, digested on that stream in one call, in
    both modes; the mixed model on a stream of its own with nothing but that stream synchronised."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    shapes = (((1 << 16, 64), torch.float32, "f32", 1.5), ((1 << 15, 16), torch.bfloat16, "bf16", -2.0), ((3000, 7), torch.float16, "f16", 0.25))
    tabs = [torch.zeros(shape, dtype=dtype, device=dev) for shape, dtype, _k, _v in shapes]
    ids = [torch.arange(0, t.shape[0], 2, dtype=torch.int64, device=dev) for t in tabs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    assert side.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    with torch.cuda.stream(side):
        for t, (_s, _d, _k, value) in zip(tabs, shapes):
            t.fill_(value)
        got = tables.digests_grouped(tabs, stream=side.cuda_stream)
        got_rows = tables.digest_rows_grouped(tabs, ids)                 # the wrapper's default: torch's current stream
    for k, (shape, dtype, kind, value) in enumerate(shapes):
        want = torch.full(shape, value, dtype=dtype).view(torch.uint8).numpy() if dtype != torch.float32 else np.full(shape, value, np.float32)
        assert got[k] == TD.digest(want.tobytes(), kind, shape[1]), kind
        assert got_rows[k] == (TD.digest(np.ascontiguousarray(want[::2]).tobytes(), kind, shape[1], 0, 2), (shape[0] + 1) // 2, 0), kind
    torch.cuda.synchronize()
    GD.run(torch, GD.mixed_model(), dev, stream=torch.cuda.Stream(device=dev), what="stream: mixed model")


def test_digest_update_digest_chained_with_one_host_read(torch_cuda):
    """Through the C ABI on one side stream with no synchronisation in between: a grouped digest of the rows a delta names, the
    grouped update, the grouped digest again, the whole tables' digests — then ONE synchronise and one copy back.  before / after
    are those of the tables before / after, and digest - before + after is the digest of the updated table."""
    torch = torch_cuda
    from recom_amd import lib, tables
    L = lib.load()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    cases = (("q8", 64, 900, 300), ("bf16", 6, 97, 97), ("f32", 3, 5000, 1), ("f16", 64, 300, 150), ("q8", 5, 64, 10))
    tabs, ids, deltas = [], [], []
    for k, (kind, dim, table_rows, n) in enumerate(cases):
        master = torch.randn((table_rows, dim), generator=gen).to(dev)
        tabs.append(master if kind == "f32" else tables.convert(master, kind))
        own = np.random.default_rng(60 + k).permutation(table_rows)[:n].astype(np.int64)
        ids.append(torch.from_numpy(np.concatenate([own, [-1, table_rows + 2]])).to(dev))
        deltas.append(torch.randn((n + 2, dim), generator=gen).to(dev))
    torch.cuda.synchronize()
    old = [TD.bytes_of(torch, t).tobytes() for t in tabs]
    n_tables = len(cases)
    by_id = (lib.TableDigestEntry * n_tables)(*[lib.TableDigestEntry(t.data_ptr(), i.data_ptr(), int(t.shape[0]), int(i.shape[0]), 3, 2, TD.KIND[c[0]], c[1], 0)
                                               for t, i, c in zip(tabs, ids, cases)])
    whole = (lib.TableDigestEntry * n_tables)(*[lib.TableDigestEntry(t.data_ptr(), None, int(t.shape[0]), 0, 3, 2, TD.KIND[c[0]], c[1], 0)
                                              for t, c in zip(tabs, cases)])
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        outs = torch.zeros((4, n_tables, 4), dtype=torch.int64, device=dev)
        ws = torch.empty((int(L.fcp_tables_digest_workspace_bytes(n_tables)) // 8,), dtype=torch.int64, device=dev)
        p, s = C.c_void_p(ws.data_ptr()), C.c_void_p(side.cuda_stream)
        lib.check(L.fcp_tables_digest(whole, n_tables, C.c_void_p(outs[0].data_ptr()), p, 0, s), "fcp_tables_digest")
        lib.check(L.fcp_tables_digest(by_id, n_tables, C.c_void_p(outs[1].data_ptr()), p, 0, s), "fcp_tables_digest")
        tables.update_rows_grouped(tabs, ids, deltas, stream=side.cuda_stream)
        lib.check(L.fcp_tables_digest(by_id, n_tables, C.c_void_p(outs[2].data_ptr()), p, 0, s), "fcp_tables_digest")
        lib.check(L.fcp_tables_digest(whole, n_tables, C.c_void_p(outs[3].data_ptr()), p, 0, s), "fcp_tables_digest")
    side.synchronize()
    host = outs.cpu().numpy()                                              # the one host read
    new = [TD.bytes_of(torch, t).tobytes() for t in tabs]
    for k, (kind, dim, table_rows, n) in enumerate(cases):
        i = ids[k].cpu().numpy()
        rec = [(int(host[j, k, 0]) & TD.M64, int(host[j, k, 1]), int(host[j, k, 2])) for j in range(4)]
        assert rec[0] == (TD.digest(old[k], kind, dim, 3, 2), table_rows, 0), k
        assert rec[1] == TD.digest_ids(old[k], kind, dim, i, 3, 2) and rec[1][1:] == (n, 2), k
        assert rec[2] == TD.digest_ids(new[k], kind, dim, i, 3, 2), k
        assert rec[3] == (TD.digest(new[k], kind, dim, 3, 2), table_rows, 0) and old[k] != new[k], k
        assert (rec[0][0] - rec[1][0] + rec[2][0]) & TD.M64 == rec[3][0], k


def test_capturing_stream(torch_cuda):
    """A capturing stream with entries is FCP_ERR_UNSUPPORTED — the records are installed from the host by every call, which a
    replay would not repeat — and nothing is recorded; n_tables == 0 is FCP_OK inside the capture.  The capture goes on and
    replays."""
    torch = torch_cuda
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    raw = TD.draw_raw("q8", 64, 65, 9)
    table = TD.as_table(torch, raw, "q8", 64, dev)
    out = torch.full((4,), GD.GUARD, dtype=torch.int64, device=dev)
    ws = torch.empty((int(L.fcp_tables_digest_workspace_bytes(1)) // 8,), dtype=torch.int64, device=dev)
    counter = torch.zeros(8, dtype=torch.int64, device=dev)
    work = (lib.TableDigestEntry * 1)(lib.TableDigestEntry(table.data_ptr(), None, 65, 0, 0, 1, TD.KIND["q8"], 64, 0))
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    statuses = []
    with torch.cuda.graph(g, stream=s):
        p = C.c_void_p(s.cuda_stream)
        statuses.append(L.fcp_tables_digest(work, 1, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 0, p))
        message = L.fcp_last_error().decode()
        statuses.append(L.fcp_tables_digest(None, 0, None, None, 0, p))
        statuses.append(L.fcp_tables_digest(work, 0, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 0, p))
        counter.add_(1)                                                 # (something for the graph to hold)
    assert statuses == [lib.FCP_ERR_UNSUPPORTED, lib.FCP_OK, lib.FCP_OK], statuses
    assert message.startswith("fcp_tables_digest: ") and "capture" in message
    g.replay()
    torch.cuda.synchronize()
    assert bool((out == GD.GUARD).all()) and int(counter[0].item()) == 1
    # the same call outside the capture does the work
    lib.check(L.fcp_tables_digest(work, 1, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 0, C.c_void_p(s.cuda_stream)), "fcp_tables_digest")
    s.synchronize()
    host = out.cpu().numpy()
    assert (int(host[0]) & TD.M64, int(host[1]), int(host[2]), int(host[3])) == (TD.digest(raw.tobytes(), "q8", 64), 65, 0, 0)
