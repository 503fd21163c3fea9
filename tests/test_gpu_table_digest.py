"""fcp_table_digest / fcp_table_digest_rows on the GPU (recom_amd/csrc/fcp_table_digest.hip): every comparison is == against the
NumPy reference (table_digest_cases.digest) of the table's bytes copied back.  Every kind at every dim and row count, one full
pass of the fixed grid plus one row, unaligned starts, chunk and shard sums, rows by id with ids outside the table and repeated
ids, a digest kept across fcp_table_update_rows against fcp_table_convert of the patched master, determinism, guard words, a
side stream."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import table_digest_cases as TD
import table_mixed_cases as TM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _dims(kind):
    return tuple(d for d in TD.DIMS if d != 129 or kind == "f32")


@pytest.mark.parametrize("kind", TD.KINDS)
def test_digest_of_every_dim_and_row_count(torch_cuda, kind):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    for dim in _dims(kind):
        for rows in (0, 1, 2, 1000):
            raw = TD.draw_raw(kind, dim, rows, 21)
            t = TD.as_table(torch, raw, kind, dim, dev)
            got = tables.digest(t)
            back = TD.bytes_of(torch, t)
            assert np.array_equal(back, raw.reshape(-1)), (kind, dim, rows, "the table's own bytes changed")
            want = TD.digest(back.tobytes(), kind, dim)
            print(kind, dim, rows, hex(got), hex(want))
            assert got == want, (kind, dim, rows, hex(got), hex(want))
            if rows == 1000:
                assert tables.digest(t, row0=5, row_step=3) == TD.digest(back.tobytes(), kind, dim, 5, 3), (kind, dim, "row0 5, row_step 3")


def test_known_answers_on_the_device(torch_cuda):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    for raw, kind, dim, want in TD.KNOWN:
        rb = TD.row_bytes(kind, dim)
        t = TD.as_table(torch, np.frombuffer(raw, np.uint8).reshape(-1, rb), kind, dim, dev)
        assert tables.digest(t) == want, (kind, dim)


@pytest.mark.parametrize("kind,dim", [(k, d) for d in (1, 64) for k in TD.KINDS], ids=lambda v: str(v))
def test_one_full_pass_of_the_grid_plus_one_row(torch_cuda, kind, dim):
    """The grid's stride plus one row (the second row of a block's unrolled step) and the whole unrolled step plus one row (the
    second trip of the walk)."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    rows = TD.full_pass_rows(kind, dim, TD.UNROLL) + 1
    raw = TD.draw_raw(kind, dim, rows, 22)
    t = TD.as_table(torch, raw, kind, dim, dev)
    back = TD.bytes_of(torch, t).reshape(rows, -1)
    for n in (TD.full_pass_rows(kind, dim) + 1, rows):
        got = tables.digest(t[:n])
        want = TD.digest(back[:n].tobytes(), kind, dim)
        print(kind, dim, n, hex(got), hex(want))
        assert got == want, (kind, dim, n)


@pytest.mark.parametrize("kind,dim", [("q8", 1), ("bf16", 1)])
def test_unaligned_starts_and_chunk_sums(torch_cuda, kind, dim):
    """Views table[a:] with row0 = a for a = 1 .. 8: q8 rows of 9 bytes start at every alignment modulo 8, bf16 rows of dim 1 at
    every even one.  No byte in front of the view is read as part of it: the view's digest is the reference's of its own bytes.
    The chunks [0, a) and [a, rows) add up to the whole."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    rows = 777
    raw = TD.draw_raw(kind, dim, rows, 23)
    t = TD.as_table(torch, raw, kind, dim, dev)
    whole = tables.digest(t)
    assert whole == TD.digest(raw.tobytes(), kind, dim)
    starts = set()
    for a in range(1, 9):
        view = t[a:]
        starts.add(view.data_ptr() % 8)
        got = tables.digest(view, row0=a)
        assert got == TD.digest(raw[a:].tobytes(), kind, dim, a), (kind, a)
        assert (tables.digest(t[:a]) + got) & TD.M64 == whole, (kind, a)
        last = tables.digest(t[a:a + 1], row0=a)                # one row: its tail is the last thing in the range
        assert last == TD.digest(raw[a:a + 1].tobytes(), kind, dim, a), (kind, a)
    assert starts == (set(range(8)) if kind == "q8" else {0, 2, 4, 6})
    for chunk in (1, 7, 100):
        if chunk == 1:
            parts = [tables.digest(t[a:a + 1], row0=a) for a in range(0, 40)] + [tables.digest(t[40:], row0=40)]
        else:
            parts = [tables.digest(t[a:a + chunk], row0=a) for a in range(0, rows, chunk)]
        assert sum(parts) & TD.M64 == whole, (kind, chunk)


def test_the_last_row_ends_where_the_allocation_ends(torch_cuda):
    """A q8 table of 9-byte rows at the very end of a buffer that is followed by a poisoned guard: the guard's bytes play no part
    (the reference sees the table's bytes alone) at any start alignment."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    for front in range(8):
        raw = TD.draw_raw("q8", 7, 3, 24 + front)                  # rows of 15 bytes: a tail of 7
        buf = torch.full((front + raw.size + 64,), 0xA5, dtype=torch.uint8, device=dev)
        buf[front:front + raw.size].copy_(torch.from_numpy(raw.reshape(-1)))
        t = buf[front:front + raw.size].view(3, 15)
        assert tables.digest(t) == TD.digest(raw.tobytes(), "q8", 7), front
        assert bool((buf[front + raw.size:] == 0xA5).all()) and bool((buf[:front] == 0xA5).all())


@pytest.mark.parametrize("kind", TD.KINDS)
def test_digest_rows(torch_cuda, kind):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    for dim in (1, 2, 5, 64, 300):
        table_rows = 211
        raw = TD.draw_raw(kind, dim, table_rows, 25)
        t = TD.as_table(torch, raw, kind, dim, dev)
        back = TD.bytes_of(torch, t).tobytes()
        whole = TD.digest(back, kind, dim)
        for what, ids, row0, step in (("none", [], 0, 1), ("one", [table_rows - 1], 0, 1), ("ends", [0, table_rows - 1], 0, 1),
                                      ("outside", [-1, 3, table_rows, 1 << 40, 0, TD.M64 >> 1, -(1 << 63)], 0, 1),
                                      ("repeated", [7, 9, 7, 7, table_rows - 1], 0, 1),
                                      ("sharded", rng.permutation(table_rows)[:50].tolist() + [table_rows + 5], 2, 3),
                                      ("all", rng.permutation(table_rows).tolist(), 0, 1)):
            ids_np = np.asarray(ids, np.int64)
            got = tables.digest_rows(t, torch.from_numpy(ids_np).to(dev), row0=row0, row_step=step)
            want = TD.digest_ids(back, kind, dim, ids_np, row0, step)
            assert got == want, (kind, dim, what, got, want)
            if what == "all":
                assert got == (whole, table_rows, 0) and got[0] == tables.digest(t)
            if what == "outside":
                assert got[1:] == (2, 5)
            if what == "repeated":
                assert got[1:] == (5, 0) and got[0] != tables.digest_rows(t, torch.from_numpy(np.asarray([7, 9, table_rows - 1])).to(dev))[0]
        assert np.array_equal(TD.bytes_of(torch, t), raw.reshape(-1)), (kind, dim, "the table's own bytes changed")


@pytest.mark.parametrize("kind,dim", [("f32", 2), ("q8", 1), ("bf16", 64)])
def test_digest_rows_of_one_full_pass_plus_one_id(torch_cuda, kind, dim):
    """All ids of a table of one unrolled step of the full grid plus one row, in a seeded order, with three ids outside it."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    table_rows = TD.full_pass_rows(kind, dim, TD.UNROLL) + 1
    raw = TD.draw_raw(kind, dim, table_rows, 26)
    t = TD.as_table(torch, raw, kind, dim, dev)
    ids = np.random.default_rng(32).permutation(table_rows).astype(np.int64)
    got = tables.digest_rows(t, torch.from_numpy(ids).to(dev), row0=1, row_step=2)
    assert got == (TD.digest(raw.tobytes(), kind, dim, 1, 2), table_rows, 0), (kind, dim, got)
    first = ids[:TD.full_pass_rows(kind, dim) + 1].copy()
    first[[0, 5, -1]] = (-1, table_rows, 1 << 40)
    keep = np.ones(first.size, bool)
    keep[[0, 5, -1]] = False
    got = tables.digest_rows(t, torch.from_numpy(first).to(dev))
    assert got == TD.digest_ids(raw.tobytes(), kind, dim, first) and got[1:] == (int(keep.sum()), 3), (kind, dim, got)


@pytest.mark.parametrize("kind", TD.KINDS)
def test_a_digest_kept_across_an_update_is_the_digest_of_the_converted_master(torch_cuda, kind):
    """The README's promise — an updated table is byte for byte what fcp_table_convert would have written from the master with
    the delta applied — checked through the digest: update_rows_tracked's result equals digest of the updated table AND digest of
    the converted patched master."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    for dim, table_rows, n in ((5, 97, 31), (64, 1500, 700)):
        gen = torch.Generator().manual_seed(41 + dim)
        master = torch.randn((table_rows, dim), generator=gen).to(dev)
        table = master.clone() if kind == "f32" else tables.convert(master, kind)
        before = tables.digest(table)
        ids = torch.from_numpy(np.random.default_rng(42).permutation(table_rows)[:n].astype(np.int64)).to(dev)
        ids_with_outsiders = torch.cat([ids, torch.tensor([-3, table_rows], dtype=torch.int64, device=dev)])
        delta = torch.randn((n + 2, dim), generator=gen).to(dev)
        skipped = torch.zeros((1,), dtype=torch.int64, device=dev)
        after = tables.update_rows_tracked(table, ids_with_outsiders, delta, before, skipped=skipped)
        patched = master.clone()
        patched[ids] = delta[:n]
        want_table = patched if kind == "f32" else tables.convert(patched, kind)
        assert int(skipped.item()) == 2
        assert after == tables.digest(table), (kind, dim)
        assert after == tables.digest(want_table), (kind, dim)
        assert after == TD.digest(TD.bytes_of(torch, want_table).tobytes(), kind, dim) and after != before
        # sharded bookkeeping: the same delta on a digest taken with row0 / row_step
        assert tables.digest(table, row0=2, row_step=5) == TD.digest(TD.bytes_of(torch, table).tobytes(), kind, dim, 2, 5)


def test_digest_tables_of_a_plan_and_its_shards(torch_cuda):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    spec = dataclasses.replace(TM.small_mixed_spec(), n_device_inputs=4)          # a fourth device input no column reads
    dims = (4, 8, 4, 6)
    full = [TD.as_table(torch, TD.draw_raw(k, d, TM.VOCAB, 51 + i), k, d, dev) for i, (k, d) in enumerate(zip(("f32", "bf16", "q8", "f16"), dims))]
    whole = tables.digest_tables(spec, full)
    assert whole[3] is None and all(isinstance(v, int) for v in whole[:3])
    for i, (k, d) in enumerate(zip(("f32", "bf16", "q8"), dims)):
        assert whole[i] == TD.digest(TD.bytes_of(torch, full[i]).tobytes(), k, d), i
    world = 3                                                                      # 37 rows: not divisible
    ranks = [tables.digest_tables(spec.with_shard(g, world), [t[g::world].contiguous() for t in full]) for g in range(world)]
    assert all(r[3] is None for r in ranks)
    for i in range(3):
        assert sum(r[i] for r in ranks) & TD.M64 == whole[i], i
        assert len({r[i] for r in ranks}) == world


def test_two_calls_leave_the_same_bytes_and_touch_nothing_else(torch_cuda):
    """Through the C ABI with buffers of the test's own: guard words in front of and behind `out` and the workspace stay, two
    calls leave the same 32 bytes, reserved is 0, and the table is unchanged."""
    torch = torch_cuda
    from recom_amd import lib as _lib
    dev = torch.device("cuda", 0)
    L = _lib.load()
    ws_words = int(L.fcp_table_digest_workspace_bytes()) // 8
    guard = 0x5A5A5A5A5A5A5A5A
    for kind, dim, rows in (("f32", 64, 70000), ("q8", 5, 70001), ("bf16", 3, 9)):
        raw = TD.draw_raw(kind, dim, rows, 61)
        t = TD.as_table(torch, raw, kind, dim, dev)
        ids = torch.from_numpy(np.random.default_rng(62).integers(-5, rows + 5, 5000).astype(np.int64)).to(dev)
        for by_id in (False, True):
            results = []
            for _ in range(2):
                buf = torch.full((4 + 4 + 4 + ws_words + 4,), guard, dtype=torch.int64, device=dev)
                out, ws = buf[4:8], buf[12:12 + ws_words]
                stream = torch.cuda.current_stream(dev).cuda_stream
                if by_id:
                    status = L.fcp_table_digest_rows(C.c_void_p(t.data_ptr()), TD.KIND[kind], rows, dim, 0, 1, C.c_void_p(ids.data_ptr()),
                                                     int(ids.numel()), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 0, C.c_void_p(stream))
                else:
                    status = L.fcp_table_digest(C.c_void_p(t.data_ptr()), TD.KIND[kind], rows, dim, 0, 1, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(ws.data_ptr()), 0, C.c_void_p(stream))
                assert status == _lib.FCP_OK, L.fcp_last_error().decode()
                torch.cuda.synchronize()
                host = buf.cpu().numpy()
                assert (host[:4] == guard).all() and (host[8:12] == guard).all() and (host[12 + ws_words:] == guard).all(), (kind, by_id)
                results.append(host[4:8].copy())
            assert np.array_equal(results[0], results[1]), (kind, by_id)
            d = _lib.TableDigest.from_buffer_copy(results[0].tobytes())
            if by_id:
                want = TD.digest_ids(raw.tobytes(), kind, dim, ids.cpu().numpy())
                assert (d.sum, d.rows, d.skipped, d.reserved) == want + (0,), (kind, want)
            else:
                assert (d.sum, d.rows, d.skipped, d.reserved) == (TD.digest(raw.tobytes(), kind, dim), rows, 0, 0), kind
        assert np.array_equal(TD.bytes_of(torch, t), raw.reshape(-1))


def test_on_a_side_stream_behind_a_fill(torch_cuda):
    """The calls are ordered on the stream they are given: a table filled on a side stream, digested on that stream."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    t = torch.zeros((1 << 16, 64), dtype=torch.float32, device=dev)
    ids = torch.arange(0, 1 << 16, 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        t.fill_(1.5)
        got = tables.digest(t, stream=side.cuda_stream)
        got_rows = tables.digest_rows(t, ids, stream=side.cuda_stream)
    want = np.full((1 << 16, 64), 1.5, np.float32)
    assert got == TD.digest(want.tobytes(), "f32", 64)
    assert got_rows == (TD.digest(want[::2].tobytes(), "f32", 64, 0, 2), 1 << 15, 0)
    torch.cuda.synchronize()
