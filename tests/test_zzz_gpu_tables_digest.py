"""fcp_tables_digest on the GPU (recom_amd/csrc/fcp_tables_digest.hip): every record is compared for equality with the NumPy
reference (table_digest_cases.digest / digest_ids) and with what the single-table entry leaves for the same entry; every call
runs twice into guarded buffers (tables_digest_cases.call).  The mixed model, the scaled deal, the search depth, the skew, ids
outside the table, the alignment classes with chunk and shard sums, the tracked grouped update and digest_tables of a plan.

Sorts behind tests/test_z_gpu_private_streams.py: the entry installs its records from a pinned ring, the reason
tests/test_zzz_gpu_tables_rows.py records."""
import dataclasses

import numpy as np
import pytest

import table_digest_cases as TD
import table_mixed_cases as TM
import tables_digest_cases as GD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def test_mixed_model(torch_cuda):
    """40 entries of every kind and dim in both modes in ONE call; six of them walk one full unrolled pass of their own scaled grid
    plus one row."""
    torch = torch_cuda
    specs = GD.mixed_model()
    blocks = GD.run(torch, specs, torch.device("cuda", 0), what="mixed model")
    full = [k for k, s in enumerate(specs) if s.count > GD.LONE_BLOCKS * GD.rows_per_block(s.kind, s.dim)]
    assert len(full) == 6
    for k in full:
        s = specs[k]
        assert s.count == GD.UNROLL * blocks[k] * GD.rows_per_block(s.kind, s.dim) + 1 and blocks[k] < GD.LONE_BLOCKS


def test_scaled_deal(torch_cuda):
    """24 entries that each fill the fixed grid alone: grouped, every one gets fewer blocks (asserted on the CPU first: otherwise
    the case tests nothing) and walks several trips with ITS stride, not the launch's."""
    torch = torch_cuda
    specs = GD.scaled_deal()
    shapes = [(s.kind, s.dim, s.count) for s in specs]
    dealt = GD.deal(shapes)
    assert all(b < GD.lone_blocks(*s) == GD.LONE_BLOCKS for b, s in zip(dealt, shapes))
    assert all(s.count > GD.UNROLL * b * GD.rows_per_block(s.kind, s.dim) for b, s in zip(dealt, specs))       # a second trip
    assert GD.run(torch, specs, torch.device("cuda", 0), what="scaled deal") == dealt


def test_search_depth(torch_cuda):
    """1500 one-block entries in two classes: ten steps of the search, every first-block value the end of the entry in front."""
    torch = torch_cuda
    specs = GD.search_depth()
    blocks = GD.run(torch, specs, torch.device("cuda", 0), what="search depth")
    assert blocks == [1] * 1500 and {TD.group_of(s.kind, s.dim) for s in specs} == {2, 4}


def test_skew(torch_cuda):
    torch = torch_cuda
    blocks = GD.run(torch, GD.skew(), torch.device("cuda", 0), what="skew")
    assert sorted(set(blocks)) == [1, GD.LONE_BLOCKS]


def test_ids_outside_the_table(torch_cuda):
    """-1, INT64_MIN, table_rows and 2^40 per entry (table_rows lies inside the allocation: the id array and the table are
    followed by other entries' memory), repeated ids; rows and skipped per entry."""
    torch = torch_cuda
    specs = GD.outside_ids()
    GD.run(torch, specs, torch.device("cuda", 0), what="outside ids")
    for k, s in enumerate(specs):
        inside = (s.ids >= 0) & (s.ids < s.raw.shape[0])
        assert s.want[1:] == (int(inside.sum()), int((~inside).sum())), k
    assert [s.want[2] for s in specs[:4]] == [4, 0, 1, 9] and specs[3].want[:2] == (0, 0)
    # a repeated id counts as often as it occurs: the sum differs from that of the distinct ids
    s = specs[0]
    distinct = np.unique(s.ids)
    assert distinct.size < s.ids.size and TD.digest_ids(s.raw.tobytes(), s.kind, s.dim, distinct)[0] != s.want[0]


def test_alignment_classes_chunks_and_shards_in_one_call(torch_cuda):
    """q8 dim-1 views t[a:] for a = 1 .. 8 (9-byte rows at every byte alignment) and bf16 dim-1 views (every even one), each with
    row0 = a, in ONE call with the chunks [0, a) and the whole: the last row of every view ends where the table ends, in front
    of a poisoned guard.  Chunks add up to the whole; ranks row0 = g, row_step = world add up to the unsharded table."""
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    rows, world = 777, 3
    items, wants, layout = [], [], {}
    bufs = []
    for kind in ("q8", "bf16"):
        raw = TD.draw_raw(kind, 1, rows, 23)
        buf = torch.full((raw.size + 64,), 0xA5, dtype=torch.uint8, device=dev)
        buf[:raw.size].copy_(torch.from_numpy(raw.reshape(-1)))
        bufs.append((buf, raw.size))
        body = buf[:raw.size]
        t = body.view(rows, 9) if kind == "q8" else body.view(torch.bfloat16).view(rows, 1)
        layout[kind, "whole"] = len(items)
        items.append(GD.Item(t, kind, 1))
        wants.append(TD.digest(raw.tobytes(), kind, 1))
        starts = set()
        for a in range(1, 9):
            layout[kind, a] = len(items)
            items.append(GD.Item(t[a:], kind, 1, row0=a))
            wants.append(TD.digest(raw[a:].tobytes(), kind, 1, a))
            items.append(GD.Item(t[:a], kind, 1))
            wants.append(TD.digest(raw[:a].tobytes(), kind, 1))
            starts.add(t[a:].data_ptr() % 8)
        assert starts == (set(range(8)) if kind == "q8" else {0, 2, 4, 6})
        layout[kind, "ranks"] = len(items)
        for g in range(world):
            items.append(GD.Item(t[g::world].contiguous(), kind, 1, row0=g, step=world))
            wants.append(TD.digest(np.ascontiguousarray(raw[g::world]).tobytes(), kind, 1, g, world))
    # q8 rows of 16 bytes at every byte of an 8-byte word: the address alone decides A, 8 | 1 | 2 | 1 | 4 | 1 | 2 | 1
    for front in range(8):
        raw = TD.draw_raw("q8", 8, 300, 24 + front)
        items.append(GD.Item(TD.as_table(torch, raw, "q8", 8, dev, front=front), "q8", 8, row0=front))
        wants.append(TD.digest(raw.tobytes(), "q8", 8, front))
    assert [GD.align_of(it.table.data_ptr(), "q8", 8) for it in items[-8:]] == [8, 1, 2, 1, 4, 1, 2, 1]
    got, _blocks = GD.call(torch, items, dev, what="alignment classes")
    assert [g[0] for g in got] == wants
    assert all(g[1:] == (int(it.table.shape[0]), 0) for g, it in zip(got, items))
    for kind in ("q8", "bf16"):
        whole = got[layout[kind, "whole"]][0]
        for a in range(1, 9):
            k = layout[kind, a]
            assert (got[k][0] + got[k + 1][0]) & TD.M64 == whole, (kind, a)
        k = layout[kind, "ranks"]
        assert sum(g[0] for g in got[k:k + world]) & TD.M64 == whole, kind
    for buf, size in bufs:
        assert bool((buf[size:] == 0xA5).all())


def test_update_rows_grouped_tracked_over_the_mixed_model(torch_cuda):
    """Every returned digest equals tables.digest of the updated table and digest_host of the converted patched master; the
    digests handed in are those of one grouped call."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(77)
    masters, tabs, ids, deltas, kinds = [], [], [], [], []
    for i in range(40):
        kind, dim = GD.KINDS[i % 4], TD.DIMS[(i + i // 20) % 10]
        table_rows = (1, 2, 97, 1500)[i % 4 if i % 7 else 3]
        n = 0 if i in (0, 19, 20, 39) else max(1, table_rows // (1 + i % 3))
        master = torch.randn((table_rows, dim), generator=gen).to(dev)
        masters.append(master), kinds.append(kind)
        tabs.append(master.clone() if kind == "f32" else tables.convert(master, kind))
        own = torch.from_numpy(np.random.default_rng(80 + i).permutation(table_rows)[:n].astype(np.int64)).to(dev)
        ids.append(torch.cat([own, torch.tensor([-3, table_rows], dtype=torch.int64, device=dev)]) if n else own)
        deltas.append(torch.randn((int(ids[-1].shape[0]), dim), generator=gen).to(dev))
    row0s, steps = [i % 5 for i in range(40)], [1 + i % 4 for i in range(40)]
    before = tables.digests_grouped(tabs, row0=row0s, row_step=steps)
    assert before == [tables.digest(t, row0=r, row_step=s) for t, r, s in zip(tabs, row0s, steps)]
    by_id = tables.digest_rows_grouped(tabs, ids, row0=row0s, row_step=steps)
    assert by_id == [tables.digest_rows(t, i, row0=r, row_step=s) for t, i, r, s in zip(tabs, ids, row0s, steps)]
    skipped = torch.zeros((40,), dtype=torch.int64, device=dev)
    after = tables.update_rows_grouped_tracked(tabs, ids, deltas, before, row0=row0s, row_step=steps, skipped=skipped)
    assert skipped.cpu().tolist() == [2 if int(i.shape[0]) else 0 for i in ids]
    for k in range(40):
        n = max(int(ids[k].shape[0]) - 2, 0)
        patched = masters[k].clone()
        patched[ids[k][:n]] = deltas[k][:n]
        want = patched if kinds[k] == "f32" else tables.convert(patched, kinds[k])
        assert after[k] == tables.digest(tabs[k], row0=row0s[k], row_step=steps[k]), k
        assert after[k] == tables.digest_host(want.cpu(), kinds[k], row0=row0s[k], row_step=steps[k]), k
        assert (after[k] != before[k]) == (n > 0), k


def test_digest_tables_of_a_plan_is_the_per_table_list(torch_cuda):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    spec = dataclasses.replace(TM.small_mixed_spec(), n_device_inputs=4)          # a fourth device input no column reads
    dims = (4, 8, 4, 6)
    full = [TD.as_table(torch, TD.draw_raw(k, d, TM.VOCAB, 51 + i), k, d, dev) for i, (k, d) in enumerate(zip(("f32", "bf16", "q8", "f16"), dims))]
    read = set(spec.read_inputs())
    for g, world in ((0, 1), (1, 3)):
        sharded = spec.with_shard(g, world) if world > 1 else spec
        mine = [t[g::world].contiguous() for t in full]
        got = tables.digest_tables(sharded, mine)
        assert got == [tables.digest(t, row0=g, row_step=world) if i in read else None for i, t in enumerate(mine)]
        assert got[3] is None and all(isinstance(v, int) for v in got[:3])
