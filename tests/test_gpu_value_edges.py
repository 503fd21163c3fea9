"""The fused kernels at their edge values, as explicit cells (tests/value_edge_cases.py): the id path (hash, transform,
vocabulary check, shard split) through its four readers, row-sharded ids at and beyond 2^31 and 2^32, and pooled sums and
means over +-inf, NaN, +-FLT_MAX, subnormals and -0.0.

Like the cells of tests/test_gpu_kernel_variants.py: caller-owned arenas filled with 0xFF bytes before each request, the
launch report asserted (kernel, V, shard world: the cell is reached, not assumed), three requests per plan (the first
installs descriptors, then a different one, then the first again), the bad-id counter asserted cumulatively.  Every result
is compared with the case module's NumPy restatement and with the C oracle under one rule (`value_edge_cases.assert_same`):
bit patterns equal wherever the expected value is not NaN, NaN where it is.  Row-sharded cells run every rank and push the
partials through fcp_shard_finalize, against `aux_kernel_cases.finalize_restated`."""
import numpy as np
import pytest

import value_edge_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _run_cell(torch, oracle, name, case, world, kernel, vec):
    """Every rank of `world` (1: the unsharded plan), three requests each, then — sharded — the finalize of every group."""
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    spec0 = case.spec
    packed = [concat_inputs(inputs) for inputs, _ in case.requests]
    d_blobs = [torch.from_numpy(blob).to(dev) for blob, _, _ in packed]
    masks = [E.copy_mask(spec0, g) for g in range(spec0.n_groups)]
    partials = {}                  # (t, rank) -> device groups
    ops, tabs = [], []
    for rank in range(world):
        spec = spec0.with_shard(rank, world) if world > 1 else spec0
        h_tabs = [np.ascontiguousarray(t[rank::world]) for t in case.tables]
        d_tabs = [torch.from_numpy(t).to(dev) for t in h_tabs]
        op = FeatureColumnProcess(spec, 0)
        nbytes = max(max(op.plan.arena_bytes(shapes, sym), 128) for (_, _, shapes), (_, sym) in zip(packed, case.requests))
        arenas = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        bad_total = 0
        for t, ((inputs, symbols), (blob, offsets, shapes)) in enumerate(zip(case.requests, packed)):
            what = (name, "rank", rank, "of", world, "request", t)
            arena = arenas[t % 2]
            arena.fill_(0xFF)
            out = op(d_blobs[t], offsets, shapes, d_tabs, symbols, arena=arena)
            torch.cuda.synchronize()
            assert out.buffer.data_ptr() == arena.data_ptr(), what
            launch = op.plan.last_launch()
            assert (launch["kernel"], launch["vec"], launch["shard_world"]) == (kernel, vec, world), (what, launch)
            got = [g.cpu().numpy() for g in out.groups]
            want, want_bad = E.restate(spec0, case.tables, inputs, symbols, rank, world)
            orc, orc_bad = oracle.process_feature_columns(spec.to_dict(), blob, offsets, shapes, h_tabs, symbols)
            for g in range(spec0.n_groups):
                E.assert_same(got[g], want[g], what + ("group", g, "restated"), masks[g])
                E.assert_same(got[g], orc[g], what + ("group", g, "oracle"), masks[g])
            assert want_bad == orc_bad, what
            bad_total += want_bad
            assert op.plan.read_bad_ids() == bad_total, (what, op.plan.read_bad_ids(), bad_total)
            if world > 1 and t < 2:
                partials[t, rank] = [g.clone() for g in out.groups]
        ops.append(op)
        tabs.append(d_tabs)
    for t in range(2 if world > 1 else 0):
        (inputs, symbols), (blob, offsets, shapes) = case.requests[t], packed[t]
        whole, _ = E.restate(spec0, case.tables, inputs, symbols)
        for g in range(spec0.n_groups):
            rows = partials[t, 0][g].shape[0]
            sl = torch.stack([partials[t, r][g] for r in range(world)]).contiguous()
            r = (t + g) % world                                   # any rank may finalize any slice
            fin = torch.empty((rows, spec0.group_width(g)), dtype=torch.float32, device=dev)
            fin.view(torch.uint8).fill_(0xFF)
            ops[r].shard_finalize(d_blobs[t], offsets, shapes, tabs[r], symbols, g, sl, world, 0, rows, out=fin)
            torch.cuda.synchronize()
            what = (name, "finalize by rank", r, "of", world, "request", t, "group", g)
            E.assert_same(fin.cpu().numpy(), E.finalized(spec0, g, sl.cpu().numpy(), inputs, rows), what, masks[g])
            # one-owner columns: the unsharded result bit for bit
            E.assert_same(fin.cpu().numpy()[:, masks[g]], whole[g][:, masks[g]], what + ("copies",), masks[g][masks[g]])
    del ops, tabs


ID_CELLS = E.id_cells()


@pytest.mark.parametrize("cell", ID_CELLS, ids=[c.id for c in ID_CELLS])
def test_id_path_cell(torch_cuda, oracle, cell):
    """Hash (every length branch of the decimal string), SELECT / FILTER over interval lists up to five long with ends and
    substitutes at the int64 extremes, the vocabulary check and the shard split, read by the dense body (group 0), the
    ragged body and the any-order ScatterNd pre-pass (group 1), and by the finalize's kept count."""
    _run_cell(torch_cuda, oracle, cell.id, E.id_case(cell), cell.world, "hybrid", cell.dim)


def test_int64_min_inside_a_filter_interval_counts(torch_cuda):
    """FILTER [INT64_MIN, 5] keeps the id INT64_MIN: it reads zeros, counts in the mean ([3.5, 4.0], not [7.0, 8.0]) and as a
    bad id.  (A kernel that reports "dropped" through a reserved id value divides by one id fewer and counts none.)"""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec, tables, inputs, symbols, want, want_bad = E.min_collision_case()
    dev = torch.device("cuda", 0)
    blob, offsets, shapes = concat_inputs(inputs)
    op = FeatureColumnProcess(spec, 0)
    out = op(torch.from_numpy(blob).to(dev), offsets, shapes, [torch.from_numpy(t).to(dev) for t in tables], symbols)
    torch.cuda.synchronize()
    got = out.groups[0].cpu().numpy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert op.plan.read_bad_ids() == want_bad


SPECIAL_CELLS = E.special_cells()


@pytest.mark.parametrize("cell", SPECIAL_CELLS, ids=[c.id for c in SPECIAL_CELLS])
def test_pooled_specials_cell(torch_cuda, oracle, cell):
    """Sums, means and filtered means over +-inf, inf - inf, NaN rows, FLT_MAX overflow in id order, subnormal sums and
    quotients, -0.0 rows and the zero line, at bag lengths on both sides of the walk batches and inside a long bag; sharded:
    the finalize's own add produces inf - inf, the overflow and the subnormal sum."""
    _run_cell(torch_cuda, oracle, cell.id, E.special_case(cell.kernel, cell.vec), cell.world, cell.kernel, cell.vec)


def test_sharded_ids_at_and_beyond_two_to_the_32(torch_cuda):
    """A table of 2^32 + 2^16 rows over three ranks (one rank's share at a time, zero-filled, then the true and the decoy
    rows written): ids on both sides of 2^31 - 1 and of 2^32 are split in 64 bits, to the row that holds their value and
    not to where a truncated id or a 32-bit division would read."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec0, requests, value, true, decoy = E.big_case()
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info()
    need = max(E.big_rows(r) for r in range(E.BIG_WORLD)) * 4
    if free < need + (8 << 30):
        pytest.skip(f"needs {need / 2**30:.0f} GiB of HBM, {free / 2**30:.0f} GiB free")
    packed = [concat_inputs(inputs) for inputs, _ in requests]
    for rank in range(E.BIG_WORLD):
        table = torch.zeros((E.big_rows(rank), 1), dtype=torch.float32, device=dev)
        rows = {**decoy[rank], **true[rank]}
        idx = torch.from_numpy(np.fromiter(rows.keys(), np.int64, len(rows))).to(dev)
        table[idx, 0] = torch.from_numpy(np.fromiter(rows.values(), np.float32, len(rows))).to(dev)
        op = FeatureColumnProcess(spec0.with_shard(rank, E.BIG_WORLD), 0)
        bad_total = 0
        for t, ((inputs, symbols), (blob, offsets, shapes)) in enumerate(zip(requests, packed)):
            what = ("rank", rank, "request", t)
            arena = torch.full((max(op.plan.arena_bytes(shapes, symbols), 128),), 0xFF, dtype=torch.uint8, device=dev)
            out = op(torch.from_numpy(blob).to(dev), offsets, shapes, [table], symbols, arena=arena)
            torch.cuda.synchronize()
            launch = op.plan.last_launch()
            assert (launch["kernel"], launch["vec"], launch["shard_world"]) == ("hybrid", 1, E.BIG_WORLD), (what, launch)
            want, bad = E.big_expected(value, inputs, rank, E.BIG_WORLD)
            for g in range(2):
                E.assert_same(out.groups[g].cpu().numpy(), want[g], what + ("group", g))
            bad_total += bad
            assert op.plan.read_bad_ids() == bad_total, what
        del op, table, out, arena
        torch.cuda.empty_cache()
