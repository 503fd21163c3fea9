"""Per-id weights and the sqrtn combiner on the GPU, through the C ABI, as explicit cells (tests/weighted_bag_cases.py).

Like the other cell tests: caller-owned arenas filled with 0xFF bytes before each request, three requests per plan (the
first installs descriptors, then another shape, then the first again), the launch report asserted — the weighted ragged
kernel for every plan with a weighted or sqrtn column, never for a plan without — and every result compared with the case
module's float32 restatement under the project's rule: bit patterns equal wherever the expected value is not NaN, NaN where
it is (copies: NaN payloads bit for bit as well).  The share of elements compared as "is NaN" is computed from the
restatement and asserted: zero in the form and id-path cells, at most a quarter in the weight-value cells."""
import dataclasses

import numpy as np
import pytest

import value_edge_cases as E
import weighted_bag_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _run(torch, name, case, vec, world=1, kernel="ragged_weighted", nan_cap=0.0, count_bad=False):
    """Every rank of `world` (1: the unsharded plan), three requests each; sharded: then the finalize of both shapes."""
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    spec0 = case.spec
    packed = [concat_inputs(inputs) for inputs, _ in case.requests]
    d_blobs = [torch.from_numpy(blob).to(dev) for blob, _, _ in packed]
    mask = W.copy_mask(spec0, 0)
    partials, ops, tabs = {}, [], []
    for rank in range(world):
        spec = spec0.with_shard(rank, world) if world > 1 else spec0
        d_tabs = [torch.from_numpy(np.ascontiguousarray(t[rank::world])).to(dev) for t in case.tables]
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
            assert launch["dense_blocks"] == 0 and launch["ragged_blocks"] > 0, (what, launch)
            want = W.restate(spec0, case.tables, inputs, symbols, rank, world)
            share = W.nan_share(spec0, want)
            assert share <= nan_cap, (what, share)
            E.assert_same(out.groups[0].cpu().numpy(), want.groups[0], what, mask)
            if count_bad:
                bad_total += want.bad
                assert op.plan.read_bad_ids() == bad_total, (what, op.plan.read_bad_ids(), bad_total)
            if world > 1 and t < 2:
                partials[t, rank] = out.groups[0].clone()
        ops.append(op)
        tabs.append(d_tabs)
    for t in range(2 if world > 1 else 0):
        (inputs, symbols), (blob, offsets, shapes) = case.requests[t], packed[t]
        whole = W.restate(spec0, case.tables, inputs, symbols).groups[0]
        rows = partials[t, 0].shape[0]
        sl = torch.stack([partials[t, r] for r in range(world)]).contiguous()
        r = t % world                                               # any rank may finalize any slice
        fin = torch.empty((rows, spec0.group_width(0)), dtype=torch.float32, device=dev)
        fin.view(torch.uint8).fill_(0xFF)
        ops[r].shard_finalize(d_blobs[t], offsets, shapes, tabs[r], symbols, 0, sl, world, 0, rows, out=fin)
        torch.cuda.synchronize()
        what = (name, "finalize by rank", r, "of", world, "request", t)
        want = W.finalize_restated(spec0, 0, sl.cpu().numpy(), inputs, rows)
        E.assert_same(fin.cpu().numpy(), want, what, mask)
        E.assert_same(fin.cpu().numpy()[:, mask], whole[:, mask], what + ("copies",), mask[mask])
        # the sharded order of additions differs from the unsharded one, not the value: within the float64 bound of it
        bound = W.float64_bound(spec0, case.tables, inputs, symbols)[0]
        truth = W.restate(spec0, case.tables, inputs, symbols, f64=True).groups[0]
        err = np.abs(fin.cpu().numpy().astype(np.float64) - truth)[:, ~mask]
        assert (err <= bound[:, ~mask]).all(), (what, float((err - bound[:, ~mask]).max()))
    del ops, tabs


FORM_CELLS = W.form_cells()


@pytest.mark.parametrize("cell", FORM_CELLS, ids=[c.id for c in FORM_CELLS])
def test_form_cell(torch_cuda, cell):
    """V x {weighted sum, mean, sqrtn, unweighted sqrtn} x segment encoding: bag lengths over the walk batches' edges, waves
    whose bags total exactly 384 and 385 ids, single bags of 385 and 1000 ids (fair-share rounds), empty rows; beside them,
    in the same spans, an unweighted sum and mean, a gather and a passthrough column holding -0.0 and a NaN payload."""
    _run(torch_cuda, cell.id, W.form_case(cell), cell.vec)


ID_CELLS = W.id_path_cells()


@pytest.mark.parametrize("cell", ID_CELLS, ids=[c.id for c in ID_CELLS])
def test_id_path_cell(torch_cuda, cell):
    """Weights x id path: a FILTER that drops ids in the middle and at the end of bags (their weights do not count),
    SELECT, hashed ids, ids outside the vocabulary (counted once each; a zero row whose weight still counts)."""
    _run(torch_cuda, cell.id, W.id_path_case(cell), cell.vec, count_bad=cell.path == "oov")


@pytest.mark.parametrize("vec", W.VECS)
def test_weight_value_cell(torch_cuda, vec):
    """Weights 0.0, -0.0, negative, cancelling to exactly zero over a non-zero numerator (the row is +0.0), all zero,
    subnormal weights and products, FLT_MAX products that overflow in id order, +inf and NaN."""
    _run(torch_cuda, f"values-V{vec}", W.value_case(vec), vec, nan_cap=0.25)


SHARD_CELLS = W.shard_cells()


@pytest.mark.parametrize("cell", SHARD_CELLS, ids=[c.id for c in SHARD_CELLS])
def test_row_sharded_cell(torch_cuda, cell):
    """World 2 and 3 on one GPU: every rank's weighted partial sums, then fcp_shard_finalize — slices added in rank order,
    divided by the denominator of the WHOLE row (its weights re-read, a FILTER's dropped ids left out)."""
    _run(torch_cuda, cell.id, W.shard_case(cell), cell.vec, world=cell.world)


def test_plans_without_weights_do_not_reach_the_weighted_kernel(torch_cuda):
    """The same plan with its weights and sqrtn columns turned into plain sums and means runs the unweighted ragged kernel."""
    torch = torch_cuda
    from recom_amd import plan as PL
    case = W.form_case(W.FormCell(4, "wmean", "csr"))
    cols = [dataclasses.replace(c, weights_input=-1) for c in case.spec.columns]
    plain = dataclasses.replace(case.spec, columns=cols)
    plain_case = W.Case(plain, case.tables, case.requests)
    _run(torch, "plain", plain_case, 4, kernel="ragged")
    assert all(c.combiner != PL.COMBINER_SQRTN for c in cols)


def test_staged_concat_inputs_carries_the_weights_through(torch_cuda):
    """The staged Addons>ConcatInputs form of a weighted plan with SparseTensor indices: the indices become row offsets on
    the host, the weights are copied through unchanged, the request needs neither the pre-pass nor the in-block search,
    and the result is the unstaged one bit for bit."""
    torch = torch_cuda
    from recom_amd import plan as PL
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    cell = W.FormCell(4, "wsqrtn", "idx64")
    case = W.form_case(cell)
    staged, stage = case.spec.staged_for_concat_inputs()
    assert stage.modes.count(PL.STAGE_SEG_TO_CSR) == sum(c.form == PL.FORM_SEGMENT_REDUCE for c in case.spec.columns)
    assert all(stage.modes[c.weights_input] == PL.STAGE_COPY for c in case.spec.columns if c.weights_input >= 0)
    d_tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    op = FeatureColumnProcess(staged, 0)
    plain_op = FeatureColumnProcess(case.spec, 0)
    mask = W.copy_mask(case.spec, 0)
    for t, (inputs, symbols) in enumerate(case.requests):
        blob, offsets, shapes = concat_inputs(list(inputs) + [symbols], stage)
        for c in case.spec.columns:                                   # the weights: the same bytes at their offset
            if c.weights_input >= 0:
                w = np.asarray(inputs[c.weights_input], np.float32)
                o = int(offsets[c.weights_input])
                assert np.array_equal(blob[o:o + w.nbytes].view(np.float32).view(np.uint32), w.view(np.uint32))
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, symbols)
        torch.cuda.synchronize()
        launch = op.plan.last_launch()
        assert (launch["kernel"], launch["vec"], launch["segment_offsets"]) == ("ragged_weighted", 4, "none"), launch
        want = W.restate(case.spec, case.tables, inputs, symbols)
        E.assert_same(out.groups[0].cpu().numpy(), want.groups[0], ("staged", t), mask)
        pb, po, ps = concat_inputs(inputs)
        ref = plain_op(torch.from_numpy(pb).to(dev), po, ps, d_tabs, symbols)
        torch.cuda.synchronize()
        assert plain_op.plan.last_launch()["segment_offsets"] in ("prepass", "search")
        E.assert_same(out.groups[0].cpu().numpy(), ref.groups[0].cpu().numpy(), ("staged vs as delivered", t), mask)


def test_a_weights_tensor_of_another_length_is_a_shape_mismatch(torch_cuda):
    torch = torch_cuda
    from recom_amd.lib import FcpError
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    case = W.form_case(W.FormCell(2, "wsum", "csr"))
    inputs, symbols = case.requests[0]
    c = next(c for c in case.spec.columns if c.weights_input >= 0)
    broken = list(inputs)
    broken[c.weights_input] = np.asarray(inputs[c.weights_input])[:-1].copy()
    blob, offsets, shapes = concat_inputs(broken)
    op = FeatureColumnProcess(case.spec, 0)
    with pytest.raises(FcpError) as e:
        op(torch.from_numpy(blob).to(dev), offsets, shapes, [torch.from_numpy(t).to(dev) for t in case.tables], symbols)
    assert e.value.status == 2                                        # FCP_ERR_SHAPE_MISMATCH
