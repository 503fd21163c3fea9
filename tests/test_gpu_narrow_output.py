"""Narrow output on the GPU (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16; kernels: recom_amd/csrc/fcp_narrow.hip), against
`narrow(oracle float32 output)` — the C oracle run on the plan's float32 twin, rounded once to nearest-even by the
restatement of tests/narrow_output_cases.py — as 16-bit patterns: equal wherever the expectation is not NaN, NaN where it is.

Like the other cell tests: caller arenas filled with 0xFF first, three requests per plan, the launch report asserted (the
matching *_narrow kernel with the cell's V, R, store policy, wide-rows bit and block counts)."""
import dataclasses
import os

import numpy as np
import pytest

import kernel_variant_cases as K
import narrow_output_cases as N

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"bf16": "bfloat16", "f16": "float16"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _bits16(torch, t):
    """The 16-bit patterns of a bf16 / fp16 device tensor."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _check_groups(torch, out, want32, dtype, what) -> float:
    """Every group against narrow(float32 expectation); returns the share of elements compared as "is NaN"."""
    nan = total = 0.0
    for g, (got, w) in enumerate(zip(out.groups, want32)):
        assert got.dtype == getattr(torch, TORCH_DTYPE[dtype]), (what, got.dtype)
        share = N.assert_same16(_bits16(torch, got), w, dtype, what + ("group", g))
        nan += share * w.size
        total += w.size
    return nan / max(total, 1.0)


def _check_arena_tail(torch, arena, op, shapes, symbols, spec, csr_off, what):
    """Narrow layout in bytes: group g lies at the 128-byte aligned running offset of rows x width x 2; padding between
    groups, and everything beyond the request's outputs and scratch, is still 0xFF."""
    need = op.plan.arena_bytes(shapes, symbols)
    host = arena.cpu().numpy()
    assert (host[need:] == 0xFF).all(), (what, "bytes beyond the request's arena were written")
    cursor = 0
    for g in range(spec.n_groups):
        nbytes = spec.group_rows(g, shapes, symbols) * spec.group_width(g) * 2
        end = cursor + -(-nbytes // 128) * 128
        assert (host[cursor + nbytes:end] == 0xFF).all(), (what, "padding behind group", g)
        cursor = end
    assert cursor == csr_off or csr_off < 0, (what, cursor, csr_off)
    if cursor == need:              # no scratch: the output region is the whole arena
        return
    assert need > cursor and (need - cursor) % 4 == 0


CELLS = N.variant_cells()


@pytest.mark.parametrize("ncell", CELLS, ids=[c.id for c in CELLS])
def test_narrow_variant_cell(torch_cuda, oracle, monkeypatch, ncell):
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    cell, dtype = ncell.cell, ncell.dtype
    case = K.build_case(*cell.key)
    if cell.store == "nt":
        monkeypatch.delenv("FCP_STORE_THROUGH_BYTES", raising=False)
    else:
        monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    diag = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] != "wide_rows"]
    monkeypatch.setenv("FCP_DIAG", ",".join(diag + (["wide_rows"] if cell.wide else [])))
    dev = torch.device("cuda", 0)
    spec = case.spec.with_out_dtype(dtype)
    twin = case.spec.to_dict()                          # the float32 twin: what the oracle computes
    d_tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    op = FeatureColumnProcess(spec, 0)
    assert op.plan.out_dtype() == dtype
    packed = [concat_inputs(inputs) for inputs, _ in case.requests]
    need = [max(op.plan.arena_bytes(shapes, sym), 128) for (_, _, shapes), (_, sym) in zip(packed, case.requests)]
    nbytes = max(need) + 256                            # a tail no request may touch
    arenas = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if cell.store == "plain" else 3)]
    seg_ids = any(c.form == K.FORM_SEGMENT_REDUCE and c.seg_kind != K.SEG_CSR_I32 for c in spec.columns)
    bad_total = 0
    nan_share = 0.0
    for t, ((inputs, symbols), (blob, offsets, shapes)) in enumerate(zip(case.requests, packed)):
        what = (ncell.id, t)
        arena = arenas[t % len(arenas)]
        arena.fill_(0xFF)
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, symbols, arena=arena)
        torch.cuda.synchronize()
        assert out.buffer.data_ptr() == arena.data_ptr(), what
        rows = [int(r) for r in symbols]
        dense_blocks, ragged_blocks = K.expected_blocks(case.span_counts, rows, cell.rpw)
        want_launch = dict(kernel=cell.kernel + "_narrow", vec=cell.vec,
                           store=cell.store if not (cell.store == "plain" and t == 0) else "sc1_nt", wide_rows=cell.wide,
                           shard_world=1, dense_blocks=dense_blocks, ragged_blocks=ragged_blocks,
                           segment_offsets="search" if seg_ids else "none")
        if cell.kernel != "ragged":
            want_launch["rows_per_wave"] = cell.rpw
        got_launch = op.plan.last_launch()
        assert {k: got_launch[k] for k in want_launch} == want_launch, (what, got_launch)
        want, bad = oracle.process_feature_columns(twin, blob, offsets, shapes, case.tables, symbols)
        nan_share = max(nan_share, _check_groups(torch, out, want, dtype, what))
        for g in range(spec.n_groups):
            assert tuple(out.groups[g].shape) == want[g].shape
            assert out.groups[g].data_ptr() == int(out.output_ptrs[[k for k, c in enumerate(spec.columns)
                                                                    if c.concat_group == g and c.concat_slot == 0][0]])
        assert (out.output_row_strides == [spec.group_width(c.concat_group) for c in spec.columns]).all()
        _check_arena_tail(torch, arena, op, shapes, symbols, spec, op.plan.last_csr()[0], what)
        bad_total += bad
        assert op.plan.read_bad_ids() == bad_total, what
    assert nan_share == 0.0
    del op


EDGE_CELLS = [(v, dt) for v in K.VECS for dt in N.DTYPES]


@pytest.mark.parametrize("vec,dtype", EDGE_CELLS, ids=[f"V{v}-{dt}" for v, dt in EDGE_CELLS])
def test_narrow_edge_cell(torch_cuda, oracle, vec, dtype):
    """GATHER and PASSTHROUGH columns carrying the edge list (ties, FLT_MAX, the fp16 overflow edge, both subnormal ranges,
    float32 subnormals, +-0.0, +-inf, NaNs) through the dense and the ragged body; pooled sums and means that land on ties,
    on the fp16 overflow edge, in both subnormal ranges, on -0.0, +-inf and NaN (inf - inf), beside rows without ids."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    case = N.edge_case(vec)
    dev = torch.device("cuda", 0)
    spec = case.spec.with_out_dtype(dtype)
    twin = case.spec.to_dict()
    d_tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    op = FeatureColumnProcess(spec, 0)
    packed = [concat_inputs(inputs) for inputs, _ in case.requests]
    nbytes = max(max(op.plan.arena_bytes(shapes, sym), 128) for (_, _, shapes), (_, sym) in zip(packed, case.requests)) + 256
    arenas = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
    for t, ((inputs, symbols), (blob, offsets, shapes)) in enumerate(zip(case.requests, packed)):
        what = ("edge", vec, dtype, t)
        arena = arenas[t % 2]
        arena.fill_(0xFF)
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, symbols, arena=arena)
        torch.cuda.synchronize()
        launch = op.plan.last_launch()
        assert (launch["kernel"], launch["vec"], launch["shard_world"]) == ("hybrid_narrow", vec, 1), (what, launch)
        assert launch["dense_blocks"] > 0 and launch["ragged_blocks"] > 0
        want, bad = oracle.process_feature_columns(twin, blob, offsets, shapes, case.tables, symbols)
        share = _check_groups(torch, out, want, dtype, what)
        # computed from the expectation: the NaN rows of the edge list and inf - inf
        assert 0.0 < share <= 0.25, (what, share)
        _check_arena_tail(torch, arena, op, shapes, symbols, spec, op.plan.last_csr()[0], what)
        assert op.plan.read_bad_ids() == 0 and bad == 0
    del op


@pytest.mark.parametrize("kind", sorted(N.refused_specs()))
def test_refused_narrow_plan_reports_the_same_on_the_device(torch_cuda, monkeypatch, kind):
    """A refused narrow plan: the same status and message from a device plan as from a host-only one."""
    from recom_amd import lib as _lib
    from recom_amd.ops import Plan
    from recom_amd.plan import FLAG_OUT_BF16, FLAG_OUT_F16, PlanSpec
    spec, word = N.refused_specs()[kind]
    monkeypatch.setattr(PlanSpec, "validate_out_dtype", lambda self: None)      # past the Python mirror: the library decides
    for flag in (FLAG_OUT_BF16, FLAG_OUT_F16):
        seen = []
        for host_only in (True, False):
            with pytest.raises(_lib.FcpError) as e:
                Plan(dataclasses.replace(spec, flags=flag), 0, host_only=host_only)
            seen.append((e.value.status, str(e.value)))
        assert seen[0] == seen[1] and seen[0][0] == _lib.FCP_ERR_UNSUPPORTED and word in seen[0][1], seen
    with pytest.raises(_lib.FcpError) as e:
        Plan(dataclasses.replace(N.refused_specs()["sharded"][0], shard_world=1, shard_rank=0, flags=FLAG_OUT_BF16 | FLAG_OUT_F16), 0)
    assert e.value.status == _lib.FCP_ERR_INVALID_ARGUMENT


def test_groups_only_and_fresh_arenas(torch_cuda, oracle):
    """The lean call and library-sized fresh arenas return the same narrow views."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    case = N.edge_case(2)
    dev = torch.device("cuda", 0)
    d_tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    inputs, symbols = case.requests[1]
    blob, offsets, shapes = concat_inputs(inputs)
    want, _ = oracle.process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, case.tables, symbols)
    for dtype in N.DTYPES:
        op = FeatureColumnProcess(case.spec.with_out_dtype(dtype), 0)
        d_blob = torch.from_numpy(blob).to(dev)
        groups = op.groups_only(d_blob, offsets, shapes, d_tabs, symbols)
        out = op(d_blob, offsets, shapes, d_tabs, symbols)
        torch.cuda.synchronize()
        assert out.buffer.numel() == max(op.plan.arena_bytes(shapes, symbols), 128)
        for g, w in enumerate(want):
            N.assert_same16(_bits16(torch, groups[g]), w, dtype, ("groups_only", dtype, g))
            N.assert_same16(_bits16(torch, out.groups[g]), w, dtype, ("call", dtype, g))
        k = 3                                           # ProcessOutputs.column: a strided narrow view
        c = case.spec.columns[k]
        off = case.spec.column_offsets()[k]
        N.assert_same16(_bits16(torch, out.column(k)), want[c.concat_group][:, off:off + c.dim], dtype, ("column", dtype))


def test_s2_full_size_bf16_closed_form(torch_cuda):
    """BASELINE's S2 at full size (1000 columns, batch 512: a [512, 30000] bf16 matrix, 30.7 MB) against the narrowed
    closed form of the table rows: 64-bit output addressing at 2 bytes per element, at scale."""
    torch = torch_cuda
    from recom_amd import synth
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    m = synth.model_s2(out_dtype="bf16")
    free, _total = torch.cuda.mem_get_info()
    if free < m.table_bytes() + (8 << 30):
        pytest.skip(f"needs {m.table_bytes() / 2**30:.0f} GiB of HBM, {free / 2**30:.0f} GiB free")
    dev = torch.device("cuda", 0)
    tabs = m.torch_tables(dev)
    op = FeatureColumnProcess(m.spec, 0)
    for seed in (0, 1):
        req = m.make_request(seed)
        blob, offsets, shapes = concat_inputs(req.inputs)
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, tabs, req.symbols)
        torch.cuda.synchronize()
        launch = op.plan.last_launch()
        assert (launch["kernel"], launch["vec"], launch["rows_per_wave"], launch["store"]) == ("dense_narrow", 4, 4, "nt"), launch
        assert out.groups[0].shape == (512, 30000) and out.groups[0].dtype == torch.bfloat16
        assert out.buffer.numel() == 512 * 30000 * 2
        N.closed_form_check16(m, req, _bits16(torch, out.groups[0]), "bf16")
    del tabs, op
    torch.cuda.empty_cache()
