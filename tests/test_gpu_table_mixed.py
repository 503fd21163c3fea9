"""Per-input table formats on the GPU (FCP_FLAG_TABLES_PER_INPUT; kernels: recom_amd/csrc/fcp_tables_mixed.hip), against the C
oracle run on the decoded tables with the plan's float32 twin, and against the bytes of that float32 twin run on the GPU on
the same decoded tables (tests/table_mixed_cases.py): float32 bit patterns equal wherever the expectation is not NaN, NaN where
it is.  No tolerance anywhere.

Without the feature every mixed cell fails: the flag is ignored and every table is read as float32.  That no kernel which
picks a NEIGHBOUR's loader can pass is shown on the CPU (test_table_mixed_host.py::test_a_neighbours_loader_cannot_pass)."""
import dataclasses
import os

import numpy as np
import pytest

import table_mixed_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _dev(torch, tables):
    dev = torch.device("cuda", 0)
    out = []
    for t in tables:
        t = np.array(t, copy=True)      # (the cases' arrays are read-only and shared)
        if t.dtype == np.uint16:        # 16-bit patterns: the op checks the torch dtype, the bytes are what counts
            out.append(torch.from_numpy(t.view(np.int16)).to(dev))
        else:
            out.append(torch.from_numpy(t).to(dev))
    return out


def _typed(torch, d_tabs, kinds):
    """the device tables with the torch dtype of their kind (a view: same bytes)"""
    return [t.view({"bf16": torch.bfloat16, "f16": torch.float16}[k]) if k in ("bf16", "f16") else t for t, k in zip(d_tabs, kinds)]


def _f32(t):
    return t.contiguous().cpu().numpy()


def _wide_rows_diag(monkeypatch, wide):
    diag = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] != "wide_rows"]
    monkeypatch.setenv("FCP_DIAG", ",".join(diag + (["wide_rows"] if wide else [])))


def _run(torch, op, d_blob, offsets, shapes, d_tabs, symbols):
    """one request into a NaN-poisoned arena with a tail no request may touch: (group 0 as float32, bad ids so far)"""
    need = max(op.plan.arena_bytes(shapes, symbols), 128)
    arena = torch.empty(need + 256, dtype=torch.uint8, device=d_blob.device)
    arena.fill_(0xFF)
    out = op(d_blob, offsets, shapes, d_tabs, symbols, arena=arena)
    torch.cuda.synchronize()
    assert bool((arena[need:] == 0xFF).all()), "bytes beyond the request's arena were written"
    return _f32(out.groups[0]), op.plan.read_bad_ids()


CELLS = M.cells()


@pytest.mark.parametrize("cell", CELLS, ids=[M.cell_id(c) for c in CELLS])
def test_mixed_cell(torch_cuda, monkeypatch, cell):
    """Every cell asserts, through fcp_plan_last_launch, the instantiation it reached (kernel, V, rows per wave); that the cells
    together name all 21 is test_table_mixed_host.py::test_the_cells_reach_all_21_instantiations."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    vec, flavour, batch, rpw, wide = cell
    what = M.cell_id(cell)
    _wide_rows_diag(monkeypatch, wide)
    plan = M.build_plan(vec, flavour)
    tabs, dec = M.plan_tables(vec, flavour)
    inputs, symbols = M.request(vec, flavour, batch)
    blob, offsets, shapes = concat_inputs(list(inputs))
    d_blob = torch.from_numpy(blob).to(torch.device("cuda", 0))
    want, want_bad = M.expectation(vec, flavour, batch)

    op = FeatureColumnProcess(plan.spec, 0)
    assert op.plan.table_dtype() == "mixed" and op.plan.table_dtypes() == plan.kinds and op.plan.out_dtype() == "f32"
    got, bad = _run(torch, op, d_blob, offsets, shapes, _typed(torch, _dev(torch, tabs), plan.kinds), symbols)
    launch = op.plan.last_launch()
    assert (launch["kernel"], launch["vec"], launch["wide_rows"]) == (flavour + "_tabmix", vec, wide), (what, launch)
    if flavour != "ragged":
        assert launch["rows_per_wave"] == rpw, (what, launch)
    if flavour == "dense":
        assert launch["dense_blocks"] >= 2 * -(-batch // (4 * rpw)) and launch["ragged_blocks"] == 0, (what, launch)
    if flavour == "hybrid":
        assert launch["dense_blocks"] > 0 and launch["ragged_blocks"] > 0, (what, launch)
    n_nan = M.assert_same_bits(got, want, (what, "oracle"))
    assert bad == want_bad, (what, bad, want_bad)
    if batch >= 5:
        assert want_bad > 0 and n_nan > 0, what          # ids -1 and vocab were counted; NaN rows came through
    del op

    # the float32 plan on the GPU, on the decoded tables: the same bytes (NaN for NaN), the same count of bad ids
    op32 = FeatureColumnProcess(plan.spec32, 0)
    got32, bad32 = _run(torch, op32, d_blob, offsets, shapes, _dev(torch, dec), symbols)
    assert not op32.plan.last_launch()["kernel"].endswith("_tabmix")
    M.assert_same_bits(got, got32, (what, "float32 plan on the GPU"))
    M.assert_same_bits(got32, got, (what, "float32 plan on the GPU, NaN for NaN"))
    assert bad32 == bad, what
    del op32


@pytest.mark.parametrize("kind", M.KINDS)
def test_uniform_kinds_under_the_flag_are_the_plan_wide_plan(torch_cuda, monkeypatch, kind):
    """All tables of one kind with FCP_FLAG_TABLES_PER_INPUT: the plan-wide launch family and the plan-wide plan's bytes."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    _wide_rows_diag(monkeypatch, False)
    plan = M.build_plan(4, "hybrid")
    spec32 = plan.spec32
    dims = {c.table_input: c.dim for c in spec32.columns if c.form in M.LOOKUP}
    tabs = [M.draw_table(kind, dims[t], 500 + t) for t in range(spec32.n_device_inputs)]
    inputs, symbols = M.request(4, "hybrid", 33)
    blob, offsets, shapes = concat_inputs(list(inputs))
    d_blob = torch.from_numpy(blob).to(torch.device("cuda", 0))
    d_tabs = _typed(torch, _dev(torch, tabs), (kind,) * len(tabs))
    flagged = dataclasses.replace(spec32, table_dtypes=(kind,) * spec32.n_device_inputs)      # goes through the library's flag
    assert flagged.plan_flags() & 64
    outs = []
    for spec in (flagged, spec32.with_table_dtype(kind)):
        op = FeatureColumnProcess(spec, 0)
        assert op.plan.table_dtype() == kind
        got, bad = _run(torch, op, d_blob, offsets, shapes, d_tabs, symbols)
        outs.append((got.tobytes(), bad, op.plan.last_launch()))
        del op
    family = {"f32": "hybrid", "bf16": "hybrid_tab16", "f16": "hybrid_tab16", "q8": "hybrid_tabq8"}[kind]
    assert outs[0][2]["kernel"] == family and outs[0][2] == outs[1][2], outs[0][2]
    assert outs[0][:2] == outs[1][:2]


def test_wrong_tables_are_refused_by_the_op_per_input(torch_cuda):
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec = M.small_mixed_spec().with_table_dtypes(M.SMALL_KINDS)
    dev = torch.device("cuda", 0)
    inputs = [np.arange(5, dtype=np.int64), np.arange(5, dtype=np.int64), np.arange(9, dtype=np.int64), np.asarray([0, 2, 4, 6, 8, 9], np.int32),
              np.ones(9, np.float32)]
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    good = [torch.zeros((M.VOCAB, 4), dtype=torch.float32, device=dev), torch.zeros((M.VOCAB, 8), dtype=torch.bfloat16, device=dev),
            torch.zeros((M.VOCAB, 12), dtype=torch.uint8, device=dev)]
    op = FeatureColumnProcess(spec, 0)
    out = op(d_blob, offsets, shapes, good, [5])                                    # the right tables are taken
    torch.cuda.synchronize()
    assert op.plan.last_launch()["kernel"] == "ragged_tabmix" and not _f32(out.groups[0]).any()
    for i, wrong in ((0, good[0].to(torch.bfloat16)), (1, good[1].to(torch.float16)), (1, good[1].float()),
                     (2, torch.zeros((M.VOCAB, 12), dtype=torch.float32, device=dev))):
        tabs = list(good)
        tabs[i] = wrong
        with pytest.raises(ValueError, match=rf"table {i} .*input {i}"):           # another dtype: the input is named
            op(d_blob, offsets, shapes, tabs, [5])
    with pytest.raises(ValueError, match=r"table 2 .*dim \+ 8"):                     # uint8 of the float32 table's width
        op(d_blob, offsets, shapes, good[:2] + [torch.zeros((M.VOCAB, 4), dtype=torch.uint8, device=dev)], [5])
    from recom_amd import lib as _lib
    with pytest.raises(_lib.FcpError) as e:                                          # a bf16 table of the q8 table's width
        op(d_blob, offsets, shapes, [good[0], torch.zeros((M.VOCAB, 16), dtype=torch.bfloat16, device=dev), good[2]], [5])
    assert e.value.status == _lib.FCP_ERR_SHAPE_MISMATCH
    del op


@pytest.mark.parametrize("why", sorted(M.refused_specs()))
def test_refused_mixed_plan_reports_the_same_on_the_device(torch_cuda, monkeypatch, why):
    """A refused plan: the same status and message from a device plan as from a host-only one."""
    from recom_amd import lib as _lib
    from recom_amd.ops import Plan
    from recom_amd.plan import PlanSpec
    spec, extra, word = M.refused_specs()[why]
    monkeypatch.setattr(PlanSpec, "validate_table_dtype", lambda self: None)      # past the Python mirror: the library decides
    monkeypatch.setattr(PlanSpec, "validate_out_dtype", lambda self: None)
    seen = []
    for host_only in (True, False):
        with pytest.raises(_lib.FcpError) as e:
            Plan(dataclasses.replace(spec, flags=spec.flags | extra, table_dtypes=M.SMALL_KINDS), 0, host_only=host_only)
        seen.append((e.value.status, str(e.value)))
    assert seen[0] == seen[1] and seen[0][0] == _lib.FCP_ERR_UNSUPPORTED and word in seen[0][1], seen
    assert "per-input table formats" in seen[0][1], seen


def test_s2_shape_with_kinds_by_dim(torch_cuda, oracle, monkeypatch):
    """S2's shape — 1000 columns, dims 8 / 16 / 32 / 64, batch 512: the full grid, the XCD mapping of 118 spans — with
    vocabulary 1000 and kinds by dim (8 f32, 16 bf16, 32 f16, 64 q8), against the oracle on the decoded tables."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    _wide_rows_diag(monkeypatch, False)
    model = M.s2_model()
    spec = model.spec
    assert spec.mixed_tables() and spec.n_columns == 1000 and model.batch == 512
    tabs = model.numpy_tables()
    kinds = [spec.input_table_dtype(t) for t in range(spec.n_device_inputs)]
    dec = [M.decode(t, k) for t, k in zip(tabs, kinds)]
    req = model.make_request(3)
    blob, offsets, shapes = concat_inputs(req.inputs)
    op = FeatureColumnProcess(spec, 0)
    got, bad = _run(torch, op, torch.from_numpy(blob).to(torch.device("cuda", 0)), offsets, shapes, _typed(torch, _dev(torch, tabs), kinds),
                    req.symbols)
    launch = op.plan.last_launch()
    assert (launch["kernel"], launch["vec"], launch["rows_per_wave"]) == ("dense_tabmix", 4, 4), launch
    assert launch["dense_blocks"] >= 118 * 32, launch                                 # 118 spans x 32 row tiles
    twin = spec.with_table_dtypes(None)
    want, want_bad = oracle.process_feature_columns(twin.to_dict(), blob, offsets, shapes, dec, req.symbols)
    assert M.assert_same_bits(got, want[0], "S2 shape") == 0 and bad == want_bad
    # the device tables synth builds are the same bytes
    for i, (a, b) in enumerate(zip(model.torch_tables(torch.device("cuda", 0))[:8], tabs[:8])):
        assert a.contiguous().view(torch.uint8).cpu().numpy().tobytes() == np.ascontiguousarray(b).tobytes(), i
    del op
