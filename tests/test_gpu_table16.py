"""16-bit tables on the GPU (FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16; kernels: recom_amd/csrc/fcp_tables16.hip), against the
C oracle run on `widen(tables)` with the plan's float32 twin (tests/table16_cases.py): float32 bit patterns equal wherever the
expectation is not NaN, NaN where it is.  No tolerance anywhere: a 16-bit element widens to float32 exactly.

Like the other cell tests: caller arenas filled with 0xFF first, three requests per plan, the launch report asserted (the
matching *_tab16 kernel with the cell's V, R, store policy, wide-rows bit and block counts)."""
import dataclasses
import os

import numpy as np
import pytest

import kernel_variant_cases as K
import narrow_output_cases as N
import table16_cases as T

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"bf16": "bfloat16", "f16": "float16"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _dev_tables(torch, bits_list, dtype, dev):
    """uint16 patterns -> device tensors of the table dtype."""
    td = getattr(torch, TORCH_DTYPE[dtype])
    return [torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).to(dev).view(td) for b in bits_list]


def _f32(t):
    return t.contiguous().cpu().numpy()


CELLS = T.variant_cells()


@pytest.mark.parametrize("tcell", CELLS, ids=[c.id for c in CELLS])
def test_tab16_variant_cell(torch_cuda, monkeypatch, tcell):
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    cell, dtype = tcell.cell, tcell.dtype
    case = K.build_case(*cell.key)
    if cell.store == "nt":
        monkeypatch.delenv("FCP_STORE_THROUGH_BYTES", raising=False)
    else:
        monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    diag = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] != "wide_rows"]
    monkeypatch.setenv("FCP_DIAG", ",".join(diag + (["wide_rows"] if cell.wide else [])))
    dev = torch.device("cuda", 0)
    spec = case.spec.with_table_dtype(dtype)
    bits, _wide = T.case_tables(cell.key, dtype)
    d_tabs = _dev_tables(torch, bits, dtype, dev)
    op = FeatureColumnProcess(spec, 0)
    assert op.plan.table_dtype() == dtype and op.plan.out_dtype() == "f32"
    packed = [concat_inputs(inputs) for inputs, _ in case.requests]
    need = [max(op.plan.arena_bytes(shapes, sym), 128) for (_, _, shapes), (_, sym) in zip(packed, case.requests)]
    nbytes = max(need) + 256                            # a tail no request may touch
    arenas = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if cell.store == "plain" else 3)]
    seg_ids = any(c.form == K.FORM_SEGMENT_REDUCE and c.seg_kind != K.SEG_CSR_I32 for c in spec.columns)
    bad_total = 0
    for t, ((inputs, symbols), (blob, offsets, shapes)) in enumerate(zip(case.requests, packed)):
        what = (tcell.id, t)
        arena = arenas[t % len(arenas)]
        arena.fill_(0xFF)                               # NaN-poisoned
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, symbols, arena=arena)
        torch.cuda.synchronize()
        assert out.buffer.data_ptr() == arena.data_ptr(), what
        rows = [int(r) for r in symbols]
        dense_blocks, ragged_blocks = K.expected_blocks(case.span_counts, rows, cell.rpw)
        want_launch = dict(kernel=cell.kernel + "_tab16", vec=cell.vec,
                           store=cell.store if not (cell.store == "plain" and t == 0) else "sc1_nt", wide_rows=cell.wide,
                           shard_world=1, dense_blocks=dense_blocks, ragged_blocks=ragged_blocks,
                           segment_offsets="search" if seg_ids else "none")
        if cell.kernel != "ragged":
            want_launch["rows_per_wave"] = cell.rpw
        got_launch = op.plan.last_launch()
        assert {k: got_launch[k] for k in want_launch} == want_launch, (what, got_launch)
        want, bad = T.case_expectation(cell.key, dtype, t)
        assert not any(np.isnan(w).any() for w in want), what        # (on the CPU: every element is compared as bits)
        for g, w in enumerate(want):
            assert out.groups[g].dtype == torch.float32
            assert T.assert_same_bits(_f32(out.groups[g]), w, what + ("group", g)) == 0
        need_t = op.plan.arena_bytes(shapes, symbols)
        assert bool((arena[need_t:] == 0xFF).all()), (what, "bytes beyond the request's arena were written")
        bad_total += bad
        assert op.plan.read_bad_ids() == bad_total, what
    del op


PATTERN_CELLS = [(v, dt) for v in K.VECS for dt in T.DTYPES]


@pytest.mark.parametrize("vec,dtype", PATTERN_CELLS, ids=[f"V{v}-{dt}" for v, dt in PATTERN_CELLS])
def test_every_pattern(torch_cuda, oracle, vec, dtype):
    """All 65 536 bit patterns of the dtype, once through a GATHER column (dense body: a copy) and once as bags of one id
    through a pooled SUM column (ragged body: +0.0 + x)."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    case = T.pattern_case(vec)
    dev = torch.device("cuda", 0)
    vocab = 65536 // vec
    d_tabs = _dev_tables(torch, [case.bits], dtype, dev)
    op = FeatureColumnProcess(case.spec.with_table_dtype(dtype), 0)
    blob, offsets, shapes = concat_inputs(case.inputs)
    arena = torch.empty(op.plan.arena_bytes(shapes, case.symbols) + 256, dtype=torch.uint8, device=dev)
    arena.fill_(0xFF)
    out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, case.symbols, arena=arena)
    torch.cuda.synchronize()
    launch = op.plan.last_launch()
    assert (launch["kernel"], launch["vec"], launch["rows_per_wave"]) == ("hybrid_tab16", vec, 4), launch
    assert launch["dense_blocks"] == (vocab + 15) // 16 and launch["ragged_blocks"] == (vocab + 3) // 4, launch
    wide = T.widen(case.bits, dtype)
    want, bad = oracle.process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, [wide], case.symbols)
    assert bad == 0 and op.plan.read_bad_ids() == 0
    gather, pooled = _f32(out.groups[0]), _f32(out.groups[1])
    assert gather.shape == (vocab, vec) and pooled.shape == (vocab, vec)
    # which pattern each output element read, and whether that pattern is a NaN: from the INPUT patterns
    nan_of = T.nan_patterns(dtype)
    src_g, src_p = case.bits[case.inputs[0]], case.bits[case.inputs[1]]
    assert np.array_equal(np.sort(src_g.ravel()), np.arange(65536)) and np.array_equal(np.sort(src_p.ravel()), np.arange(65536))
    nan_g, nan_p = nan_of[src_g], nan_of[src_p]
    assert int(nan_g.sum()) == int(nan_p.sum()) == (254 if dtype == "bf16" else 2046)
    assert np.array_equal(np.isnan(want[0]), nan_g) and np.array_equal(np.isnan(want[1]), nan_p)
    if dtype == "bf16":     # a copy keeps every pattern, NaN sign and payload included
        assert np.array_equal(gather.view(np.uint32), src_g.astype(np.uint32) << 16)
    else:
        assert np.isnan(gather[nan_g]).all()
        assert np.array_equal(gather.view(np.uint32)[~nan_g], want[0].view(np.uint32)[~nan_g])
    assert np.array_equal(gather.view(np.uint32)[~nan_g], wide[case.inputs[0]].view(np.uint32)[~nan_g])
    # the pooled sum: +0.0 + x — -0.0 becomes +0.0, everything else finite or infinite is x, NaN stays NaN
    assert np.isnan(pooled[nan_p]).all()
    assert np.array_equal(pooled.view(np.uint32)[~nan_p], want[1].view(np.uint32)[~nan_p])
    neg0 = src_p == 0x8000
    assert int(neg0.sum()) == 1 and pooled.view(np.uint32)[neg0][0] == 0
    del op


def _run_plan(torch, spec32, dtype, bits, requests, oracle, what, skip_cols=()):
    """A 16-bit plan against the oracle on the widened tables, request by request, in a NaN-poisoned arena.  Returns the
    op and the bad-id total.  `skip_cols`: EXTERNAL columns — not compared, and still 0xFF afterwards."""
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import LAYOUT_CONCAT
    dev = torch.device("cuda", 0)
    spec = spec32.with_table_dtype(dtype)
    wide = [T.widen(b, dtype) for b in bits]
    d_tabs = _dev_tables(torch, bits, dtype, dev)
    op = FeatureColumnProcess(spec, 0)
    twin = dataclasses.replace(spec32, layout=LAYOUT_CONCAT)
    offs = twin.column_offsets()
    bad_total = 0
    for t, (inputs, symbols) in enumerate(requests):
        blob, offsets, shapes = concat_inputs(inputs)
        arena = torch.empty(max(op.plan.arena_bytes(shapes, symbols), 128), dtype=torch.uint8, device=dev)
        arena.fill_(0xFF)
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, symbols, arena=arena)
        torch.cuda.synchronize()
        assert op.plan.last_launch()["kernel"].endswith("_tab16"), op.plan.last_launch()
        want, bad = oracle.process_feature_columns(twin.to_dict(), blob, offsets, shapes, wide, symbols)
        for k, c in enumerate(spec.columns):
            w = want[c.concat_group][:, offs[k]:offs[k] + c.dim]
            got = _f32(out.column(k)) if c.form != 6 else None
            if k in skip_cols:
                g = _f32(out.groups[c.concat_group])[:, offs[k]:offs[k] + c.dim]
                assert (g.view(np.uint32) == 0xFFFFFFFF).all(), (what, t, "EXTERNAL slot written", k)
                continue
            T.assert_same_bits(got, w, (what, dtype, t, "column", k))
        bad_total += bad
        assert op.plan.read_bad_ids() == bad_total, (what, t)
    return op, bad_total


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_copies_beside_16_bit_lookups(torch_cuda, oracle, dtype):
    """GATHER_SCATTER with its row ids in any order, PASSTHROUGH, BATCH_COL_REDUCTION and an EXTERNAL slot beside 16-bit
    lookups (the blob payloads stay float32); out-of-vocabulary and negative ids read zeros and are counted, with the
    float32 twin's counts; the same plan in FCP_LAYOUT_PER_COLUMN."""
    torch = torch_cuda
    from recom_amd.plan import LAYOUT_PER_COLUMN
    m, spec = T.mixed_spec()
    bits = [N.narrow(t, dtype) for t in m.numpy_tables()]
    requests = []
    for seed in (0, 1):
        req = m.make_request(seed)
        requests.append((T.with_bad_ids(req.inputs, spec, seed) if seed else req.inputs, req.symbols))
    ext = [k for k, c in enumerate(spec.columns) if c.form == 6]
    assert len(ext) == 1 and {c.form for c in spec.columns} == {1, 2, 3, 4, 5, 6}
    op, bad = _run_plan(torch, spec, dtype, bits, requests, oracle, "mixed", skip_cols=ext)
    assert bad > 0
    del op
    _, spec_pc = T.mixed_spec(layout=LAYOUT_PER_COLUMN)
    op, bad_pc = _run_plan(torch, spec_pc, dtype, bits, requests, oracle, "per_column")
    assert bad_pc == bad
    del op


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_id_transforms_in_front_of_16_bit_lookups(torch_cuda, oracle, dtype):
    """A filtered mean, a SELECT gather and a hashed sum."""
    spec = T.xform_spec()
    bits = [T.random_bits((c.vocab, c.dim), dtype, 40 + k) for k, c in enumerate(spec.columns)]
    op, bad = _run_plan(torch_cuda, spec, dtype, bits, [T.xform_request(29, 5), T.xform_request(70, 6)], oracle, "xform")
    assert bad > 0
    del op


def test_wrong_table_dtype_is_refused_by_the_op(torch_cuda):
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec = T.xform_spec()
    inputs, symbols = T.xform_request()
    blob, offsets, shapes = concat_inputs(inputs)
    dev = torch.device("cuda", 0)
    f32 = [torch.zeros((c.vocab, c.dim), dtype=torch.float32, device=dev) for c in spec.columns]
    for dtype in T.DTYPES:
        op = FeatureColumnProcess(spec.with_table_dtype(dtype), 0)
        with pytest.raises(ValueError, match="table"):
            op(torch.from_numpy(blob).to(dev), offsets, shapes, f32, symbols)
    op = FeatureColumnProcess(spec, 0)
    with pytest.raises(ValueError, match="table"):
        op(torch.from_numpy(blob).to(dev), offsets, shapes, [t.to(torch.bfloat16) for t in f32], symbols)


@pytest.mark.parametrize("kind", sorted(T.refused_specs()))
def test_refused_tab16_plan_reports_the_same_on_the_device(torch_cuda, monkeypatch, kind):
    """A refused plan: the same status and message from a device plan as from a host-only one."""
    from recom_amd import lib as _lib
    from recom_amd.ops import Plan
    from recom_amd.plan import FLAG_TABLES_BF16, FLAG_TABLES_F16, PlanSpec
    spec, extra, word = T.refused_specs()[kind]
    monkeypatch.setattr(PlanSpec, "validate_table_dtype", lambda self: None)      # past the Python mirror: the library decides
    monkeypatch.setattr(PlanSpec, "validate_out_dtype", lambda self: None)
    for flag in (FLAG_TABLES_BF16, FLAG_TABLES_F16):
        seen = []
        for host_only in (True, False):
            with pytest.raises(_lib.FcpError) as e:
                Plan(dataclasses.replace(spec, flags=flag | extra), 0, host_only=host_only)
            seen.append((e.value.status, str(e.value)))
        assert seen[0] == seen[1] and seen[0][0] == _lib.FCP_ERR_UNSUPPORTED and word in seen[0][1], seen
    with pytest.raises(_lib.FcpError) as e:
        Plan(dataclasses.replace(T.refused_specs()["sharded"][0], shard_world=1, shard_rank=0,
                                 flags=FLAG_TABLES_BF16 | FLAG_TABLES_F16), 0)
    assert e.value.status == _lib.FCP_ERR_INVALID_ARGUMENT


def test_s2_full_size_bf16_tables_closed_form(torch_cuda):
    """BASELINE's S2 at full size with bf16 tables (1000 columns, vocab 1M: 60 GB of tables in HBM, batch 512) against the
    closed form of the table rows, rounded once to bf16 and widened: 64-bit table addressing at 2 bytes per element, at
    scale.  Skipped if the device is too small."""
    torch = torch_cuda
    from recom_amd import synth
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    m = synth.model_s2(table_dtype="bf16")
    assert m.table_bytes() == 60 * 10 ** 9
    free, _total = torch.cuda.mem_get_info()
    if free < m.table_bytes() + (8 << 30):
        pytest.skip(f"needs {m.table_bytes() / 2**30:.0f} GiB of HBM, {free / 2**30:.0f} GiB free")
    dev = torch.device("cuda", 0)
    tabs = m.torch_tables(dev)
    assert all(t.dtype == torch.bfloat16 for t in tabs)
    op = FeatureColumnProcess(m.spec, 0)
    for seed in (0, 1):
        req = m.make_request(seed)
        blob, offsets, shapes = concat_inputs(req.inputs)
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, tabs, req.symbols)
        torch.cuda.synchronize()
        launch = op.plan.last_launch()
        # (the output side is the float32 plan's: 61 MB in a fresh arena, beyond what the L2s hold -> write-through stores)
        assert (launch["kernel"], launch["vec"], launch["rows_per_wave"], launch["store"]) == ("dense_tab16", 4, 4, "sc1_nt"), launch
        assert out.groups[0].shape == (512, 30000) and out.groups[0].dtype == torch.float32
        T.closed_form_check(m, req, _f32(out.groups[0]), "bf16")
    del tabs, op
    torch.cuda.empty_cache()
