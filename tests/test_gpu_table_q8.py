"""8-bit row-quantised tables on the GPU (FCP_FLAG_TABLES_Q8; kernels: recom_amd/csrc/fcp_tables_q8.hip), against the C oracle
run on `dequantize(tables)` with the plan's float32 twin (tests/table_q8_cases.py): float32 bit patterns equal wherever the
expectation is not NaN, NaN where it is.  No tolerance anywhere: an element is fma(float(code), scale, bias) rounded once, and
everything behind it is the float32 plan's.

Like the other cell tests: caller arenas filled with 0xFF first, three requests per plan, the launch report asserted (the
matching *_tabq8 kernel with the cell's V, R, store policy, wide-rows bit and block counts), bytes beyond the request's arena
untouched, bad-id counts equal to the twin's."""
import dataclasses
import os

import numpy as np
import pytest

import kernel_variant_cases as K
import table_q8_cases as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _dev_tables(torch, tables, dev):
    return [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in tables]


def _f32(t):
    return t.contiguous().cpu().numpy()


def _no_wide_rows_diag(monkeypatch, wide=False):
    diag = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] != "wide_rows"]
    monkeypatch.setenv("FCP_DIAG", ",".join(diag + (["wide_rows"] if wide else [])))


CELLS = Q.variant_cells()


@pytest.mark.parametrize("cell", CELLS, ids=[Q.cell_id(c) for c in CELLS])
def test_tabq8_variant_cell(torch_cuda, monkeypatch, cell):
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    case = K.build_case(*cell.key)
    if cell.store == "nt":
        monkeypatch.delenv("FCP_STORE_THROUGH_BYTES", raising=False)
    else:
        monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    _no_wide_rows_diag(monkeypatch, cell.wide)
    dev = torch.device("cuda", 0)
    spec = case.spec.with_table_dtype("q8")
    q8, _deq = Q.case_tables(cell.key)
    d_tabs = _dev_tables(torch, q8, dev)
    op = FeatureColumnProcess(spec, 0)
    assert op.plan.table_dtype() == "q8" and op.plan.out_dtype() == "f32"
    packed = [concat_inputs(inputs) for inputs, _ in case.requests]
    need = [max(op.plan.arena_bytes(shapes, sym), 128) for (_, _, shapes), (_, sym) in zip(packed, case.requests)]
    nbytes = max(need) + 256                            # a tail no request may touch
    arenas = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if cell.store == "plain" else 3)]
    seg_ids = any(c.form == K.FORM_SEGMENT_REDUCE and c.seg_kind != K.SEG_CSR_I32 for c in spec.columns)
    bad_total = 0
    for t, ((inputs, symbols), (blob, offsets, shapes)) in enumerate(zip(case.requests, packed)):
        what = (Q.cell_id(cell), t)
        arena = arenas[t % len(arenas)]
        arena.fill_(0xFF)                               # NaN-poisoned
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, symbols, arena=arena)
        torch.cuda.synchronize()
        assert out.buffer.data_ptr() == arena.data_ptr(), what
        rows = [int(r) for r in symbols]
        dense_blocks, ragged_blocks = K.expected_blocks(case.span_counts, rows, cell.rpw)
        want_launch = dict(kernel=cell.kernel + "_tabq8", vec=cell.vec,
                           store=cell.store if not (cell.store == "plain" and t == 0) else "sc1_nt", wide_rows=cell.wide,
                           shard_world=1, dense_blocks=dense_blocks, ragged_blocks=ragged_blocks,
                           segment_offsets="search" if seg_ids else "none")
        if cell.kernel != "ragged":
            want_launch["rows_per_wave"] = cell.rpw
        got_launch = op.plan.last_launch()
        assert {k: got_launch[k] for k in want_launch} == want_launch, (what, got_launch)
        want, bad = Q.case_expectation(cell.key, t)
        assert not any(np.isnan(w).any() for w in want), what        # (on the CPU: every element is compared as bits)
        for g, w in enumerate(want):
            assert out.groups[g].dtype == torch.float32
            assert Q.assert_same_bits(_f32(out.groups[g]), w, what + ("group", g)) == 0
        need_t = op.plan.arena_bytes(shapes, symbols)
        assert bool((arena[need_t:] == 0xFF).all()), (what, "bytes beyond the request's arena were written")
        bad_total += bad
        assert op.plan.read_bad_ids() == bad_total, what
    del op


@pytest.mark.parametrize("vec", K.VECS, ids=[f"V{v}-dim{Q.MISALIGNED_DIMS[v]}" for v in K.VECS])
def test_misaligned_rows_with_the_edge_list(torch_cuda, oracle, monkeypatch, vec):
    """Rows of 11 / 14 / 20 bytes (V = 1 / 2 / 4): no slot-multiples of 16 bytes, scale and bias at every byte (V = 1), even
    (V = 2) or 4-byte (V = 4) alignment, rows across 128-byte lines and a 4 KiB page; in them every edge scale with every
    edge bias, all 256 codes, products that overflow alone and results on float32 ties.  Once through a GATHER column (the
    dense body: a copy) and once as bags of one id through a pooled SUM column (the ragged body: +0.0 + x)."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    _no_wide_rows_diag(monkeypatch)
    case = Q.edge_case(vec)
    dim = Q.MISALIGNED_DIMS[vec]
    vocab = case.table.shape[0]
    assert case.table.shape == (vocab, dim + 8) and (dim + 8) % 16 != 0
    dev = torch.device("cuda", 0)
    d_tabs = _dev_tables(torch, [case.table], dev)
    op = FeatureColumnProcess(case.spec.with_table_dtype("q8"), 0)
    blob, offsets, shapes = concat_inputs(case.inputs)
    need = op.plan.arena_bytes(shapes, case.symbols)
    arena = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    arena.fill_(0xFF)
    out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, case.symbols, arena=arena)
    torch.cuda.synchronize()
    launch = op.plan.last_launch()
    assert (launch["kernel"], launch["vec"], launch["rows_per_wave"], launch["wide_rows"]) == ("hybrid_tabq8", vec, 4, False), launch
    assert launch["dense_blocks"] > 1 and launch["ragged_blocks"] > 1, launch
    deq = Q.dequantize(case.table)
    want, bad = oracle.process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, [deq], case.symbols)
    assert bad == 0 and op.plan.read_bad_ids() == 0
    gather, pooled = _f32(out.groups[0]), _f32(out.groups[1])
    # the expectation holds NaN, both infinities, both zeros, subnormals and FLT_MAX
    w0 = want[0]
    assert np.isnan(w0).any() and (w0 == np.inf).any() and (w0 == -np.inf).any() and (w0.view(np.uint32) == 0x80000000).any()
    assert (np.abs(w0) == np.float32(Q.FLT_MAX)).any() and ((w0 != 0) & (np.abs(w0) < np.float32(2.0 ** -126))).any()
    n_nan = Q.assert_same_bits(gather, want[0], ("edge", vec, "gather"))
    assert n_nan == int(np.isnan(deq).sum()) > 0
    # a gather is a copy of the dequantised row
    Q.assert_same_bits(gather, deq[case.inputs[0]], ("edge", vec, "gather vs table"))
    assert Q.assert_same_bits(pooled, want[1], ("edge", vec, "pooled")) == n_nan
    assert not (pooled.view(np.uint32) == 0x80000000).any()          # +0.0 + -0.0 = +0.0
    assert bool((arena[need:] == 0xFF).all())
    del op


def _run_plan(torch, spec32, tables, requests, oracle, what, skip_cols=()):
    """A q8 plan against the oracle on the dequantised tables, request by request, in a NaN-poisoned arena.  Returns the
    op and the bad-id total.  `skip_cols`: EXTERNAL columns — not compared, and still 0xFF afterwards."""
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import LAYOUT_CONCAT
    dev = torch.device("cuda", 0)
    spec = spec32.with_table_dtype("q8")
    deq = [Q.dequantize(t) for t in tables]
    d_tabs = _dev_tables(torch, tables, dev)
    op = FeatureColumnProcess(spec, 0)
    twin = dataclasses.replace(spec32, layout=LAYOUT_CONCAT)
    offs = twin.column_offsets()
    bad_total = 0
    for t, (inputs, symbols) in enumerate(requests):
        blob, offsets, shapes = concat_inputs(inputs)
        need = max(op.plan.arena_bytes(shapes, symbols), 128)
        arena = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        arena.fill_(0xFF)
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, symbols, arena=arena)
        torch.cuda.synchronize()
        assert op.plan.last_launch()["kernel"].endswith("_tabq8"), op.plan.last_launch()
        want, bad = oracle.process_feature_columns(twin.to_dict(), blob, offsets, shapes, deq, symbols)
        for k, c in enumerate(spec.columns):
            w = want[c.concat_group][:, offs[k]:offs[k] + c.dim]
            if k in skip_cols:
                g = _f32(out.groups[c.concat_group])[:, offs[k]:offs[k] + c.dim]
                assert (g.view(np.uint32) == 0xFFFFFFFF).all(), (what, t, "EXTERNAL slot written", k)
                continue
            Q.assert_same_bits(_f32(out.column(k)), w, (what, t, "column", k))
        assert bool((arena[need:] == 0xFF).all()), (what, t, "bytes beyond the request's arena were written")
        bad_total += bad
        assert op.plan.read_bad_ids() == bad_total, (what, t)
    return op, bad_total


def test_copies_beside_q8_lookups(torch_cuda, oracle, monkeypatch):
    """GATHER_SCATTER with its row ids in any order, PASSTHROUGH, BATCH_COL_REDUCTION and an EXTERNAL slot beside q8 lookups
    (the blob payloads stay float32); out-of-vocabulary and negative ids read +0.0 rows and are counted, with the float32
    twin's counts; the same plan in FCP_LAYOUT_PER_COLUMN."""
    torch = torch_cuda
    from recom_amd.plan import LAYOUT_PER_COLUMN
    _no_wide_rows_diag(monkeypatch)
    m, spec = Q.mixed_spec()
    tables = [Q.draw_table(t.vocab, t.dim, 300 + i) for i, t in enumerate(m.tables)]
    requests = []
    for seed in (0, 1):
        req = m.make_request(seed)
        requests.append((Q.with_bad_ids(req.inputs, spec, seed) if seed else req.inputs, req.symbols))
    ext = [k for k, c in enumerate(spec.columns) if c.form == 6]
    assert len(ext) == 1 and {c.form for c in spec.columns} == {1, 2, 3, 4, 5, 6}
    op, bad = _run_plan(torch, spec, tables, requests, oracle, "mixed", skip_cols=ext)
    assert bad > 0
    del op
    _, spec_pc = Q.mixed_spec(layout=LAYOUT_PER_COLUMN)
    op, bad_pc = _run_plan(torch, spec_pc, tables, requests, oracle, "per_column")
    assert bad_pc == bad
    del op


def test_id_transforms_in_front_of_q8_lookups(torch_cuda, oracle, monkeypatch):
    """A filtered mean, a SELECT gather and a hashed sum."""
    _no_wide_rows_diag(monkeypatch)
    spec = Q.xform_spec()
    tables = [Q.draw_table(c.vocab, c.dim, 40 + k) for k, c in enumerate(spec.columns)]
    op, bad = _run_plan(torch_cuda, spec, tables, [Q.xform_request(29, 5), Q.xform_request(70, 6)], oracle, "xform")
    assert bad > 0
    del op


def test_wide_rows_are_decided_from_the_q8_stride(torch_cuda, monkeypatch):
    """One table of dim 1 and 480 000 000 rows (4.32 GB, uninitialised except the rows read): vocab * dim / V stays below
    2^32 - 3, vocab * (dim + 8) / V does not — the launch must report 64-bit row arithmetic with no FCP_DIAG asking for it,
    and rows 0, floor(2^32 / 9) - 1 .. + 1 and vocab - 1 must come out right."""
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    _no_wide_rows_diag(monkeypatch)
    assert "wide_rows" not in os.environ.get("FCP_DIAG", "")
    vocab, dim = Q.WIDE_VOCAB, Q.WIDE_DIM
    assert vocab * dim < 2 ** 32 - 3 <= vocab * (dim + 8)
    nbytes = vocab * (dim + 8)
    free, _total = torch.cuda.mem_get_info()
    if free < nbytes + (1 << 30):
        pytest.skip(f"needs {nbytes / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free")
    dev = torch.device("cuda", 0)
    table = torch.empty((vocab, dim + 8), dtype=torch.uint8, device=dev)
    rows = np.asarray(Q.WIDE_ROWS, np.int64)
    assert rows.max() == vocab - 1 and (rows[1:4] * 9 >= 2 ** 32 - 18).all()
    drawn = Q.draw_table(len(rows), dim, 77)
    table[torch.from_numpy(rows).to(dev)] = torch.from_numpy(drawn).to(dev)
    op = FeatureColumnProcess(Q.wide_rows_spec().with_table_dtype("q8"), 0)
    ids = np.concatenate([rows, [vocab, -1], rows[::-1]]).astype(np.int64)
    blob, offsets, shapes = concat_inputs([ids])
    need = op.plan.arena_bytes(shapes, None)
    arena = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    arena.fill_(0xFF)
    out = op(torch.from_numpy(blob).to(dev), offsets, shapes, [table], None, arena=arena)
    torch.cuda.synchronize()
    launch = op.plan.last_launch()
    assert (launch["kernel"], launch["vec"], launch["wide_rows"]) == ("dense_tabq8", 1, True), launch
    deq = Q.dequantize(drawn)
    want = np.concatenate([deq, np.zeros((2, dim), np.float32), deq[::-1]])
    assert Q.assert_same_bits(_f32(out.groups[0]), want, "wide rows") == 0
    assert op.plan.read_bad_ids() == 2
    assert bool((arena[need:] == 0xFF).all())
    del op, table
    torch.cuda.empty_cache()


def test_wrong_tables_are_refused_by_the_op(torch_cuda):
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec = Q.xform_spec()
    inputs, symbols = Q.xform_request()
    blob, offsets, shapes = concat_inputs(inputs)
    dev = torch.device("cuda", 0)
    d_blob = torch.from_numpy(blob).to(dev)
    f32 = [torch.zeros((c.vocab, c.dim), dtype=torch.float32, device=dev) for c in spec.columns]
    q8 = [torch.zeros((c.vocab, c.dim + 8), dtype=torch.uint8, device=dev) for c in spec.columns]
    op = FeatureColumnProcess(spec.with_table_dtype("q8"), 0)
    op(d_blob, offsets, shapes, q8, symbols)                                       # the right tables are taken
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="table"):                                 # another dtype
        op(d_blob, offsets, shapes, f32, symbols)
    with pytest.raises(ValueError, match=r"dim \+ 8"):                             # uint8 of the float32 table's shape
        op(d_blob, offsets, shapes, [torch.zeros((c.vocab, c.dim), dtype=torch.uint8, device=dev) for c in spec.columns], symbols)
    with pytest.raises(ValueError, match=r"dim \+ 8"):                             # a row short
        op(d_blob, offsets, shapes, [q8[0][:-1]] + q8[1:], symbols)
    with pytest.raises(ValueError, match=r"dim \+ 8"):                             # the right shape, not contiguous
        op(d_blob, offsets, shapes, [torch.zeros((spec.columns[0].dim + 8, spec.columns[0].vocab), dtype=torch.uint8, device=dev).t()] + q8[1:],
           symbols)
    for other in ("f32", "bf16", "f16"):                                            # uint8 tables for other plans
        op2 = FeatureColumnProcess(spec.with_table_dtype(other), 0)
        with pytest.raises(ValueError, match="table"):
            op2(d_blob, offsets, shapes, q8, symbols)


@pytest.mark.parametrize("kind", sorted(Q.refused_specs()))
def test_refused_q8_plan_reports_the_same_on_the_device(torch_cuda, monkeypatch, kind):
    """A refused plan: the same status and message from a device plan as from a host-only one."""
    from recom_amd import lib as _lib
    from recom_amd.ops import Plan
    from recom_amd.plan import FLAG_TABLES_BF16, FLAG_TABLES_Q8, PlanSpec
    spec, extra, word = Q.refused_specs()[kind]
    monkeypatch.setattr(PlanSpec, "validate_table_dtype", lambda self: None)      # past the Python mirror: the library decides
    monkeypatch.setattr(PlanSpec, "validate_out_dtype", lambda self: None)
    seen = []
    for host_only in (True, False):
        with pytest.raises(_lib.FcpError) as e:
            Plan(dataclasses.replace(spec, flags=FLAG_TABLES_Q8 | extra), 0, host_only=host_only)
        seen.append((e.value.status, str(e.value)))
    assert seen[0] == seen[1] and seen[0][0] == _lib.FCP_ERR_UNSUPPORTED and word in seen[0][1] and "8-bit tables" in seen[0][1], seen
    with pytest.raises(_lib.FcpError) as e:
        Plan(dataclasses.replace(Q.refused_specs()["sharded"][0], shard_world=1, shard_rank=0, flags=FLAG_TABLES_BF16 | FLAG_TABLES_Q8), 0)
    assert e.value.status == _lib.FCP_ERR_INVALID_ARGUMENT
