"""The nine kernels of fcp_kernels.hip outside the fused matrix, as explicit cells (tests/aux_kernel_cases.py): the
segment-offset pre-pass, fcp_shard_finalize_kernel<4/2/1>, fcp_concat_outputs_kernel<4/2/1>, the descriptor upload and
the stager's H2D copy.  Every cell first asserts the launch-counter deltas it expects (recom_amd.lib.aux_launch_counts: the
instantiation was reached, not assumed), then compares bit patterns with a NumPy restatement; outputs and scratch are
prefilled so that a skipped or stray store shows."""
import ctypes as C
import zlib

import numpy as np
import pytest

import aux_kernel_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture
def counts():
    from recom_amd import lib
    return lib.aux_launch_counts


def _dev_blob(torch, blob, dev):
    return torch.from_numpy(blob).to(dev) if blob.size else torch.empty(0, dtype=torch.int8, device=dev)


# ---- pre-pass ----------------------------------------------------------------------------------------------------------
PREPASS = A.prepass_cells()


def _prepass_plan(kind, rows_sym):
    from recom_amd.plan import FLAG_COUNT_BAD_IDS, PlanSpec
    seg_rank, seg_esz = {"ids_i32": (1, 4), "ids_i64": (1, 8)}.get(kind, (2, 8))
    col = A.prepass_column(kind, 0, 1, 0, 1)
    spec = PlanSpec([col], [1, seg_rank], [4, seg_esz], 1, n_groups=1, n_symbols=2 if rows_sym else 1,
                    flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    return spec


@pytest.mark.parametrize("cell", PREPASS, ids=[c.id for c in PREPASS])
def test_prepass_cell(oracle, counts, cell):
    """Raw CSR offsets of every entry 0..rows against np_segment_offsets of the mapped ids clamped to `rows`; scratch words
    outside the written range keep the 0xFF fill.  A row-sharded plan (world 2): the pre-pass runs (the finalize needs it)."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    rng = np.random.default_rng(zlib.crc32(cell.id.encode()))
    row_ids, rows = A.prepass_rows(cell, rng)
    seg = A.prepass_segment_input(cell.kind, row_ids, rng)
    mapped = A.mapped_rows(cell.kind, seg)
    assert np.array_equal(mapped, row_ids) and np.all(np.diff(mapped) >= 0), cell.id      # (the generator's own promise)
    ids = rng.integers(0, 50, cell.nnz).astype(np.int32)
    spec = _prepass_plan(cell.kind, cell.kind == "div_sym").with_shard(0, 2)
    symbols = np.asarray([rows, A.DIV_SYM] if cell.kind == "div_sym" else [rows], np.int32)
    dev = torch.device("cuda", 0)
    table = np.random.default_rng(1).standard_normal((50, 4)).astype(np.float32)
    tabs = [torch.from_numpy(np.ascontiguousarray(table[0::2])).to(dev)]
    op = FeatureColumnProcess(spec, 0)
    if cell.any_order:
        op.plan.set_inputs_ready(True)
    blob, offsets, shapes = concat_inputs([ids, seg])
    d_blob = _dev_blob(torch, blob, dev)
    nbytes = max(op.plan.arena_bytes(shapes, symbols), 128)
    arena = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev)
    before = counts()
    op(d_blob, offsets, shapes, tabs, symbols, arena=arena)
    torch.cuda.synchronize()
    assert A.counter_delta(before, counts()) == {"segment_offsets": 1}, cell.id
    assert op.plan.last_launch()["segment_offsets"] == "prepass"
    off, base = op.plan.last_csr()
    assert off >= 0 and base[0] >= 0 and off % 4 == 0
    words = arena.cpu().numpy().view(np.int32)
    got = words[off // 4 + base[0]: off // 4 + base[0] + rows + 1]
    want = A.raw_offsets(mapped, rows)
    assert np.array_equal(got, want), (cell.id, np.argwhere(got != want)[:4].tolist())
    rest = np.ones(words.size, bool)
    rest[:off // 4] = False                                        # the outputs
    rest[off // 4 + base[0]: off // 4 + base[0] + rows + 1] = False
    assert np.all(words[rest] == -1), (cell.id, "scratch outside the column's offsets was written")
    want_out, _ = oracle.process_feature_columns(spec.to_dict(), blob, offsets, shapes, [table[0::2]], symbols)
    got_out = words[:want_out[0].size].view(np.float32).reshape(want_out[0].shape)
    A.assert_bits_equal(got_out, want_out[0], cell.id)
    del op


def test_prepass_descending_step_is_counted(counts):
    """Segment ids that step down break the sorted contract: the pre-pass counts every such step as a bad id (the offsets
    are unspecified then)."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    spec = _prepass_plan("ids_i32", False).with_shard(1, 2)
    seg = np.asarray([0, 0, 3, 2, 5, 5, 1, 6] + [7] * 1100 + [6], np.int32)     # three steps down, one across a block
    ids = np.arange(seg.size, dtype=np.int32) % 50
    blob, offsets, shapes = concat_inputs([ids, seg])
    op = FeatureColumnProcess(spec, 0)
    tabs = [torch.zeros((25, 4), dtype=torch.float32, device=dev)]
    before = counts()
    op(torch.from_numpy(blob).to(dev), offsets, shapes, tabs, np.asarray([9], np.int32))
    torch.cuda.synchronize()
    assert A.counter_delta(before, counts()) == {"segment_offsets": 1}
    assert op.plan.read_bad_ids() == 3


@pytest.mark.parametrize("filtered", [False, True])
def test_prepass_scatter_inverse_map(oracle, counts, filtered):
    """Any-order ScatterNd row ids: inv[row] = 1 + the last position whose row id is `row` (of the ids the filter keeps), 0
    where none landed; rows outside [0, B) are counted as bad ids.  The result equals the oracle bit for bit."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import (COMBINER_NONE, FLAG_COUNT_BAD_IDS, FORM_GATHER_SCATTER, IDS_I32, ROWS_FROM_SYMBOL,
                                SEG_IDS_I32, XFORM_FILTER, ColumnSpec, PlanSpec)
    rng = np.random.default_rng(7 + filtered)
    B, nnz = 300, 2 * A.SEG_IDS_PER_BLOCK + 9
    xf = dict(xform_mode=XFORM_FILTER, xform_lo=(0,), xform_hi=(30,)) if filtered else {}
    col = ColumnSpec(FORM_GATHER_SCATTER, 4, 50, COMBINER_NONE, IDS_I32, 0, 0, 1, SEG_IDS_I32, 1, ROWS_FROM_SYMBOL, 0,
                     None, 0, 0, **xf)
    spec = PlanSpec([col], [1, 1], [4, 4], 1, n_groups=1, n_symbols=1, flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    rows = rng.integers(0, B, nnz).astype(np.int32)
    rows[rng.random(nnz) < 0.03] = -1
    rows[rng.random(nnz) < 0.03] = B + 4
    rows[10:20] = 17                                         # one row hit many times
    ids = rng.integers(0, 50, nnz).astype(np.int32)
    keep = (ids <= 30) if filtered else np.ones(nnz, bool)
    want_inv = np.zeros(B, np.int32)
    for i in range(nnz):
        if keep[i] and 0 <= rows[i] < B:
            want_inv[rows[i]] = i + 1
    stray = int(np.sum(keep & ((rows < 0) | (rows >= B))))
    dev = torch.device("cuda", 0)
    table = rng.standard_normal((50, 4)).astype(np.float32)
    table[3] = A.NEG0
    op = FeatureColumnProcess(spec, 0)
    blob, offsets, shapes = concat_inputs([ids, rows])
    symbols = np.asarray([B], np.int32)
    nbytes = max(op.plan.arena_bytes(shapes, symbols), 128)
    arena = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    before = counts()
    op(torch.from_numpy(blob).to(dev), offsets, shapes, [torch.from_numpy(table).to(dev)], symbols, arena=arena)
    torch.cuda.synchronize()
    assert A.counter_delta(before, counts()) == {"segment_offsets": 1}
    off, base = op.plan.last_csr()
    words = arena.cpu().numpy().view(np.int32)
    assert np.array_equal(words[off // 4 + base[0]: off // 4 + base[0] + B], want_inv)
    assert op.plan.read_bad_ids() == stray
    want, bad = oracle.process_feature_columns(spec.to_dict(), blob, offsets, shapes, [table], symbols)
    assert bad == stray
    A.assert_bits_equal(words[:want[0].size].view(np.float32).reshape(want[0].shape), want[0], "scatter output")


# ---- finalize ----------------------------------------------------------------------------------------------------------
FINALIZE = A.finalize_cells()


@pytest.mark.parametrize("cell", FINALIZE, ids=[c.id for c in FINALIZE])
def test_finalize_cell(oracle, counts, cell):
    """Every rank's partials (bit-exact against the sharded C oracle), a batch slice of them finalized into a prefilled
    output: pooled columns equal the NumPy float32 restatement (rank-order adds, division by the kept count), one-owner
    columns are bit-identical to the unsharded result (-0.0, NaN payloads and subnormals included), the EXTERNAL hole keeps
    its fill."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import COMBINER_MEAN, FORM_EXTERNAL, FORM_SEGMENT_REDUCE, SEG_CSR_I32
    import fcp_oracle
    rng = np.random.default_rng(cell.vec * 10 + cell.world)
    spec, roles = A.finalize_plan(cell.vec)
    tables = A.finalize_tables(spec, rng)
    B = A.FINALIZE_ROWS
    inputs, symbols = A.finalize_request(spec, roles, rng, B)
    blob, offsets, shapes = concat_inputs(inputs)
    dev = torch.device("cuda", 0)
    d_blob = torch.from_numpy(blob).to(dev)
    full, _ = oracle.process_feature_columns(spec.to_dict(), blob, offsets, shapes, tables, symbols)
    parts, ops, tabs = [], [], []
    for rank in range(cell.world):
        sspec = spec.with_shard(rank, cell.world)
        stabs = [np.ascontiguousarray(t[rank::cell.world]) for t in tables]
        d_tabs = [torch.from_numpy(t).to(dev) for t in stabs]
        op = FeatureColumnProcess(sspec, 0)
        out = op(d_blob, offsets, shapes, d_tabs, symbols)
        torch.cuda.synchronize()
        got = out.groups[0].cpu().numpy()
        want, _ = oracle.process_feature_columns(sspec.to_dict(), blob, offsets, shapes, stabs, symbols)
        ext = np.zeros(got.shape[1], bool)
        offs = spec.column_offsets()
        for k, c in enumerate(spec.columns):
            if c.form == FORM_EXTERNAL:
                ext[offs[k]:offs[k] + c.dim] = True
        A.assert_bits_equal(got[:, ~ext], want[0][:, ~ext], (cell.id, "partials of rank", rank))
        parts.append(out.groups[0].clone())
        ops.append(op)
        tabs.append(d_tabs)
    lo, cnt = cell.rows(B)
    sl = torch.stack([p[lo:lo + cnt] for p in parts]).contiguous()
    r = (lo + cnt) % cell.world                                   # any rank may finalize any slice
    fin = torch.full((cnt, spec.group_width(0)), float("nan"), dtype=torch.float32, device=dev)
    fin.view(torch.int32).fill_(int(A.SENTINEL.view(np.int32)))
    before = counts()
    ops[r].shard_finalize(d_blob, offsets, shapes, tabs[r], symbols, 0, sl, cell.world, lo, cnt, out=fin)
    torch.cuda.synchronize()
    assert A.counter_delta(before, counts()) == {f"shard_finalize_v{cell.vec}": 1,
                                                 "segment_offsets": 1}, cell.id   # (mean over segment ids: the pre-pass)
    got = fin.cpu().numpy()
    offs = spec.column_offsets()
    kept = {}
    ins = iter(range(len(inputs)))
    for k, c in enumerate(spec.columns):
        if c.form == FORM_SEGMENT_REDUCE and c.combiner == COMBINER_MEAN:
            ids, seg = inputs[c.ids_input], inputs[c.seg_input]
            o = seg if c.seg_kind == SEG_CSR_I32 else fcp_oracle.np_segment_offsets(seg, B)
            kept[k] = A.kept_counts(c, ids, np.asarray(o, np.int64))[lo:lo + cnt]
    restated = A.finalize_restated(spec, sl.cpu().numpy(), kept)
    for k, (c, role) in enumerate(zip(spec.columns, roles)):
        a = got[:, offs[k]:offs[k] + c.dim]
        what = (cell.id, role)
        if c.form == FORM_EXTERNAL:
            assert np.all(a.view(np.uint32) == A.SENTINEL), what
        elif c.form == FORM_SEGMENT_REDUCE:
            A.assert_bits_equal(a, restated[:, offs[k]:offs[k] + c.dim], what)
            ref = full[0][lo:lo + cnt, offs[k]:offs[k] + c.dim].astype(np.float64)
            assert np.all(np.abs(a - ref) <= 1e-5 * np.maximum(np.abs(ref), 1.0)), what
        else:
            A.assert_bits_equal(a, full[0][lo:lo + cnt, offs[k]:offs[k] + c.dim], what)
            A.assert_bits_equal(a, restated[:, offs[k]:offs[k] + c.dim], what)
    del ops


def test_finalize_of_an_unsharded_plan_does_not_divide(oracle, counts):
    """World 1: the plan's own kernels have divided; the finalize copies its one slice (one-owner columns bit for bit)."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    rng = np.random.default_rng(5)
    spec, roles = A.finalize_plan(2)
    tables = A.finalize_tables(spec, rng)
    inputs, symbols = A.finalize_request(spec, roles, rng, A.FINALIZE_ROWS)
    blob, offsets, shapes = concat_inputs(inputs)
    dev = torch.device("cuda", 0)
    d_blob = torch.from_numpy(blob).to(dev)
    d_tabs = [torch.from_numpy(t).to(dev) for t in tables]
    op = FeatureColumnProcess(spec, 0)
    out = op(d_blob, offsets, shapes, d_tabs, symbols)
    torch.cuda.synchronize()
    whole = out.groups[0].clone()
    fin = torch.empty_like(whole)
    fin.view(torch.int32).fill_(int(A.SENTINEL.view(np.int32)))
    before = counts()
    op.shard_finalize(d_blob, offsets, shapes, d_tabs, symbols, 0, whole[None].contiguous(), 1, 0, whole.shape[0], out=fin)
    torch.cuda.synchronize()
    assert A.counter_delta(before, counts()) == {"shard_finalize_v2": 1, "segment_offsets": 1}
    restated = A.finalize_restated(spec, whole[None].cpu().numpy(), {})
    got = fin.cpu().numpy()
    offs = spec.column_offsets()
    for k, (c, role) in enumerate(zip(spec.columns, roles)):
        sl = slice(offs[k], offs[k] + c.dim)
        if role == "external":
            assert np.all(got[:, sl].view(np.uint32) == A.SENTINEL)
        else:
            A.assert_bits_equal(got[:, sl], restated[:, sl], ("world 1", role))


# ---- concat ------------------------------------------------------------------------------------------------------------
CONCAT = A.concat_cells()


def _concat_layout(cell):
    """(dims, col offsets, input row strides, width, out float offset, input float offsets) of the cell."""
    dims = list(cell.dims)
    n = len(dims)
    a = 2 if cell.vec == 2 else 1
    if cell.entry in ("concat", "host_direct", "host_copied") and cell.cause in ("none", "chunks", "dim"):
        offs = list(np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(int))
        in_at = [0] * n
        if cell.cause == "chunks":
            in_at = [0 if i < A.CONCAT_CHUNK else (2 if i < 2 * A.CONCAT_CHUNK else 1) for i in range(n)]
        return dims, offs, list(dims), int(sum(dims)), 0, in_at
    offs = [0, 12, 20]
    width, out_at, in_at = 32, 0, [0] * n
    if cell.cause == "out_ptr":
        out_at = a
    elif cell.cause == "width":
        width = 32 + a
    elif cell.cause == "dim":
        dims[1] = 4 + a
    elif cell.cause == "offset":
        offs[1] = 12 + a
    strides = list(dims)
    if cell.cause == "stride":
        strides[1] = dims[1] + a
    elif cell.cause == "in_ptr":
        in_at[1] = a
    if cell.entry.startswith("host") and cell.cause == "offset":
        offs = [0, 256, 386]
        width = 390
    return dims, offs, strides, width, out_at, in_at


@pytest.mark.parametrize("cell", CONCAT, ids=[c.id for c in CONCAT])
def test_concat_cell(counts, cell):
    """Inputs with -0.0, +-inf, NaN payloads and subnormals; the output prefilled with a NaN sentinel: the copied elements
    bit for bit, every other element untouched."""
    import torch
    from recom_amd import lib
    L = lib.load()
    rng = np.random.default_rng(len(cell.id) * 131 + cell.prefix)
    dims, offs, strides, width, out_at, in_at = _concat_layout(cell)
    P = cell.prefix
    dev = torch.device("cuda", 0)
    xs = [A.special_values(rng, (P, s)) for s in strides]
    keep = []
    ptrs = []
    for x, at in zip(xs, in_at):
        t = torch.empty(x.size + 4, dtype=torch.float32, device=dev)
        t[at:at + x.size] = torch.from_numpy(x.reshape(-1)).to(dev)
        keep.append(t)
        ptrs.append(t.data_ptr() + 4 * at)
    want = np.full((P, width), A.SENTINEL, np.uint32).view(np.float32)
    for x, d, o in zip(xs, dims, offs):
        want[:, o:o + d] = x[:, :d]
    store = torch.empty(P * width + 4, dtype=torch.float32, device=dev)
    store.view(torch.int32).fill_(int(A.SENTINEL.view(np.int32)))
    out_ptr = store.data_ptr() + 4 * out_at
    n = len(dims)
    c_dims, c_offs, c_strides = (np.asarray(v, np.int32) for v in (dims, offs, strides))
    c_ptrs = (C.c_void_p * n)(*ptrs)
    stream = torch.cuda.current_stream(dev).cuda_stream
    before = counts()
    if cell.entry == "concat":
        lib.check(L.fcp_concat_outputs(c_ptrs, c_dims.ctypes.data, n, P, out_ptr, stream), "concat")
    elif cell.entry == "scatter":
        lib.check(L.fcp_concat_outputs_scatter(c_ptrs, c_dims.ctypes.data, c_offs.ctypes.data, n, P, width, out_ptr, stream),
                  "scatter")
    elif cell.entry == "strided":
        lib.check(L.fcp_concat_outputs_scatter_strided(c_ptrs, c_dims.ctypes.data, c_strides.ctypes.data, c_offs.ctypes.data,
                                                       n, P, width, out_ptr, stream), "strided")
    else:
        host = [np.ascontiguousarray(x[:, :d]) for x, d in zip(xs, dims)]
        h_ptrs = (C.c_void_p * n)(*[h.ctypes.data for h in host])
        temps = []

        def alloc(_ctx, nbytes):
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            temps.append(t)
            return t.data_ptr()
        cb = lib.ALLOC_FN(alloc)
        packed = sum((P * d * 4 + 15) // 16 * 16 for d in dims)
        assert (packed <= 1 << 20) == (cell.entry == "host_direct"), packed
        lib.check(L.fcp_concat_outputs_host(h_ptrs, c_dims.ctypes.data, c_offs.ctypes.data, n, P, width, out_ptr, cb, None,
                                            0, stream), "host")
        assert bool(temps) == (cell.entry == "host_copied")
    torch.cuda.synchronize()
    if cell.vec:
        want_counts = {f"concat_v{cell.vec}": 1}
    else:
        want_counts = {"concat_v4": 1, "concat_v2": 1}
        if n > 2 * A.CONCAT_CHUNK:
            want_counts["concat_v1"] = 1
    assert A.counter_delta(before, counts()) == want_counts, cell.id
    got = store.cpu().numpy()
    A.assert_bits_equal(got[out_at:out_at + P * width].reshape(P, width), want, cell.id)
    assert np.all(got[:out_at].view(np.uint32) == A.SENTINEL) and np.all(got[out_at + P * width:].view(np.uint32) == A.SENTINEL)


# ---- upload ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [341, 342, 1365, 1366])
def test_upload_kernel(monkeypatch, counts, n_cols):
    """FCP_DYN_UPLOAD=kernel (read at plan creation): the request's column records go up by fcp_upload_kernel — 1, 4 or 8
    blocks by the records' size.  Two requests of different shapes each install (one upload each) and equal the gathered
    table rows bit for bit; the first shape again is resident (no upload)."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import COMBINER_NONE, FORM_GATHER, IDS_I32, ROWS_FROM_IDS, SEG_NONE, ColumnSpec, PlanSpec
    monkeypatch.setenv("FCP_DYN_UPLOAD", "kernel")
    cols = [ColumnSpec(FORM_GATHER, 4, 61, COMBINER_NONE, IDS_I32, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, k)
            for k in range(n_cols)]
    spec = PlanSpec(cols, [1], [4], 1, n_groups=1, n_symbols=0)
    spec.validate()
    dev = torch.device("cuda", 0)
    table = A.special_values(np.random.default_rng(n_cols), (61, 4))
    tabs = [torch.from_numpy(table).to(dev)]
    op = FeatureColumnProcess(spec, 0)
    monkeypatch.delenv("FCP_DYN_UPLOAD")
    for t, (B, uploads) in enumerate(((5, 1), (67, 1), (5, 0))):
        ids = np.random.default_rng(t).integers(0, 61, B).astype(np.int32)
        blob, offsets, shapes = concat_inputs([ids])
        before = counts()
        out = op(torch.from_numpy(blob).to(dev), offsets, shapes, tabs)
        torch.cuda.synchronize()
        assert A.counter_delta(before, counts()) == ({"upload": 1} if uploads else {}), (n_cols, t)
        A.assert_bits_equal(out.groups[0].cpu().numpy(), np.tile(table[ids], (1, n_cols)), (n_cols, t))


# ---- h2d copy ----------------------------------------------------------------------------------------------------------
def test_h2d_copy_through_the_stager(monkeypatch, counts):
    """The stager ships each request in 16 groups (FCP_STAGER_GROUPS, FCP_DIAG=stager_groups_always) by the copy kernel:
    group boundaries at every byte residue, requests of 4..60 bytes and one of more than 1 MiB + 12 (several rounds of the
    64-block grid).  The staged device bytes equal the host packing byte for byte."""
    import torch
    from recom_amd.ops import RequestStager, concat_inputs
    monkeypatch.setenv("FCP_DIAG", "stager_groups_always")
    monkeypatch.setenv("FCP_STAGER_GROUPS", "16")
    st = RequestStager(3 << 20, 64, 64, depth=2, n_threads=8, copy="kernel")
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(3)
    sizes = [[n] for n in range(4, 61, 4)] + [[1 + r, 16 + s] for r in range(16) for s in range(0, 16, 5)]
    sizes += [[(1 << 20) + 12], [700000, 13, 400001], [(1 << 21) + 5 * 16 + 3]]
    try:
        for parts in sizes:
            inputs = [rng.integers(-128, 128, n).astype(np.int8) for n in parts]
            blob, _, _ = concat_inputs(inputs)
            before = counts()
            d_ptr, nbytes, _, _ = st.stage(inputs)
            torch.cuda.synchronize()
            delta = A.counter_delta(before, counts())
            assert set(delta) == {"h2d_copy"} and delta["h2d_copy"] >= 1, (parts, delta)
            tmp = torch.empty(nbytes, dtype=torch.int8, device="cuda")
            assert hip.hipMemcpy(C.c_void_p(tmp.data_ptr()), C.c_void_p(d_ptr), C.c_size_t(nbytes), 3) == 0
            got = tmp.cpu().numpy()
            assert nbytes == blob.size and np.array_equal(got, blob), parts
    finally:
        st.close()
