"""fcp_plan_traffic_count on the GPU (recom_amd/csrc/fcp_table_traffic.hip, fcp_process.hip): the rows a request reads, counted
through the plan's own id path, against the NumPy restatement of tests/plan_traffic_cases.py — exactly, integers — and, with
no restatement in between, against the plan's own output over identity tables.  Smallest shapes at which the kernel can go
wrong: id streams around one tile of PT.TILE positions, rows that share a home slot of the block's PT.CELLS-cell table.

The module's name puts it behind tests/test_z_gpu_private_streams.py in the suite's (alphabetical) order, on purpose: that
module's supervisor tests time event-linked streams with verification switched off, and what such streams cost depends on
what the process did to the device before — with these tests in front of it, in the whole suite,
test_supervisor_re_admits_a_demoted_caller_when_the_private_streams_win_again measured the private streams 8 to 10 times
slower than stream order where it needs them below 3 (it passes with these tests alone in front of it, and with the suite
without them).  Nothing here uses private streams, so the order costs these tests nothing."""
import dataclasses

import numpy as np
import pytest

import plan_traffic_cases as PT

pytestmark = pytest.mark.gpu
GUARD = 64           # cells on either side of every count array that nothing may touch


@pytest.fixture(scope="module")
def torch_cuda():
    import gc
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()
    yield torch
    # whatever this module's tests dropped (ops, tensors, callbacks) goes now, not in the middle of a later module
    gc.collect()
    torch.cuda.synchronize()


_LIVE = []           # the plans of the running test


@pytest.fixture(autouse=True)
def plans_destroyed_with_their_test(torch_cuda):
    """A plan's destructor synchronises the device.  Left to the garbage collector it would run in the middle of some later
    test — the timing windows of tests/test_z_gpu_private_streams.py among them — so every plan made here is closed here."""
    yield
    torch_cuda.cuda.synchronize()
    while _LIVE:
        _LIVE.pop().close()


class Counted:
    """a plan with guarded count arrays bound to it"""

    def __init__(self, torch, spec, count=None, with_skipped=True, plan=None):
        from recom_amd.ops import Plan
        self.torch, self.spec = torch, spec
        self.plan = plan if plan is not None else Plan(spec, 0)
        _LIVE.append(self.plan)
        self.rows = self.plan.table_rows()
        assert list(self.rows) == PT.table_rows(spec)
        self.bind(count, with_skipped)

    def bind(self, count=None, with_skipped=True):
        torch = self.torch
        dt = getattr(torch, "uint32", torch.int32)
        self.bufs = [None if r < 0 else torch.zeros((r + 2 * GUARD,), dtype=dt, device="cuda:0") for r in self.rows]
        self.counted = [r >= 0 and (count is None or t in count) for t, r in enumerate(self.rows)]
        self.counts = [b[GUARD:GUARD + r] if on else None for b, r, on in zip(self.bufs, self.rows, self.counted)]
        self.skipped = torch.zeros((1,), dtype=torch.int64, device="cuda:0") if with_skipped else None
        self.plan.traffic_bind(self.counts, self.skipped)

    def count(self, inputs, symbols=None, stream=None):
        from recom_amd.ops import concat_inputs
        torch = self.torch
        blob, offsets, shapes = concat_inputs(list(inputs))
        d_blob = torch.from_numpy(blob).to("cuda:0") if blob.size else torch.empty(0, dtype=torch.int8, device="cuda:0")
        self.plan.traffic_count(d_blob, offsets, shapes, symbols, stream)
        return d_blob

    def read(self):
        """(list of uint32 arrays or None, skipped or None); asserts that every guard cell, and every cell of an uncounted
        table's would-be array, is still zero"""
        self.torch.cuda.synchronize()
        out = []
        for b, r, on in zip(self.bufs, self.rows, self.counted):
            if b is None:
                out.append(None)
                continue
            a = b.cpu().numpy().view(np.uint32)
            assert not a[:GUARD].any() and not a[GUARD + r:].any(), "a guard cell was written"
            if not on:
                assert not a.any(), "an uncounted table's memory was written"
            out.append(a[GUARD:GUARD + r].copy() if on else None)
        return out, None if self.skipped is None else int(self.skipped.item())


def assert_counts(got, want):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), t
        if g is not None:
            assert g.dtype == np.uint32 and np.array_equal(g, w), (t, np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])


# ---- the matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5, 21, 65])
def test_matrix_of_forms_id_sources_segment_encodings_and_transforms(torch_cuda, batch):
    """synth.model_mixed with test_oracle's XFORMS: the three lookup forms, int32 / int64 / bucketized ids, CSR / row-id /
    SparseTensor-index segments, SELECT / FILTER / hash.  Counts and skipped equal the restatement exactly; request 0 of every
    batch has ids outside their vocab and filtered ids (asserted on the NumPy side)."""
    from recom_amd import synth
    from test_oracle import XFORMS, _xform_spec
    m = synth.model_mixed(batch=batch, vocab=997)
    spec = _xform_spec(m, XFORMS)
    req = m.make_request(0)
    want, skipped = PT.expected_counts(spec, req.inputs, req.symbols)
    filtered = sum(PT.n_filtered(c, req.inputs) for c in spec.columns if c.form in PT.LOOKUP_FORMS)
    assert skipped > 0 and filtered > 0
    forms = {c.form for c in spec.columns}
    assert set(PT.LOOKUP_FORMS) <= forms and {c.id_source for c in spec.columns if c.form in PT.LOOKUP_FORMS} == {PT.IDS_I32, PT.IDS_I64, PT.IDS_F32_BUCKETIZE}
    cp = Counted(torch_cuda, spec)
    cp.count(req.inputs, req.symbols)
    got, got_skipped = cp.read()
    assert_counts(got, want)
    assert got_skipped == skipped


# ---- no restatement in between --------------------------------------------------------------------------------------------
def _identity_plan():
    """GATHER columns over tables whose row r is [r + 1] * dim: the plan's own output names the row every lookup read (0: an
    id outside the vocab read as zeros).  Three bucketize tiers (reproducible boundaries, evenly spaced ones, uneven ones),
    hashed ids, SELECT with a substitute inside and one outside the vocab, plain int32 / int64 ids."""
    even = np.arange(0.0, 500.0, 5.0, dtype=np.float32)                      # fma(i, 5, 0) bit for bit: computed, never read
    near = (np.arange(100, dtype=np.float64) * 4.999 + 0.01 * np.sin(np.arange(100))).astype(np.float32)   # guess and verify
    uneven = (np.arange(60, dtype=np.float32) ** 2 / 7.0).astype(np.float32)                               # binary search
    cols = [PT.gather_col(0, 101, 0, PT.IDS_F32_BUCKETIZE, boundaries=even),
            PT.gather_col(1, 101, 1, PT.IDS_F32_BUCKETIZE, boundaries=near),
            PT.gather_col(2, 50, 2, PT.IDS_F32_BUCKETIZE, boundaries=uneven),          # (buckets 50..60 lie outside the vocab)
            PT.gather_col(3, 640, 3, hash_buckets=640),
            PT.gather_col(4, 300, 4, xform_mode=PT.XFORM_SELECT, xform_lo=(10, 200), xform_hi=(99, 250), xform_substitute=7),
            PT.gather_col(5, 300, 5, PT.IDS_I32, xform_mode=PT.XFORM_SELECT, xform_lo=(0,), xform_hi=(150,), xform_substitute=300),
            PT.gather_col(6, 1 << 20, 6), PT.gather_col(7, 33, 7, PT.IDS_I32)]
    return PT.gather_spec(cols, 8)


@pytest.mark.parametrize("batch", [3, 700])
def test_counts_equal_the_bincount_of_the_plan_s_own_output(torch_cuda, batch):
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    torch = torch_cuda
    spec = _identity_plan()
    rng = np.random.default_rng(batch)
    inputs = [rng.uniform(-20, 520, batch).astype(np.float32), rng.uniform(-20, 520, batch).astype(np.float32),
              rng.uniform(-5, 600, batch).astype(np.float32), rng.integers(-2 ** 62, 2 ** 62, batch, dtype=np.int64),
              rng.integers(-50, 350, batch, dtype=np.int64), rng.integers(-50, 350, batch).astype(np.int32),
              rng.integers(-3, (1 << 20) + 3, batch, dtype=np.int64), rng.integers(-2, 35, batch).astype(np.int32)]
    tables = [torch.arange(1, c.vocab + 1, dtype=torch.float32, device="cuda:0").reshape(-1, 1).repeat(1, c.dim).contiguous()
              for c in spec.columns]
    op = FeatureColumnProcess(spec, 0)
    cp = Counted(torch, spec, plan=op.plan)
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to("cuda:0")
    op.traffic_count(d_blob, offsets, shapes, tables)
    out = op(d_blob, offsets, shapes, tables)
    got, skipped = cp.read()
    group = out.groups[0].cpu().numpy()
    offs = spec.column_offsets()
    zeros = 0
    for k, c in enumerate(spec.columns):
        v = group[:, offs[k]]
        assert np.array_equal(v, np.rint(v)) and v.min() >= 0 and v.max() <= c.vocab
        rows = v.astype(np.int64) - 1                                # -1: a row of zeros, an id outside the vocab
        zeros += int((rows < 0).sum())
        assert np.array_equal(got[k], np.bincount(rows[rows >= 0], minlength=c.vocab).astype(np.uint32)), k
    assert skipped == zeros and zeros > 0
    assert_counts(got, PT.expected_counts(spec, inputs)[0])         # (and the restatement agrees with both)


def test_sum_of_pooled_outputs_over_all_ones_tables_equals_the_sum_of_counts(torch_cuda):
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    torch = torch_cuda
    spec = PT.bag_spec(3, 211, [0, 1, 1])
    cols = list(spec.columns)
    cols[2] = dataclasses.replace(cols[2], xform_mode=PT.XFORM_FILTER, xform_lo=(20,), xform_hi=(180,))
    spec = PT.with_replaced(spec, columns=cols)
    rng = np.random.default_rng(5)
    rows = 9
    inputs = PT.bag_inputs([rng.integers(-3, 215, n) for n in (40, 1500, 333)], rows)
    sym = np.asarray([rows], np.int32)
    tables = [torch.ones((211, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    op = FeatureColumnProcess(spec, 0)
    cp = Counted(torch, spec, plan=op.plan)
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to("cuda:0")
    op.traffic_count(d_blob, offsets, shapes, tables, sym)
    out = op(d_blob, offsets, shapes, tables, sym)
    got, skipped = cp.read()
    group = out.groups[0].cpu().numpy().astype(np.float64)
    offs = spec.column_offsets()
    assert group[:, offs[0]].sum() == got[0].sum()
    assert group[:, offs[1]].sum() + group[:, offs[2]].sum() == got[1].sum()
    assert skipped > 0 and PT.n_filtered(spec.columns[2], inputs) > 0
    assert_counts(got, PT.expected_counts(spec, inputs, sym)[0])


# ---- edges of the tiling ---------------------------------------------------------------------------------------------------
def test_id_streams_around_a_tile_beside_each_other(torch_cuda):
    """nnz 0, 1, TILE - 1, TILE, TILE + 1, 2 TILE + 3 in one request: the grid's second dimension follows the longest stream,
    the blocks of the others past their nnz leave early (the empty column next to the longest one has nothing but such)."""
    lens = (2 * PT.TILE + 3, 0, 1, PT.TILE - 1, PT.TILE, PT.TILE + 1)
    spec = PT.bag_spec(len(lens), 3001, list(range(len(lens))))
    rng = np.random.default_rng(11)
    rows = 5
    inputs = PT.bag_inputs([rng.integers(-1, 3002, n) for n in lens], rows)
    sym = np.asarray([rows], np.int32)
    want, skipped = PT.expected_counts(spec, inputs, sym)
    assert [int(w.sum()) for w in want] != [0] * len(lens) and int(want[1].sum()) == 0
    cp = Counted(torch_cuda, spec)
    cp.count(inputs, sym)
    got, got_skipped = cp.read()
    assert_counts(got, want)
    assert got_skipped == skipped and sum(int(g.sum()) for g in got) + skipped == sum(lens)


def test_an_empty_request_launches_nothing(torch_cuda):
    spec = PT.gather_spec([PT.gather_col(0, 17, 0), PT.gather_col(1, 17, 1, PT.IDS_I32)], 2)
    cp = Counted(torch_cuda, spec)
    cp.plan.traffic_count(None, [0, 0], [0, 0], None)            # 0 rows: no blob either
    cp.count([np.zeros(0, np.int64), np.zeros(0, np.int32)])
    got, skipped = cp.read()
    assert skipped == 0 and not any(g.any() for g in got)


# ---- aggregation ------------------------------------------------------------------------------------------------------------
def test_aggregation_in_the_block_s_table(torch_cuda):
    """all ids equal: one cell = nnz; more distinct rows with ONE home slot than a row probes cells (r, r + CELLS, ...): some
    go to memory directly; two columns on two tables given the SAME row ids: neither array receives the other's reads; three
    columns on one shared table: their sum."""
    vocab = 9 * PT.CELLS + 5
    n = PT.TILE + 77
    rng = np.random.default_rng(3)
    equal = np.full(n, 1234, np.int64)
    colliding = 7 + PT.CELLS * rng.integers(0, 2 * PT.PROBES + 1, n, dtype=np.int64)
    same = rng.integers(0, vocab, n, dtype=np.int64)
    shared = [rng.integers(0, 40, n, dtype=np.int64) for _ in range(3)]
    spec = PT.bag_spec(7, vocab, [0, 1, 2, 3, 4, 4, 4])
    rows = 3
    inputs = PT.bag_inputs([equal, colliding, same, same] + shared, rows)
    sym = np.asarray([rows], np.int32)
    assert len(np.unique(colliding)) == 2 * PT.PROBES + 1 and len(np.unique(colliding % PT.CELLS)) == 1
    cp = Counted(torch_cuda, spec)
    cp.count(inputs, sym)
    got, skipped = cp.read()
    assert skipped == 0
    assert got[0][1234] == n and int(got[0].sum()) == n
    assert np.array_equal(got[1], np.bincount(colliding, minlength=vocab).astype(np.uint32))
    assert np.array_equal(got[2], got[3]) and int(got[2].sum()) == n and np.array_equal(got[2], np.bincount(same, minlength=vocab))
    assert np.array_equal(got[4], sum(np.bincount(s, minlength=vocab) for s in shared)) and int(got[4].sum()) == 3 * n
    assert_counts(got, PT.expected_counts(spec, inputs, sym)[0])


# ---- id extremes ------------------------------------------------------------------------------------------------------------
def test_id_extremes(torch_cuda):
    vocab = 100
    lo = PT.INT64_MIN
    cols = [PT.gather_col(0, vocab, 0),                                                     # int64 ids as they come
            PT.gather_col(1, vocab, 1, PT.IDS_I32),                                         # int32: -1 widens with its sign
            PT.gather_col(2, vocab, 2, xform_mode=PT.XFORM_SELECT, xform_lo=(0,), xform_hi=(9,), xform_substitute=42),     # inside
            PT.gather_col(3, vocab, 3, xform_mode=PT.XFORM_SELECT, xform_lo=(0,), xform_hi=(9,), xform_substitute=vocab),  # outside
            PT.gather_col(4, vocab, 4, xform_mode=PT.XFORM_FILTER, xform_lo=(lo, 5), xform_hi=(lo, 6))]  # keeps INT64_MIN: bad
    spec = PT.gather_spec(cols, 5)
    inputs = [np.asarray([-1, vocab, 2 ** 32 + 1, lo, vocab - 1], np.int64), np.asarray([-1, 0, vocab - 1, -2 ** 31, 2 ** 31 - 1], np.int32),
              np.asarray([3, 50, -1, lo, 9], np.int64), np.asarray([3, 50, -1, lo, 9], np.int64), np.asarray([lo, 5, 7, lo, 6], np.int64)]
    cp = Counted(torch_cuda, spec)
    cp.count(inputs)
    got, skipped = cp.read()
    assert got[0].nonzero()[0].tolist() == [vocab - 1] and got[0][vocab - 1] == 1
    assert got[1].nonzero()[0].tolist() == [0, vocab - 1]
    assert got[2][3] == 1 and got[2][9] == 1 and got[2][42] == 3 and int(got[2].sum()) == 5
    assert got[3][3] == 1 and got[3][9] == 1 and int(got[3].sum()) == 2
    assert got[4][5] == 1 and got[4][6] == 1 and int(got[4].sum()) == 2          # 7 is filtered, INT64_MIN twice skipped
    assert skipped == 4 + 3 + 0 + 3 + 2
    want, want_skipped = PT.expected_counts(spec, inputs)
    assert_counts(got, want)
    assert want_skipped == skipped


# ---- accumulation and isolation --------------------------------------------------------------------------------------------
def test_accumulation_isolation_rebind_and_unbind(torch_cuda):
    from recom_amd import lib
    from recom_amd.plan import FLAG_COUNT_BAD_IDS
    torch = torch_cuda
    spec = PT.bag_spec(3, 500, [0, 1, 2])
    spec = PT.with_replaced(spec, flags=spec.flags | FLAG_COUNT_BAD_IDS)
    rng = np.random.default_rng(21)
    req_a = (PT.bag_inputs([rng.integers(-2, 502, n) for n in (30, 1100, 7)], 4), np.asarray([4], np.int32))
    req_b = (PT.bag_inputs([rng.integers(-2, 502, n) for n in (900, 3, 64)], 6), np.asarray([6], np.int32))
    cp = Counted(torch, spec, count={0, 2})                 # table 1: NULL — its would-be memory is watched by read()
    bad_before = cp.plan.read_bad_ids()
    cp.count(*req_a)
    cp.count(*req_b)                                         # two calls of different shapes into the same arrays add
    got, skipped = cp.read()
    first, s1 = PT.expected_counts(spec, *req_a)
    both, s2 = PT.expected_counts(spec, *req_b, start=first)
    assert got[1] is None
    assert_counts([got[0], got[2]], [both[0], both[2]])
    # skipped counts the ids outside the vocab of the COUNTED columns only: an uncounted table's column is not walked
    only = [c for k, c in enumerate(spec.columns) if k != 1]
    want_skipped = sum(int((PT.lookup_ids(c, inp).view(np.uint64) >= np.uint64(c.vocab)).sum()) for inp, _s in (req_a, req_b) for c in only)
    assert skipped == want_skipped and 0 < skipped < s1 + s2
    assert cp.plan.read_bad_ids() == bad_before == 0        # the plan's own counter is never touched
    # skipped = NULL is accepted; rebinding moves the counting to other arrays and leaves the old ones as they are
    old = list(cp.bufs)
    snapshot = [b.cpu().numpy().copy() for b in old]
    cp.bind(count=None, with_skipped=False)
    cp.count(*req_a)
    got, skipped = cp.read()
    assert skipped is None
    assert_counts(got, first)
    assert all(np.array_equal(b.cpu().numpy(), s) for b, s in zip(old, snapshot))
    assert np.array_equal(snapshot[0].view(np.uint32)[GUARD:GUARD + 500], both[0])
    # unbind: a count is refused, nothing is written
    cp.plan.traffic_bind(None)
    with pytest.raises(lib.FcpError, match="fcp_plan_traffic_bind") as e:
        cp.count(*req_a)
    assert e.value.status == lib.FCP_ERR_INVALID_ARGUMENT
    assert_counts(cp.read()[0], first)
    # shape errors are the request path's own
    cp.bind()
    bad_shapes = list(req_a[0])
    bad_shapes[1] = bad_shapes[1][:-1]                       # CSR offsets with rows entries instead of rows + 1
    with pytest.raises(lib.FcpError, match="CSR offsets must have rows\\+1 entries") as e:
        cp.count(bad_shapes, req_a[1])
    assert e.value.status == lib.FCP_ERR_SHAPE_MISMATCH


# ---- serving is not disturbed ------------------------------------------------------------------------------------------------
def _serve(torch, m, spec, reqs, counted: bool):
    """process(A), [count(A), count(B),] process(A), process(B) on one stream; the outputs of the last two requests"""
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    op = FeatureColumnProcess(spec, 0)
    _LIVE.append(op.plan)
    tabs = m.torch_tables("cuda:0")
    packed = []
    for r in reqs:
        blob, offsets, shapes = concat_inputs(r.inputs)
        packed.append((torch.from_numpy(blob).to("cuda:0"), offsets, shapes, r.symbols))
    cp = Counted(torch, spec, plan=op.plan) if counted else None
    (ba, oa, sa, ya), (bb, ob, sb, yb) = packed
    if counted:
        op.traffic_count(bb, ob, sb, None, yb)              # before anything was served, before any table is bound
    op(ba, oa, sa, tabs, ya)
    if counted:
        op.traffic_count(ba, oa, sa, tabs, ya)
        op.traffic_count(bb, ob, sb, tabs, yb)
    out_a = op(ba, oa, sa, tabs, ya)
    out_b = op(bb, ob, sb, tabs, yb)
    torch.cuda.synchronize()
    res = [[g.cpu().numpy().copy() for g in o.groups] for o in (out_a, out_b)]
    return res, cp


@pytest.mark.parametrize("model", ["mixed", "plain_dense"])
def test_counts_do_not_disturb_serving(torch_cuda, model):
    """`plain_dense`: a plan whose requests take the plain dense kernel — its descriptor slot carries table addresses, and here
    a count installs the slot of request B before any table is bound."""
    from recom_amd import synth
    m = synth.model_mixed(batch=21, vocab=997) if model == "mixed" else synth.model_s2(columns=12, vocab=900, batch=80)
    reqs = [m.make_request(0), m.make_request(1, 33) if model == "mixed" else m.make_request(1, 96)]
    plain, _none = _serve(torch_cuda, m, m.spec, reqs, False)
    counted, cp = _serve(torch_cuda, m, m.spec, reqs, True)
    for a, b in zip(plain, counted):
        assert len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    got, skipped = cp.read()
    first, s1 = PT.expected_counts(m.spec, reqs[1].inputs, reqs[1].symbols)
    second, s2 = PT.expected_counts(m.spec, reqs[0].inputs, reqs[0].symbols, start=first)
    third, s3 = PT.expected_counts(m.spec, reqs[1].inputs, reqs[1].symbols, start=second)
    assert_counts(got, third)
    assert skipped == s1 + s2 + s3
    if model == "plain_dense":
        assert cp.plan.last_dense_front() == "plain"


# ---- every plan kind ---------------------------------------------------------------------------------------------------------
def _weighted_pair():
    """a plan with per-id weights and the sqrtn combiner, and its float32 unweighted twin on the same id inputs"""
    from recom_amd.plan import COMBINER_SQRTN
    twin = PT.bag_spec(2, 300, [0, 1])
    cols = [dataclasses.replace(twin.columns[0], weights_input=4), dataclasses.replace(twin.columns[1], combiner=COMBINER_SQRTN)]
    weighted = PT.with_replaced(twin, columns=cols, host_input_ranks=[1] * 5, host_input_elem_sizes=[8, 4, 8, 4, 4])
    return weighted, twin


@pytest.mark.parametrize("kind", ["weighted", "narrow", "q8", "mixed", "shard0", "shard1"])
def test_every_plan_kind_counts_what_its_float32_unsharded_twin_counts(torch_cuda, kind):
    from recom_amd import synth
    torch = torch_cuda
    if kind == "weighted":
        spec, twin = _weighted_pair()
        rng = np.random.default_rng(8)
        inputs = PT.bag_inputs([rng.integers(-2, 303, n) for n in (1200, 50)], 7)
        sym = np.asarray([7], np.int32)
        weights = rng.normal(0, 1, 1200).astype(np.float32)
        weights[::3] = 0.0                                       # a weight of 0 counts
        reqs = {"twin": (inputs, sym), "kind": (inputs + [weights], sym)}
    else:
        from test_oracle import XFORMS, _xform_spec
        m = synth.model_mixed(batch=21, vocab=997)
        twin = _xform_spec(m, XFORMS)
        read = set(twin.read_inputs())
        cycle = ("f32", "bf16", "f16", "q8")
        spec = {"narrow": lambda: twin.with_out_dtype("bf16"), "q8": lambda: twin.with_table_dtype("q8"),
                "mixed": lambda: twin.with_table_dtypes(tuple(cycle[t % 4] if t in read else "-" for t in range(twin.n_device_inputs))),
                "shard0": lambda: twin.with_shard(0, 2), "shard1": lambda: twin.with_shard(1, 2)}[kind]()
        spec.validate()
        r = m.make_request(0)
        reqs = {"twin": (r.inputs, r.symbols), "kind": (r.inputs, r.symbols)}
    want, want_skipped = PT.expected_counts(twin, *reqs["twin"])
    assert want_skipped > 0
    results = []
    for s, key in ((twin, "twin"), (spec, "kind")):
        cp = Counted(torch, s)
        cp.count(*reqs[key])
        results.append(cp.read())
    for got, skipped in results:
        assert_counts(got, want)
        assert skipped == want_skipped


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_counts_feed_the_weighted_audit(torch_cuda):
    """traffic_count -> tables.audit_tables(row_counts=) is byte-identical to the audit weighed by tables.count_ids on the
    NumPy-transformed ids, column by column — the composition a caller had to write before."""
    from recom_amd import synth, tables
    from test_oracle import XFORMS, _xform_spec
    torch = torch_cuda
    m = synth.model_mixed(batch=33, vocab=997)
    spec = _xform_spec(m, XFORMS)
    tabs = m.torch_tables("cuda:0")
    req = m.make_request(2)
    counts = tables.new_plan_counts(spec, "cuda:0")
    from recom_amd.ops import Plan
    plan = Plan(spec, 0)
    _LIVE.append(plan)
    assert [None if c is None else c.shape[0] for c in counts] == [None if r < 0 else r for r in plan.table_rows()]
    plan.traffic_bind(counts)
    cp = Counted.__new__(Counted)
    cp.torch, cp.plan = torch, plan
    Counted.count(cp, req.inputs, req.symbols)
    by_hand = tables.new_plan_counts(plan, "cuda:0")
    for c in spec.columns:
        if c.form in PT.LOOKUP_FORMS:
            tables.count_ids(by_hand[c.table_input][:c.vocab], torch.from_numpy(PT.lookup_ids(c, req.inputs)).to("cuda:0"))
    torch.cuda.synchronize()
    assert all((a is None and b is None) or np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(counts, by_hand))
    assert sum(int(a.cpu().numpy().view(np.uint32).sum()) for a in counts if a is not None) > 0
    got = tables.audit_tables(spec, tabs, row_counts=counts)
    want = tables.audit_tables(spec, tabs, row_counts=by_hand)
    assert len(got) == len(want) == spec.n_device_inputs
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g == w and bytes(g.raw) == bytes(w.raw) and g.sum_sq > 0
