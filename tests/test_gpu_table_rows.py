"""fcp_table_update_rows / fcp_table_read_rows on the GPU (kernels: recom_amd/csrc/fcp_table_rows.hip).  Every expectation is
computed on the CPU — by the restatements tests/test_table_convert_host.py pins to quantized::embedding_bag_byte_prepack, by
synth.dequantize_q8, narrow_output_cases.narrow and table16_cases.widen — or by the existing plans and fcp_table_convert, and
compared as bytes; nothing has a tolerance (NaN counts as equal to NaN only where T16.assert_same_bits does).  The calls on a
non-default stream and the pinned-buffer loader: tests/test_zzz_gpu_table_rows_stream.py."""
import numpy as np
import pytest

import narrow_output_cases as N
import table16_cases as T16
import table_convert_cases as TC
import table_rows_cases as R
from recom_amd import synth

pytestmark = pytest.mark.gpu

STREAM_DIMS = (1, 2, 3, 4, 6, 12, 64, 260)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))      # (a copy: the cases' arrays are read-only)


def _bytes(torch, t) -> np.ndarray:
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _update_cells(torch, kind, dim, x, want):
    """Every n of TC.QUANT_ROWS: rows x[:n] at n distinct ids of a poisoned table of n + 37 rows."""
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    src = _dev(torch, x)
    for n in TC.QUANT_ROWS:
        table_rows = n + R.SLACK_ROWS
        ids = R.distinct_ids(n, table_rows, 1000 * dim + n)
        assert len(set(ids.tolist())) == n                       # pairwise distinct: the entry's contract
        buf, table = R.poisoned(torch, kind, dim, table_rows, dev)
        assert tables.update_rows(table, _dev(torch, ids), src[:n]) is table
        R.check_poisoned(buf, kind, dim, table_rows, ids, want[:n], (kind, dim, n))


@pytest.mark.parametrize("dim", TC.QUANT_DIMS, ids=[f"dim{d}-V{TC.vec_of(d)}-G{TC.group_of(d)}" for d in TC.QUANT_DIMS])
def test_update_cells_q8(torch_cuda, dim):
    """float32 -> q8 by id at one dim, for every row count of TC.QUANT_ROWS: the rows at the ids are the restatement's
    bytes, every other byte of the table and of the three rows behind it is still the poison."""
    _update_cells(torch_cuda, "q8", dim, TC.quant_rows(dim), TC.quant_expectation(dim))


@pytest.mark.parametrize("dim", STREAM_DIMS)
def test_update_cells_16_bit_and_float32(torch_cuda, dim):
    """The streaming updater at V = 1, 2, 4, single slots and rows of many: N.narrow for the 16-bit kinds, a copy for float32."""
    x = TC.quant_rows(dim)
    for kind in ("bf16", "f16", "f32"):
        _update_cells(torch_cuda, kind, dim, x, R.expect_bytes(x, kind))


@pytest.mark.parametrize("dim", (4, 2, 1))
def test_update_edge_values_through_the_scattered_store(torch_cuda, dim):
    """N.EDGE_VALUES — every rounding edge of both 16-bit types, NaN among them — through the scattered store: where the
    expected element is not NaN the pattern of N.narrow, a NaN stays NaN; float32 keeps every bit pattern."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    x = np.resize(N.EDGE_VALUES, (len(N.EDGE_VALUES) // dim + 1, dim)).astype(np.float32)
    n = x.shape[0]
    table_rows = n + R.SLACK_ROWS
    ids = R.distinct_ids(n, table_rows, 77 + dim)
    assert len(set(ids.tolist())) == n
    for kind in ("bf16", "f16", "f32"):
        buf, table = R.poisoned(torch, kind, dim, table_rows, dev)
        tables.update_rows(table, _dev(torch, ids), _dev(torch, x))
        got = buf.cpu().numpy().reshape(table_rows + R.BEHIND_ROWS, -1)
        named = np.zeros(table_rows + R.BEHIND_ROWS, bool)
        named[ids] = True
        assert (got[~named] == R.POISON).all(), (kind, dim)
        if kind == "f32":
            assert (got[ids].view(np.uint32) == x.view(np.uint32)).all()
            continue
        g16, want = got[ids].view(np.uint16), N.narrow(x, kind)
        nan = N.is_nan16(want, kind)
        assert nan.any() and (nan == np.isnan(x)).all()
        assert (N.is_nan16(g16, kind) == nan).all(), (kind, dim, "NaN did not stay NaN")
        assert (g16[~nan] == want[~nan]).all(), (kind, dim)


@pytest.mark.parametrize("kind,dim", (("q8", 3), ("q8", 64), ("q8", 260), ("bf16", 64), ("bf16", 6)),
                         ids=("q8-G1", "q8-G16", "q8-G64", "bf16-V4", "bf16-V2"))
def test_skipped_ids(torch_cuda, kind, dim):
    """Ids outside [0, table_rows) at fixed positions: -1, table_rows (INSIDE the allocation: a missing range check would
    overwrite poison), 2^32 + 5 (its low half names row 5, which no other id names) and INT64_MIN.  Their rows land nowhere,
    the counter rises by four from whatever it held, and a null counter is accepted."""
    torch = torch_cuda
    from recom_amd import tables
    if kind == "q8":
        assert TC.group_of(dim) == {3: 1, 64: 16, 260: 64}[dim]
    dev = torch.device("cuda", 0)
    n = 257
    table_rows = n + R.SLACK_ROWS
    x = TC.quant_rows(dim)[:n]
    want = R.expect_bytes(x, kind)
    ids = R.distinct_ids(n, table_rows, 5 + dim, exclude=(5,))
    outside = {5: -1, 6: table_rows, 64: (1 << 32) + 5, n - 1: R.INT64_MIN}
    for pos, bad in outside.items():
        ids[pos] = bad
    keep = np.asarray([i for i in range(n) if i not in outside])
    assert 5 not in ids and len(set(ids[keep].tolist())) == len(keep)
    d_ids, d_x = _dev(torch, ids), _dev(torch, x)
    for counter in (torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), 7, dtype=torch.int64, device=dev), None):
        buf, table = R.poisoned(torch, kind, dim, table_rows, dev)
        before = 0 if counter is None else int(counter.item())
        tables.update_rows(table, d_ids, d_x, skipped=counter)
        R.check_poisoned(buf, kind, dim, table_rows, ids[keep], want[keep], (kind, dim, "skipped"))
        if counter is not None:
            assert int(counter.item()) == before + len(outside)
    # every id outside: nothing is written, every row is counted
    far = np.asarray([table_rows + i for i in range(n)], np.int64)
    far[::3] = -1 - np.arange(len(far[::3]))
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    buf, table = R.poisoned(torch, kind, dim, table_rows, dev)
    tables.update_rows(table, _dev(torch, far), d_x, skipped=counter)
    assert bool((buf == R.POISON).all()) and int(counter.item()) == n


@pytest.mark.parametrize("dim", (7, 6, 64))
@pytest.mark.parametrize("kind", ("q8", "bf16", "f16", "f32"))
def test_equality_with_convert(torch_cuda, kind, dim):
    """update_rows(convert(master), ids, delta) == convert(master with the delta applied), whole tables as bytes.  dim 7: q8
    rows of 15 bytes start at every byte alignment."""
    torch = torch_cuda
    from recom_amd import tables
    master = TC.quant_rows(dim)[:500].copy()
    delta = TC.family_rows(dim, 170, 11)
    ids = np.random.default_rng(dim).permutation(500)[:170].astype(np.int64)
    assert len(set(ids.tolist())) == 170
    applied = master.copy()
    applied[ids] = delta
    if kind == "f32":                                            # float32 -> float32 is no conversion: the master itself
        a, b = _dev(torch, master), _dev(torch, applied)
    else:
        a, b = tables.convert(_dev(torch, master), kind), tables.convert(_dev(torch, applied), kind)
    tables.update_rows(a, _dev(torch, ids), _dev(torch, delta))
    ga, gb = _bytes(torch, a), _bytes(torch, b)
    assert ga.shape == gb.shape == (500, R.row_bytes(kind, dim))
    bad = np.argwhere((ga != gb).any(axis=1))[:, 0]
    assert bad.size == 0, (kind, dim, bad[:5])
    assert (gb == R.expect_bytes(applied, kind)).all()


N_OUTSIDE = 5


def _read_ids(rows: int, repeats: int, seed: int):
    """int64 [rows + repeats + N_OUTSIDE]: every row of a table of `rows` rows once, in a seeded order, `repeats` rows a
    second time, and five ids outside the table in between; and which of them lie inside."""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([rng.permutation(rows), rng.integers(0, rows, repeats)]).astype(np.int64)
    n = len(ids)
    ids = np.insert(ids, [3, min(64, n), min(64, n), n // 2, n], [-1, rows, (1 << 32) + 1, rows + 2, R.INT64_MIN])
    inside = (ids >= 0) & (ids < rows)
    assert (~inside).sum() == N_OUTSIDE and set(ids[inside].tolist()) == set(range(rows))
    return ids, inside


def _read(torch, table, ids: np.ndarray, dim: int) -> np.ndarray:
    """read_rows into the front of a sentinel-filled buffer; the element behind the last row keeps its sentinel."""
    from recom_amd import tables
    n = len(ids)
    out = torch.empty((n * dim + 1,), dtype=torch.int32, device=table.device).fill_(0x5A5A5A5A).view(torch.float32)
    front = out[:n * dim].view(n, dim)
    assert tables.read_rows(table, _dev(torch, ids), out=front) is front
    got = out.cpu().numpy()
    assert got[-1:].view(np.uint32)[0] == 0x5A5A5A5A, "the element behind the last row was written"
    return got[:-1].reshape(n, dim)


@pytest.mark.parametrize("dim", (1, 3, 4, 6, 64))
def test_read_q8_arbitrary_bytes(torch_cuda, dim):
    """q8 rows of random bytes (scales and biases of every kind, NaN and infinity among them) by id equal
    synth.dequantize_q8 bit for bit; ids outside the table give rows whose bits are all zero."""
    torch = torch_cuda
    from recom_amd import tables
    rows = 1027
    q = np.random.default_rng(50 + dim).integers(0, 256, (rows, dim + 8), dtype=np.uint8)
    ids, inside = _read_ids(rows, 468, dim)
    n = len(ids)
    got = _read(torch, _dev(torch, q), ids, dim)
    T16.assert_same_bits(got[inside], synth.dequantize_q8(q[ids[inside]]), ("read q8", dim))
    assert (got[~inside].view(np.uint32) == 0).all()
    fresh = tables.read_rows(_dev(torch, q), _dev(torch, ids))      # the allocating form
    assert fresh.dtype == torch.float32 and tuple(fresh.shape) == (n, dim)
    T16.assert_same_bits(fresh.cpu().numpy(), got, ("read q8, fresh", dim))


@pytest.mark.parametrize("dtype", T16.DTYPES)
def test_read_16_bit_every_pattern(torch_cuda, dtype):
    """All 65 536 patterns of the type as tables of dim 4, 2 and 1, read by a permutation of the rows: T16.widen, and for
    bf16 (widened in integers) the exact bits, NaN payloads included."""
    torch = torch_cuda
    bits = np.arange(65536, dtype=np.uint16)
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    for dim in (4, 2, 1):
        rows = 65536 // dim
        ids, inside = _read_ids(rows, 100, 9 + dim)
        table = _dev(torch, bits.view(np.int16).reshape(-1, dim)).view(tdt)
        got = _read(torch, table, ids, dim)
        want = T16.widen(bits.reshape(-1, dim)[ids[inside]], dtype)
        T16.assert_same_bits(got[inside], want, ("read", dtype, dim))
        if dtype == "bf16":
            assert (got[inside].view(np.uint32) == want.view(np.uint32)).all()
        assert (got[~inside].view(np.uint32) == 0).all()


@pytest.mark.parametrize("dim", (64, 6, 3))
def test_read_float32_is_a_copy(torch_cuda, dim):
    torch = torch_cuda
    rows = 700
    x = np.random.default_rng(dim).integers(0, 2 ** 32, (rows, dim), dtype=np.uint64).astype(np.uint32)
    ids, inside = _read_ids(rows, 200, 4 + dim)
    got = _read(torch, _dev(torch, x.view(np.float32)), ids, dim).view(np.uint32)
    assert (got[inside] == x[ids[inside]]).all() and (got[~inside] == 0).all()


@pytest.mark.parametrize("dim", (64, 6, 3))
@pytest.mark.parametrize("kind", ("f32", "bf16", "f16", "q8"))
def test_read_equals_the_plans(torch_cuda, kind, dim):
    """read_rows and a one-column FCP_FORM_GATHER plan over the same table and ids, ids outside the table included: the same
    bits."""
    torch = torch_cuda
    from recom_amd import tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import (COMBINER_NONE, FORM_GATHER, IDS_I64, ROWS_FROM_IDS, SEG_NONE, ColumnSpec, PlanSpec)
    dev = torch.device("cuda", 0)
    vocab = 333
    spec = PlanSpec([ColumnSpec(FORM_GATHER, dim, vocab, COMBINER_NONE, IDS_I64, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 0)],
                    [1], [8], 1, n_groups=1, n_symbols=0)
    spec.validate()
    master = _dev(torch, TC.quant_rows(dim)[:vocab])
    table = master if kind == "f32" else tables.convert(master, kind)
    ids, inside = _read_ids(vocab, 162, 30 + dim)
    assert len(ids) == 500
    op = FeatureColumnProcess(spec if kind == "f32" else spec.with_table_dtype(kind), 0)
    assert op.plan.table_dtype() == kind
    blob, offsets, shapes = concat_inputs([ids])
    out = op(torch.from_numpy(blob).to(dev), offsets, shapes, [table], None)
    got = tables.read_rows(table, _dev(torch, ids))
    torch.cuda.synchronize()
    plan = out.groups[0].cpu().numpy()
    assert plan.shape == (500, dim) and plan.dtype == np.float32
    assert (plan.view(np.uint32) == got.cpu().numpy().view(np.uint32)).all(), (kind, dim)
    assert (plan[~inside].view(np.uint32) == 0).all() and np.abs(plan[inside]).max() > 0


def test_plan_on_an_updated_table(torch_cuda):
    """The two-column model (a gather, a mean-pooled column) on q8 tables of which a third of the rows were updated: the
    tables are the restatement's bytes, and the plan's output equals, bit for bit, the float32 plan on the dequantised
    updated tables."""
    torch = torch_cuda
    from recom_amd import tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    spec, masters, deltas, (inputs, symbols) = R.small_model()
    q8 = [tables.convert(_dev(torch, m), "q8") for m in masters]
    for t, (ids, rows) in zip(q8, deltas):
        assert len(ids) == t.shape[0] // 3
        tables.update_rows(t, _dev(torch, ids), _dev(torch, rows))
    want_q8, want_deq = R.small_model_expected_tables(masters, deltas)
    for t, w in zip(q8, want_q8):
        assert (t.cpu().numpy() == w).all()
    op, op32 = FeatureColumnProcess(spec.with_table_dtype("q8"), 0), FeatureColumnProcess(spec, 0)
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    out = op(d_blob, offsets, shapes, q8, symbols)
    ref = op32(d_blob, offsets, shapes, [_dev(torch, w) for w in want_deq], symbols)
    torch.cuda.synchronize()
    got, want = out.groups[0].cpu().numpy(), ref.groups[0].cpu().numpy()
    assert got.shape == (int(symbols[0]), 12) and not np.isnan(want).any() and np.abs(want).max() > 0
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("kind,rows", (("q8", 1 << 26), ("f32", TC.BIG_ROWS)), ids=("q8-4.8GB", "f32-4.3GB"))
def test_offsets_beyond_32_bits(torch_cuda, kind, rows):
    """A zero-filled table of dim 64 whose byte offsets pass 2^32: the three rows around byte offset 2^32, the last 64 rows
    and 1 000 sampled rows are updated with the closed form of TC.big_rows_numpy, read back with read_rows and by indexing,
    and compared with the restatement; 1 000 untouched sampled rows are still zero."""
    torch = torch_cuda
    from recom_amd import tables
    dim = TC.BIG_DIM
    rb = R.row_bytes(kind, dim)
    free, _total = torch.cuda.mem_get_info()
    need = rows * rb + (1 << 30)
    assert free >= need, f"needs {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free"
    dev = torch.device("cuda", 0)
    table = torch.zeros((rows, dim + 8), dtype=torch.uint8, device=dev) if kind == "q8" else torch.zeros((rows, dim), dtype=torch.float32, device=dev)
    edge = (1 << 32) // rb
    rng = np.random.default_rng(8)
    ids = np.unique(np.concatenate([[edge - 1, edge, edge + 1], np.arange(rows - 64, rows), rng.integers(0, rows, 1000)])).astype(np.int64)
    ids = ids[rng.permutation(len(ids))]
    assert rows * rb > 2 ** 32 and edge + 1 < rows and ids.max() == rows - 1 and len(set(ids.tolist())) == len(ids)
    x = TC.big_rows_numpy(ids)
    d_ids = _dev(torch, ids)
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    tables.update_rows(table, d_ids, _dev(torch, x), skipped=skipped)
    want = R.expect_bytes(x, kind)
    assert int(skipped.item()) == 0
    assert (_bytes(torch, table[d_ids]) == want).all()
    read = tables.read_rows(table, d_ids).cpu().numpy()
    want32 = synth.dequantize_q8(want) if kind == "q8" else x
    assert (read.view(np.uint32) == want32.view(np.uint32)).all()
    others = np.setdiff1d(rng.integers(0, rows, 1100), ids)[:1000].astype(np.int64)
    assert len(others) == 1000
    assert bool((table[_dev(torch, others)] == 0).all())
    del table
    torch.cuda.empty_cache()
