"""fcp_table_count_ids and fcp_table_audit_weighted on the GPU (kernels: recom_amd/csrc/fcp_table_traffic.hip,
fcp_table_audit.hip), and the path from counted traffic to a served plan.

Counting is exact: the count array equals np.bincount modulo 2^32 (table_traffic_cases.count_ref) and `skipped` the number of
ids outside the table, whatever the grid, the LDS table or the order did.  The weighted audit: everything that decides
admissibility equals the unweighted audit's to the bit; a float64 sum lies within (n_elements + rows) * 2^-52, relative, of
table_traffic_cases.weighted_aggregate — the kernel's n fused adds are within n * 2^-53 of the exact sum, numpy's per-row sums,
one product a row and the sum over the rows within (dim + rows) * 2^-53 of it, every term non-negative."""
import numpy as np
import pytest

import table_audit_cases as TA
import table_convert_cases as TC
import table_traffic_cases as TT

pytestmark = pytest.mark.gpu

FULL_PASS_DIMS = (3, 4, 5, 62, 64, 300, TC.REGISTER_CAP[4] + 4)      # the dims tests/test_gpu_table_audit.py gives a full pass
GUARD = 64                                                            # cells before and after a count array
GUARD_BITS = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _count(torch, table_rows, ids, start=None, with_skipped=True, skipped0=0):
    """tables.count_ids of the host ids into a count array between two guards; (uint32 counts, skipped or None) on the host"""
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    host = np.full(table_rows + 2 * GUARD, GUARD_BITS, np.uint32)
    host[GUARD:GUARD + table_rows] = 0 if start is None else start
    buf = torch.from_numpy(host.view(np.int32)).to(dev)
    counts = buf[GUARD:GUARD + table_rows]
    skipped = torch.full((1,), skipped0, dtype=torch.int64, device=dev) if with_skipped else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
    assert tables.count_ids(counts, d_ids, skipped=skipped) is counts
    torch.cuda.synchronize()
    back = buf.cpu().numpy().view(np.uint32)
    assert (back[:GUARD] == GUARD_BITS).all() and (back[GUARD + table_rows:] == GUARD_BITS).all(), "a guard cell was written"
    return back[GUARD:GUARD + table_rows].copy(), (int(skipped.item()) if with_skipped else None)


@pytest.mark.parametrize("id_dtype", (np.int64, np.int32), ids=("int64", "int32"))
def test_counts_equal_bincount(torch_cuda, id_dtype):
    """Every size at every vocabulary and pattern: n from one id to a full pass of the grid + 1, table_rows 1, 2 and more rows
    than the LDS table has cells, and the five id patterns (at the small sizes; the largest takes uniform and Zipf ids)."""
    for table_rows in (1, 2, TT.BIG_VOCAB):
        for n in TT.SIZES:
            patterns = TT.PATTERNS if n <= TT.TILE_IDS + 1 else ("uniform", "zipf")
            for pattern in patterns:
                ids = TT.draw_ids(pattern, n, table_rows, seed=n % 97).astype(id_dtype)
                want, _ = TT.count_ref(table_rows, ids)
                got, skipped = _count(torch_cuda, table_rows, ids)
                assert skipped == 0 and got.dtype == np.uint32
                assert np.array_equal(got, want), (table_rows, n, pattern, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("id_dtype", (np.int64, np.int32), ids=("int64", "int32"))
def test_the_fall_through_and_the_probes(torch_cuda, id_dtype):
    """More distinct rows in one block's share than its LDS table holds: `tiles - 1` passes of the grid and a tile give block 0
    `tiles` tiles, more than SLOTS distinct rows whose home slots collide tile by tile.  And rows congruent modulo the slot count
    at a size where every block sees all of them: PROBES cells by probing, the rest straight to memory."""
    torch = torch_cuda
    tiles = TT.SLOTS // TT.TILE_IDS + 1
    n = (tiles - 1) * TT.GRID_BLOCKS * TT.TILE_IDS + TT.TILE_IDS
    table_rows = n + 5
    assert tiles * TT.TILE_IDS > TT.SLOTS and (TT.GRID_BLOCKS * TT.TILE_IDS) % TT.SLOTS == 0
    ids = TT.draw_ids("distinct", n, table_rows).astype(id_dtype)
    got, skipped = _count(torch, table_rows, ids)
    assert skipped == 0 and (got[:n] == 1).all() and not got[n:].any()
    n = 4 * TT.GRID_BLOCKS * TT.TILE_IDS + 77
    ids = TT.draw_ids("congruent", n, TT.BIG_VOCAB, seed=3).astype(id_dtype)
    got, skipped = _count(torch, TT.BIG_VOCAB, ids)
    assert skipped == 0 and np.array_equal(got, TT.count_ref(TT.BIG_VOCAB, ids)[0]) and np.count_nonzero(got) == 3 * TT.PROBES
    # both at once: a hot head inside a stream of distinct rows
    ids = TT.draw_ids("distinct", n, table_rows)
    ids[::3] = TT.draw_ids("zipf", len(ids[::3]), 50, seed=4)
    ids = ids.astype(id_dtype)
    got, skipped = _count(torch, table_rows, ids)
    assert skipped == 0 and np.array_equal(got, TT.count_ref(table_rows, ids)[0])


def test_ids_outside_the_table(torch_cuda):
    """-1, table_rows, 2^32 + a valid row as int64 (the whole value is compared), INT64_MIN and negative int32 ids touch no
    memory and are counted in skipped — added to what the counter held; with skipped NULL they are dropped."""
    torch = torch_cuda
    for table_rows in (1, 2, 1000, TT.BIG_VOCAB):
        out = TT.outside_ids(table_rows)
        rng = np.random.default_rng(table_rows)
        for n in (len(out), 64, 257, TT.TILE_IDS + 1, 3 * TT.TILE_IDS + 5):
            ids = rng.integers(0, table_rows, n, dtype=np.int64)
            where = rng.permutation(n)[:max(len(out), n // 3)]
            ids[where] = out[np.arange(len(where)) % len(out)]
            want, n_out = TT.count_ref(table_rows, ids)
            assert n_out >= 7
            got, skipped = _count(torch, table_rows, ids, skipped0=1000)
            assert np.array_equal(got, want) and skipped == 1000 + n_out, (table_rows, n, skipped, n_out)
            got, skipped = _count(torch, table_rows, ids, with_skipped=False)
            assert np.array_equal(got, want) and skipped is None
            ids32 = np.where((ids >= -2 ** 31) & (ids < 2 ** 31), ids, -7).astype(np.int32)      # (what does not fit: another negative id)
            ids32[where[0]] = -2 ** 31
            want, n_out = TT.count_ref(table_rows, ids32)
            got, skipped = _count(torch, table_rows, ids32)
            assert np.array_equal(got, want) and skipped == n_out > 0, (table_rows, n, skipped, n_out)
    # a whole wave, a whole block and a whole call outside
    for n in (64, TT.BLOCK_THREADS, TT.TILE_IDS + 3):
        got, skipped = _count(torch, 5, np.full(n, -1, np.int64))
        assert not got.any() and skipped == n


def test_accumulation_wrap_and_dtypes(torch_cuda):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    # a cell preset to 2^32 - 2 plus five reads gives 3
    start = np.asarray([7, 2 ** 32 - 2, 0], np.uint32)
    got, _ = _count(torch, 3, np.asarray([1, 1, 0, 1, 1, 1], np.int64), start=start)
    assert got.tolist() == [8, 3, 0]
    got, _ = _count(torch, 3, np.full(TT.TILE_IDS + 5, 1, np.int32), start=start)
    assert got.tolist() == [7, (2 ** 32 - 2 + TT.TILE_IDS + 5) % 2 ** 32, 0]
    # two calls add up; ids of any shape; the count tensor new_counts makes (uint32 where torch has it)
    counts = tables.new_counts(TT.BIG_VOCAB, dev)
    assert counts.shape == (TT.BIG_VOCAB,) and counts.element_size() == 4 and counts.device == dev
    a = TT.draw_ids("zipf", 3000, TT.BIG_VOCAB, seed=1).reshape(30, 100)
    b = TT.draw_ids("uniform", 2 * TT.TILE_IDS + 1, TT.BIG_VOCAB, seed=2).astype(np.int32)
    tables.count_ids(counts, torch.from_numpy(a).to(dev))
    tables.count_ids(counts, torch.from_numpy(b).to(dev))
    tables.count_ids(counts, torch.empty((0,), dtype=torch.int64, device=dev))           # n == 0: nothing
    torch.cuda.synchronize()
    want, _ = TT.count_ref(TT.BIG_VOCAB, b, start=TT.count_ref(TT.BIG_VOCAB, a)[0])
    assert np.array_equal(counts.view(torch.int32).cpu().numpy().view(np.uint32), want)
    with pytest.raises(ValueError, match="contiguous"):
        tables.count_ids(counts, torch.from_numpy(a).to(dev)[:, ::2])
    with pytest.raises(ValueError, match="int32 or int64"):
        tables.count_ids(counts, torch.zeros((4,), dtype=torch.int16, device=dev))


def test_on_a_side_stream_behind_a_fill(torch_cuda):
    """The call is ordered on the stream it is given: counts full of 9s, zeroed on a side stream, counted on that stream."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    rows = 1 << 20
    ids = TT.draw_ids("zipf", 1 << 18, rows, seed=5)
    d_ids = torch.from_numpy(ids).to(dev)
    counts = torch.full((rows,), 9, dtype=torch.int32, device=dev)
    skipped = torch.zeros((1,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        counts.fill_(0)
        tables.count_ids(counts, d_ids, skipped=skipped, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), TT.count_ref(rows, ids)[0]) and int(skipped.item()) == 0
    torch.cuda.synchronize()


# ---- the weighted audit --------------------------------------------------------------------------------------------------------
def _admissibility(a):
    """every field of a tables.TableAudit that is not a sum, max_abs_err as its bits"""
    return (a.rows, a.dim, a.rows_nonfinite, a.first_nonfinite_row) + tuple(
        (a.kinds[k].rows_bad, a.kinds[k].first_bad_row, np.float32(a.kinds[k].max_abs_err).view(np.uint32).item(), a.raw.kind[TA.KINDS[k]].reserved)
        for k in ("f32",) + TA.COMPACT)


def _sums(a):
    return (a.sum_sq,) + tuple(a.kinds[k].sum_sq_err for k in ("f32",) + TA.COMPACT)


def _weighted_cases(dim):
    """(rows, first, last): no row, one row, rows per block + 1 with a non-finite and a bad row first and last, and — for
    FULL_PASS_DIMS — one row more than a pass of the fixed grid"""
    rpb = TA.rows_per_block(dim)
    q8_bad = "q8_bad" if dim >= 2 else "f16_bad"
    out = [(0, None, None), (1, None, None), (1, "nan", None), (rpb + 1, "neg_inf", "bf16_bad"), (rpb + 1, q8_bad, "good")]
    if dim in FULL_PASS_DIMS:
        out.append((TA.GRID_BLOCKS * rpb + 1, "f16_bad", "nan"))
    return out


@pytest.mark.parametrize("dim", TA.DIMS, ids=[f"dim{d}-V{TC.vec_of(d)}-G{TC.group_of(d)}" for d in TA.DIMS])
def test_weighted_audit_cells(torch_cuda, dim):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    src = torch.from_numpy(np.array(TA.source(dim))).to(dev)
    stats = TA.source_stats(dim)

    def on_device(c):
        return torch.from_numpy(np.ascontiguousarray(c, np.uint32).view(np.int32)).to(dev)

    for rows, first, last in _weighted_cases(dim):
        what = (dim, rows, first, last)
        idx = TA.table_index(dim, rows, first, last)
        t = src[torch.from_numpy(idx).to(dev)].contiguous() if rows else torch.empty((0, dim), dtype=torch.float32, device=dev)
        plain = tables.audit(t)
        # all ones: the bytes of the unweighted audit
        ones = tables.audit(t, row_counts=on_device(np.ones(rows, np.uint32)))
        assert bytes(ones.raw) == bytes(plain.raw), what
        # all zeros: sums exactly 0.0, every other field the unweighted audit's
        zeros = tables.audit(t, row_counts=on_device(np.zeros(rows, np.uint32)))
        assert _sums(zeros) == (0.0,) * 5 and _admissibility(zeros) == _admissibility(plain), what
        assert not any(np.signbit(v) for v in _sums(zeros)), what
        # random counts with 0 and 2^32 - 1 among them
        c = TT.draw_counts(rows, dim)
        got = tables.audit(t, row_counts=on_device(c))
        want = TT.weighted_aggregate(stats, idx, c)
        assert _admissibility(got) == _admissibility(plain), what
        tol = (rows * dim + rows) * 2.0 ** -52
        print(what, "sum_sq", got.sum_sq, want["sum_sq"])
        assert np.isfinite(got.sum_sq) and abs(got.sum_sq - want["sum_sq"]) <= tol * want["sum_sq"], (what, got.sum_sq, want["sum_sq"])
        assert got.kinds["f32"].sum_sq_err == 0.0
        for kind in TA.COMPACT:
            g, w = got.kinds[kind].sum_sq_err, want[kind]["sum_sq_err"]
            print("   ", kind, g, w)
            assert np.isfinite(g) and abs(g - w) <= tol * w, (what, kind, g, w)
        # the same bytes twice
        again = tables.audit(t, row_counts=on_device(c))
        assert bytes(again.raw) == bytes(got.raw), what
        # counts only on rows the sums leave out: non-finite rows for all of them, a kind's bad rows for that kind's
        nonfinite = ~stats["finite"][idx]
        only = tables.audit(t, row_counts=on_device(np.where(nonfinite, np.uint32(0xFFFFFFFF), np.uint32(0))))
        assert _sums(only) == (0.0,) * 5 and _admissibility(only) == _admissibility(plain), what
        for kind in TA.COMPACT:
            left_out = nonfinite | stats[kind]["bad"][idx]
            only = tables.audit(t, row_counts=on_device(np.where(left_out, np.uint32(0xFFFFFFFF), np.uint32(0))))
            assert only.kinds[kind].sum_sq_err == 0.0 and all(np.isfinite(v) for v in _sums(only)), (what, kind)
            assert _admissibility(only) == _admissibility(plain), (what, kind)


def test_wrappers_on_the_device(torch_cuda):
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    t = torch.ones((6, 8), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="row_counts has 5 cells, the table 6 rows"):
        tables.audit(t, row_counts=tables.new_counts(5, dev))
    with pytest.raises(ValueError, match="row_counts on cpu"):
        tables.audit(t, row_counts=torch.zeros((6,), dtype=torch.int32))
    c = tables.new_counts(6, dev)
    tables.count_ids(c, torch.tensor([5, 5, 5, 2], device=dev))
    a = tables.audit(t, row_counts=c)
    assert a.sum_sq == 8.0 * 4 and a.rows == 6 and tables.audit(t).sum_sq == 8.0 * 6


# ---- from counted traffic to a served plan -------------------------------------------------------------------------------------
def test_from_traffic_to_a_served_plan(torch_cuda):
    """Two tables of one shape, table 1 = table 0 with its rows permuted; half the rows small integers (bf16 holds them), half
    noisy.  Every element is a multiple of 2^-10 below 4 in magnitude, so every square of a value or of a bf16 error is a
    multiple of 2^-20 and every sum here is exact in float64 in any order: the unweighted audits are EQUAL.  Requests read
    table 0's noisy rows and table 1's exact rows.  With weights (1, 1) and a budget that lets exactly one table go to bf16, the
    unweighted choice is a tie and takes table 0; the weighted choice takes table 1, whose traffic loses nothing; with the
    tables swapped it follows the traffic.  The plan on the chosen formats is, bit for bit, the float32 plan on the converted
    tables."""
    torch = torch_cuda
    from recom_amd import tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import COMBINER_NONE, FORM_GATHER, IDS_I64, ROWS_FROM_IDS, SEG_NONE, ColumnSpec, PlanSpec
    dev = torch.device("cuda", 0)
    rows, dim = 64, 8
    cols = [ColumnSpec(FORM_GATHER, dim, rows, COMBINER_NONE, IDS_I64, t, t, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, t) for t in (0, 1)]
    spec32 = PlanSpec(cols, [1, 1], [8, 8], 2, n_groups=1, n_symbols=0)
    spec32.validate()
    rng = np.random.default_rng(77)
    t0 = rng.integers(-3, 4, (rows, dim)).astype(np.float32)
    noisy = np.arange(rows) % 2 == 1
    t0[noisy] = (rng.integers(-4000, 4000, (rows // 2, dim)) | 1).astype(np.float32) / np.float32(1024.0)    # 12 odd bits: no bf16 value
    perm = rng.permutation(rows)
    host = [t0, t0[perm]]
    noisy_rows = [np.flatnonzero(noisy), np.flatnonzero(noisy[perm])]
    exact_rows = [np.flatnonzero(~noisy), np.flatnonzero(~noisy[perm])]
    zipf = (rng.zipf(1.5, size=4000) - 1) % (rows // 2)
    streams = [noisy_rows[0][zipf].astype(np.int64), exact_rows[1][zipf[::-1]].astype(np.int32)]       # (both id widths)
    tabs = [torch.from_numpy(h).to(dev) for h in host]
    counts = [tables.count_ids(tables.new_counts(rows, dev), torch.from_numpy(s).to(dev)) for s in streams]
    plain = tables.audit_tables(spec32, tabs)
    assert bytes(plain[0].raw) == bytes(plain[1].raw) and plain[0].kinds["bf16"].sum_sq_err > 0 and plain[0].admissible("bf16")
    weighted = tables.audit_tables(spec32, tabs, row_counts=counts)
    assert weighted[0].kinds["bf16"].sum_sq_err > 0 and weighted[1].kinds["bf16"].sum_sq_err == 0.0
    half_and_half = tables.audit_tables(spec32, tabs, row_counts=[counts[0], None])
    assert bytes(half_and_half[0].raw) == bytes(weighted[0].raw) and bytes(half_and_half[1].raw) == bytes(plain[1].raw)
    budget = rows * dim * (4 + 2)
    pick = dict(allowed=("bf16",), weights=(1.0, 1.0))
    assert tables.choose_dtypes(spec32, plain, budget, **pick)[0] == ("bf16", "f32")            # a tie: the lower index
    names, nbytes, err = tables.choose_dtypes(spec32, weighted, budget, **pick)
    assert names == ("f32", "bf16") and nbytes == budget and err == 0.0
    swapped = tables.audit_tables(spec32, tabs[::-1], row_counts=counts[::-1])
    assert tables.choose_dtypes(spec32, swapped, budget, **pick)[0] == ("bf16", "f32")
    # the plan on the chosen formats
    spec = spec32.with_table_dtypes(names)
    compact = [tables.convert(t, n) if n != "f32" else t for t, n in zip(tabs, names)]
    widened = [tables.convert(t, "f32") if n != "f32" else t for t, n in zip(compact, names)]
    blob, offsets, shapes = concat_inputs([streams[0][:5].astype(np.int64), streams[1][:5].astype(np.int64)])
    d_blob = torch.from_numpy(blob).to(dev)
    outs = []
    for s, tt in ((spec, compact), (spec32, widened)):
        op = FeatureColumnProcess(s, 0)
        out = op(d_blob, offsets, shapes, tt, [])
        torch.cuda.synchronize()
        outs.append(out.groups[0].contiguous().cpu().numpy())
        del op
    assert outs[0].dtype == np.float32 and outs[0].shape == (5, 2 * dim) and outs[0].any() and outs[0].tobytes() == outs[1].tobytes()
    assert np.array_equal(outs[0][:, dim:], host[1][streams[1][:5]])              # table 1's traffic reads rows bf16 holds exactly
