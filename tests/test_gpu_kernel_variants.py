"""Every fused-kernel instantiation under every output store policy, as an explicit cell (tests/kernel_variant_cases.py):
fcp_dense_kernel<V, R, SHARDED>, fcp_ragged_kernel<V, SHARDED> and fcp_hybrid_kernel<V, R, SHARDED> for V, R in {1, 2, 4},
each with `nt`, write-through `sc1 nt` and plain stores, the dense and hybrid ones also with the 64-bit row arithmetic.

For every cell a small plan that lands in it runs three requests with different inputs into caller-owned arenas that are
filled with 0xFF bytes (NaN) first, so a store that is skipped or lands elsewhere shows even in a reused arena.  Each
request asserts the launch report (fcp_plan_last_launch: the cell was reached, not assumed, down to the grid's block
count with the XCD mapping's padding), equals the C oracle bit for bit — row-sharded plans: the per-rank partials of rank
0 and of the last rank of world 2 or 3 — lies within the fp32 rounding bound of the float64 restatement (unsharded), and
counts the oracle's bad ids.  Reached by shape and per-plan settings only (FCP_STORE_THROUGH_BYTES and
FCP_DIAG=wide_rows are read at plan creation); no process-wide switch."""
import os

import numpy as np
import pytest

import kernel_variant_cases as K

pytestmark = pytest.mark.gpu

CELLS = K.cells()


def _expected_launch(cell, case, rows, t):
    kernel = {(True, False): "dense", (False, True): "ragged", (True, True): "hybrid"}[
        (any(c[0] for c in case.span_counts), any(c[1] for c in case.span_counts))]
    assert kernel == cell.kernel, (cell.id, case.span_counts)       # (the generator's own promise)
    dense_blocks, ragged_blocks = K.expected_blocks(case.span_counts, rows, cell.rpw)
    seg_ids = any(c.form == K.FORM_SEGMENT_REDUCE and c.seg_kind != K.SEG_CSR_I32 for c in case.spec.columns)
    want = dict(kernel=kernel, vec=cell.vec, store=cell.store if not (cell.store == "plain" and t == 0) else "sc1_nt",
                wide_rows=cell.wide, shard_world=1, dense_blocks=dense_blocks, ragged_blocks=ragged_blocks,
                segment_offsets="none" if not seg_ids else ("prepass" if cell.sharded else "search"))
    if kernel != "ragged":
        want["rows_per_wave"] = cell.rpw
    return want


@pytest.mark.parametrize("cell", CELLS, ids=[c.id for c in CELLS])
def test_kernel_variant_cell(oracle, monkeypatch, cell):
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    case = K.build_case(*cell.key)
    # per-plan settings, read when the plan is created
    if cell.store == "nt":
        monkeypatch.delenv("FCP_STORE_THROUGH_BYTES", raising=False)
    else:
        monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    diag = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] != "wide_rows"]
    monkeypatch.setenv("FCP_DIAG", ",".join(diag + (["wide_rows"] if cell.wide else [])))
    dev = torch.device("cuda", 0)
    world = 2 + CELLS.index(cell) % 2 if cell.sharded else 1
    bad_total = 0
    for rank in ((0, world - 1) if cell.sharded else (0,)):
        spec = case.spec.with_shard(rank, world) if cell.sharded else case.spec
        tables = [np.ascontiguousarray(t[rank::world]) for t in case.tables]
        d_tabs = [torch.from_numpy(t).to(dev) for t in tables]
        op = FeatureColumnProcess(spec, 0)
        plan_dict = spec.to_dict()
        packed = [concat_inputs(inputs) for inputs, _ in case.requests]
        nbytes = max(max(op.plan.arena_bytes(shapes, sym), 128) for (_, _, shapes), (_, sym) in zip(packed, case.requests))
        # `sc1_nt`: a ring of three arenas (the plan remembers two); `plain`: one arena, reused; `nt`: a ring as well
        arenas = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if cell.store == "plain" else 3)]
        for t, ((inputs, symbols), (blob, offsets, shapes)) in enumerate(zip(case.requests, packed)):
            what = (cell.id, rank, world, t)
            arena = arenas[t % len(arenas)]
            arena.fill_(0xFF)                                   # on the request's stream (torch's current one)
            d_blob = torch.from_numpy(blob).to(dev)
            out = op(d_blob, offsets, shapes, d_tabs, symbols, arena=arena)
            torch.cuda.synchronize()
            assert out.buffer.data_ptr() == arena.data_ptr(), what
            rows = [int(r) for r in symbols]
            want_launch = _expected_launch(cell, case, rows, t)
            want_launch["shard_world"] = world
            got_launch = op.plan.last_launch()
            assert {k: got_launch[k] for k in want_launch} == want_launch, what
            want, bad = oracle.process_feature_columns(plan_dict, blob, offsets, shapes, tables, symbols)
            got_groups = [g.cpu().numpy() for g in out.groups]
            for g, (got, w) in enumerate(zip(got_groups, want)):
                assert got.shape == w.shape, (what, g)
                diff = ~((got == w) | (np.isnan(got) & np.isnan(w)))
                if diff.any():
                    r, c = np.argwhere(diff)[0]
                    raise AssertionError(f"{what} group {g}: {int(diff.sum())} elements differ from the oracle, first "
                                         f"[{r}, {c}] got {got[r, c]!r} want {w[r, c]!r}")
            if not cell.sharded:
                K.check_against_float64(got_groups, cell.key, t, what)
                bad_total += bad
                assert op.plan.read_bad_ids() == bad_total, what
        del op


def test_caller_arena_that_is_too_small_is_refused(oracle):
    """``arena=``: a caller-owned arena below the request's size is a clear error, before any kernel touches it; the
    same request then runs into one of the right size."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    cell = CELLS[0]
    case = K.build_case(*cell.key)
    dev = torch.device("cuda", 0)
    d_tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    op = FeatureColumnProcess(case.spec, 0)
    inputs, symbols = case.requests[1]
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    need = max(op.plan.arena_bytes(shapes, symbols), 128)
    small = torch.full((need - 4,), 0xFF, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="arena"):
        op(d_blob, offsets, shapes, d_tabs, symbols, arena=small)
    with pytest.raises(ValueError, match="arena"):
        op.groups_only(d_blob, offsets, shapes, d_tabs, symbols, arena=small.view(torch.int32)[:1])
    torch.cuda.synchronize()
    assert bool((small == 0xFF).all())                          # nothing was written into it
    arena = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    got = op.groups_only(d_blob, offsets, shapes, d_tabs, symbols, arena=arena)
    torch.cuda.synchronize()
    want, _ = oracle.process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, case.tables, symbols)
    for g, w in zip(got, want):
        assert g.data_ptr() >= arena.data_ptr() and np.array_equal(g.cpu().numpy(), w)
