"""The plain dense kernel (fcp_dense_kernel_plain) against the generic dense kernel and a NumPy restatement.

Every cell (tests/dense_plain_cases.py) runs the same requests through two plans of one spec: one created as it ships —
the requests must report the plain front (fcp_plan_last_dense_front) — and one created with FCP_DIAG=dense_generic, whose
requests must report the generic front.  Both report the same launch (FCP_LAUNCH_DENSE, V 4, R 4, block count, store
policy), write the same bit patterns into arenas pre-filled with 0xFF bytes, equal the NumPy restatement bit for bit, and
count the same bad ids.  The gate test runs one plan per disqualifier: the generic front is reported and the arena equals,
byte for byte, that of the same plan created with FCP_DIAG=dense_generic."""
import os

import numpy as np
import pytest

import dense_plain_cases as D

pytestmark = pytest.mark.gpu

STORES = ("nt", "sc1_nt", "plain")


def _diag(monkeypatch, *keys, drop=("dense_generic", "wide_rows")):
    kept = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] not in drop]
    monkeypatch.setenv("FCP_DIAG", ",".join(kept + list(keys)))


def _blocks(spec, rows):
    nspans = (spec.group_width(0) // 4 + 63) // 64
    return (8 * ((nspans + 7) // 8) if nspans >= 8 else nspans) * ((rows + 15) // 16)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _ops(monkeypatch, spec, store, extra_diag=()):
    """(plan as it ships, the same plan kept on the generic kernel)"""
    from recom_amd.ops import FeatureColumnProcess
    if store == "nt":
        monkeypatch.delenv("FCP_STORE_THROUGH_BYTES", raising=False)
    else:
        monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    _diag(monkeypatch, *extra_diag)
    shipped = FeatureColumnProcess(spec, 0)
    _diag(monkeypatch, "dense_generic", *extra_diag)
    generic = FeatureColumnProcess(spec, 0)
    _diag(monkeypatch)
    return shipped, generic


@pytest.mark.parametrize("count_bad", (True, False), ids=("count", "nocount"))
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("width", sorted(D.WIDTHS))
def test_plain_kernel_equals_generic_and_numpy(monkeypatch, width, store, count_bad):
    import torch
    from recom_amd.ops import concat_inputs
    case = D.build_case(width, count_bad)
    spec = case.spec
    dev = torch.device("cuda", 0)
    d_tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    ops = _ops(monkeypatch, spec, store)
    nbytes = max(ops[0].plan.arena_bytes(concat_inputs(D.make_inputs(spec, r, 0))[2], None) for r in D.ROWS)
    # `sc1_nt`: a ring of three arenas (the plan remembers two); `plain`: one arena, reused; `nt`: a ring as well
    arenas = [[torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if store == "plain" else 3)] for _ in ops]
    bad_total = 0
    for t, rows in enumerate(D.ROWS):
        inputs = D.make_inputs(spec, rows, 100 * t + rows)
        blob, offsets, shapes = concat_inputs(inputs)
        d_blob = torch.from_numpy(blob).to(dev)
        want, bad = D.restate(spec, case.tables, inputs, rows)
        assert bad > 0
        bad_total += bad
        got = []
        for which, (op, ring, front) in enumerate(zip(ops, arenas, ("plain", "generic"))):
            what = (width, store, count_bad, rows, front)
            arena = ring[t % len(ring)]
            arena.fill_(0xFF)
            out = op(d_blob, offsets, shapes, d_tabs, None, arena=arena)
            torch.cuda.synchronize()
            assert op.plan.last_dense_front() == front, what
            launch = op.plan.last_launch()
            assert launch == dict(launch, kernel="dense", vec=4, rows_per_wave=4, wide_rows=False, shard_world=1, ragged_blocks=0,
                                  dense_blocks=_blocks(spec, rows),
                                  store=store if not (store == "plain" and t == 0) else "sc1_nt"), what
            g = _bits(out.groups[0])
            assert g.shape == want.shape, what
            diff = g != want.view(np.uint32)
            if diff.any():
                r, c = np.argwhere(diff)[0]
                raise AssertionError(f"{what}: {int(diff.sum())} elements differ from the NumPy restatement, first [{r}, {c}] "
                                     f"got {g[r, c]:#x} want {want.view(np.uint32)[r, c]:#x}")
            # nothing outside the group was written
            tail = arena[out.groups[0].numel() * 4:]
            assert bool((tail == 0xFF).all()), what
            assert op.plan.read_bad_ids() == (bad_total if count_bad else 0), what
            got.append(g)
        assert np.array_equal(got[0], got[1]), (width, store, rows)


def test_image_follows_new_shapes_resident_shapes_and_a_table_rebind(monkeypatch):
    """Descriptor slots: new shapes install a span image, resident shapes reuse it, and binding one table at another
    address rewrites the images of the resident slots — the next request of a resident shape reads the new table."""
    import torch
    from recom_amd.ops import concat_inputs
    case = D.build_case("mixed", True)
    spec = case.spec
    dev = torch.device("cuda", 0)
    tables = [t.copy() for t in case.tables]
    d_tabs = [torch.from_numpy(t).to(dev) for t in tables]
    ops = _ops(monkeypatch, spec, "nt")

    def run(rows, seed):
        inputs = D.make_inputs(spec, rows, seed)
        blob, offsets, shapes = concat_inputs(inputs)
        d_blob = torch.from_numpy(blob).to(dev)
        want, _ = D.restate(spec, tables, inputs, rows)
        for op, front in zip(ops, ("plain", "generic")):
            out = op(d_blob, offsets, shapes, d_tabs, None)
            torch.cuda.synchronize()
            assert op.plan.last_dense_front() == front, (rows, seed, front)
            assert np.array_equal(_bits(out.groups[0]), want.view(np.uint32)), (rows, seed, front)

    run(64, 1)
    run(96, 2)            # new shapes: a second slot
    run(64, 3)            # resident shapes, other ids
    for k in (1, len(tables) - 1):    # two tables move (and change): every resident image names them
        tables[k] = -tables[k] + np.float32(1.0)
        d_tabs = list(d_tabs)
        d_tabs[k] = torch.from_numpy(tables[k]).to(dev)
        run(96, 4 + k)
        run(64, 5 + k)


GATE_CASES = ("passthrough", "id_transform", "two_groups", "world2", "wide_rows", "bf16", "vec2", "rows63", "boundaries",
              "per_column", "pooled", "external")


def _gate_case(which):
    """(spec, tables, rows, extra FCP_DIAG keys, symbols) — the one-span-plus-a-slot plan with ONE disqualifier."""
    import dataclasses
    from recom_amd.plan import (COMBINER_SUM, FORM_EXTERNAL, FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE, IDS_F32_BUCKETIZE, IDS_I32,
                                LAYOUT_PER_COLUMN, ROWS_FROM_GROUP, ROWS_FROM_INPUT_DIM0, ROWS_FROM_SYMBOL, SEG_CSR_I32, SEG_NONE,
                                XFORM_FILTER, ColumnSpec)
    base = D.build_case("span_plus_slot", True)
    spec = dataclasses.replace(base.spec, columns=[dataclasses.replace(c) for c in base.spec.columns],
                               host_input_ranks=list(base.spec.host_input_ranks),
                               host_input_elem_sizes=list(base.spec.host_input_elem_sizes))
    tables, rows, diag, symbols = list(base.tables), 64, (), None
    n = len(spec.columns)
    rng = np.random.default_rng(5)

    def new_table(vocab, dim):
        tables.append(rng.standard_normal((vocab, dim)).astype(np.float32))
        spec.n_device_inputs = len(tables)
        return len(tables) - 1

    def new_host(rank, esz):
        spec.host_input_ranks.append(rank)
        spec.host_input_elem_sizes.append(esz)
        return len(spec.host_input_ranks) - 1

    if which == "passthrough":
        i = new_host(2, 4)
        spec.columns.append(ColumnSpec(FORM_PASSTHROUGH, 8, 0, 0, IDS_I32, -1, i, -1, SEG_NONE, 1, ROWS_FROM_INPUT_DIM0, i, None, 0, n))
    elif which == "id_transform":
        spec.columns[0] = dataclasses.replace(spec.columns[0], xform_mode=XFORM_FILTER, xform_lo=(0,), xform_hi=(3,))
    elif which == "two_groups":
        spec.n_groups = 2
        spec.columns.append(D.gather(8, 11, IDS_I32, new_table(11, 8), new_host(1, 4), 0, group=1))
    elif which == "world2":
        spec = spec.with_shard(0, 2)
        tables = [np.ascontiguousarray(t[0::2]) for t in tables]
    elif which == "wide_rows":
        diag = ("wide_rows",)
    elif which == "bf16":
        spec = spec.with_out_dtype("bf16")
    elif which == "vec2":
        spec.columns.append(D.gather(6, 11, IDS_I32, new_table(11, 6), new_host(1, 4), n))
    elif which == "rows63":
        rows = 63
    elif which == "boundaries":
        k = next(k for k, c in enumerate(spec.columns) if c.id_source == IDS_F32_BUCKETIZE)
        spec.columns[k] = dataclasses.replace(spec.columns[k], boundaries=np.asarray([0.0, 1.0, 3.0, 7.5, 20.0], np.float32))
    elif which == "per_column":
        spec = spec.with_layout(LAYOUT_PER_COLUMN)
    elif which == "pooled":
        spec.n_symbols = 1
        symbols = np.asarray([rows], np.int32)
        spec.columns.append(ColumnSpec(FORM_SEGMENT_REDUCE, 8, 11, COMBINER_SUM, IDS_I32, new_table(11, 8), new_host(1, 4),
                                       new_host(1, 4), SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None, 0, n))
    elif which == "external":
        spec.columns.append(ColumnSpec(FORM_EXTERNAL, 4, rows_source=ROWS_FROM_GROUP, concat_slot=n))
    spec.validate()
    return spec, tables, rows, diag, symbols


def _gate_inputs(spec, rows, which):
    from recom_amd.plan import FORM_GATHER, FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE
    rng = np.random.default_rng(11)
    gathers = iter(D.make_inputs(spec, rows, 7))
    inputs = []
    for c in spec.columns:
        if c.form == FORM_GATHER:
            inputs.append(next(gathers))
        elif c.form == FORM_PASSTHROUGH:
            inputs.append(rng.standard_normal((rows, c.dim)).astype(np.float32))
        elif c.form == FORM_SEGMENT_REDUCE:
            lens = rng.integers(0, 4, rows)
            inputs.append(rng.integers(0, c.vocab, int(lens.sum())).astype(np.int32))
            inputs.append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    return inputs


@pytest.mark.parametrize("which", GATE_CASES)
def test_gate_keeps_every_other_plan_on_the_generic_kernel(monkeypatch, which):
    import torch
    from recom_amd.ops import concat_inputs
    spec, tables, rows, diag, symbols = _gate_case(which)
    dev = torch.device("cuda", 0)
    d_tabs = [torch.from_numpy(t).to(dev) for t in tables]
    ops = _ops(monkeypatch, spec, "nt", diag)
    inputs = _gate_inputs(spec, rows, which)
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    nbytes = max(ops[0].plan.arena_bytes(shapes, symbols), 128)
    got = []
    for op in ops:
        arena = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        op(d_blob, offsets, shapes, d_tabs, symbols, arena=arena)
        torch.cuda.synchronize()
        assert op.plan.last_dense_front() == "generic", which
        assert op.plan.last_launch()["dense_blocks"] > 0, which
        got.append(arena.cpu().numpy())
    assert np.array_equal(got[0], got[1]), which
    assert not bool((got[0] == 0xFF).all()), which
    if which == "rows63":     # the plan itself qualifies: one more row and the same plan takes the plain kernel
        inputs = _gate_inputs(spec, 64, which)
        blob, offsets, shapes = concat_inputs(inputs)
        want, _ = D.restate(spec, tables, inputs, 64)
        for op, front in zip(ops, ("plain", "generic")):
            out = op(torch.from_numpy(blob).to(dev), offsets, shapes, d_tabs, None)
            torch.cuda.synchronize()
            assert op.plan.last_dense_front() == front
            assert np.array_equal(_bits(out.groups[0]), want.view(np.uint32))


def test_front_query_before_the_first_request_and_argument_checks():
    import ctypes as C
    from recom_amd import lib
    from recom_amd.ops import Plan
    plan = Plan(D.build_case("one_span").spec, 0)
    assert plan.last_dense_front() == "none"
    L = lib.load()
    v = C.c_int32()
    assert L.fcp_plan_last_dense_front(None, C.byref(v)) == lib.FCP_ERR_INVALID_ARGUMENT
    assert L.fcp_plan_last_dense_front(plan.handle, None) == lib.FCP_ERR_INVALID_ARGUMENT

