"""The any-order flag and the stop event through the launch every variant unit shares (fcp_klaunch,
recom_amd/csrc/fcp_fused_launch.h), for the five variants beside float32: weighted, narrow bf16, 16-bit fp16 tables, q8
tables, mixed tables.

One plan per variant, the smallest that reaches the variant's hybrid kernel (the weighted variant has none: its ragged
kernel): a plain gather of dim 8 in one concat group, a pooled column of dim 4 with CSR offsets in another (no segment-id
pre-pass in front of the fused kernel), 8 rows, V = 4.  Three requests of the same shapes and different ids, back to back on
the current stream, into three arenas filled with 0xFF: the first installs the descriptors and its launch carries their
stop event, the later ones find the shapes resident.  Once in stream order and once with the inputs-ready request order,
under which every launch also carries the any-order flag (blobs and arenas are complete before the first request: the
promise holds).  After one synchronise the arenas of the two runs are equal byte for byte and the groups equal the
expectation bit for bit; fcp_plan_last_launch names the variant's kernel in both runs.

The expectation is the C oracle's on the float32 values the tables hold (rounded once for bf16 output).  The C oracle has
no per-id weights: the weighted plan is checked against the float32 restatement of tests/weighted_bag_cases.py, as
tests/test_gpu_weighted_bags.py does."""
import dataclasses
import functools

import numpy as np
import pytest

import narrow_output_cases as N
import table_q8_cases as Q
import weighted_bag_cases as W
from recom_amd import synth
from recom_amd.plan import (COMBINER_MEAN, COMBINER_NONE, FORM_GATHER, FORM_SEGMENT_REDUCE, IDS_I32, IDS_I64, ROWS_FROM_IDS,
                            ROWS_FROM_SYMBOL, SEG_CSR_I32, SEG_NONE, ColumnSpec, PlanSpec)

pytestmark = pytest.mark.gpu

ROWS, VOCAB = 8, 37
DIMS = (8, 4)                                       # gather, pooled: V = 4
BAG_LENS = (0, 1, 2, 3, 1, 0, 4, 2)                 # the same in every request: the shapes do not change
N_REQUESTS = 3
VARIANTS = ("weighted", "narrow_bf16", "tab16_f16", "tabq8", "tabmix")
KERNEL = {"weighted": "ragged_weighted", "narrow_bf16": "hybrid_narrow", "tab16_f16": "hybrid_tab16", "tabq8": "hybrid_tabq8",
          "tabmix": "hybrid_tabmix"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _spec32(weighted: bool) -> PlanSpec:
    cols = [ColumnSpec(FORM_GATHER, DIMS[0], VOCAB, COMBINER_NONE, IDS_I32, 0, 0, -1, SEG_NONE, 1, ROWS_FROM_IDS, 0, None, 0, 0),
            ColumnSpec(FORM_SEGMENT_REDUCE, DIMS[1], VOCAB, COMBINER_MEAN, IDS_I64, 1, 1, 2, SEG_CSR_I32, 1, ROWS_FROM_SYMBOL, 0, None,
                       1, 0, weights_input=3 if weighted else -1)]
    spec = PlanSpec(cols, [1, 1, 1] + [1] * weighted, [4, 8, 4] + [4] * weighted, 2, n_groups=2, n_symbols=1)
    spec.validate()
    return spec


@functools.lru_cache(maxsize=None)
def _case(variant: str):
    """(spec, tables as the plan reads them, the float32 values they hold, requests): computed once per variant."""
    rng = np.random.default_rng(VARIANTS.index(variant))
    spec = _spec32(variant == "weighted")
    f32 = [rng.normal(0, 1, (VOCAB, d)).astype(np.float32) for d in DIMS]
    kinds = {"tab16_f16": ("f16", "f16"), "tabq8": ("q8", "q8"), "tabmix": ("f32", "q8")}.get(variant, ("f32", "f32"))
    tables, values = [], []
    for t, (kind, x) in enumerate(zip(kinds, f32)):
        if kind == "q8":
            tables.append(Q.draw_table(VOCAB, DIMS[t], 7 + t))
            values.append(Q.dequantize(tables[-1]))
        elif kind == "f16":
            tables.append(synth.table_patterns(x, "f16"))
            values.append(synth.table_values(tables[-1], "f16"))
        else:
            tables.append(x)
            values.append(x)
    if variant == "narrow_bf16":
        spec = spec.with_out_dtype("bf16")
    elif variant != "weighted":
        spec = spec.with_table_dtypes(kinds)
    nnz = sum(BAG_LENS)
    requests = []
    for _ in range(N_REQUESTS):
        inputs = [rng.integers(0, VOCAB, ROWS).astype(np.int32), rng.integers(0, VOCAB, nnz).astype(np.int64),
                  np.concatenate([[0], np.cumsum(BAG_LENS)]).astype(np.int32)]
        if variant == "weighted":
            inputs.append(rng.normal(1, 0.5, nnz).astype(np.float32))
        requests.append(inputs)
    assert not np.array_equal(requests[0][1], requests[1][1]) and not np.array_equal(requests[1][1], requests[2][1])
    return spec, tables, values, requests


def _expected(variant: str, oracle):
    """Per request, per group: the bytes the plan must write."""
    spec, _tables, values, requests = _case(variant)
    symbols = np.asarray([ROWS], np.int32)
    from recom_amd.ops import concat_inputs
    out = []
    for inputs in requests:
        if variant == "weighted":
            res = W.restate(spec, values, inputs, symbols)
            want, bad = res.groups, res.bad
        else:
            twin = dataclasses.replace(spec, out_dtype="f32", table_dtype="f32", table_dtypes=None)
            blob, offsets, shapes = concat_inputs(inputs)
            want, bad = oracle.process_feature_columns(twin.to_dict(), blob, offsets, shapes, values, symbols)
        assert bad == 0 and not any(np.isnan(w).any() for w in want)
        out.append([N.narrow(w, "bf16") if variant == "narrow_bf16" else np.ascontiguousarray(w, np.float32) for w in want])
    return out


def _device_table(torch, t, dev):
    if t.dtype == np.uint16:
        return torch.from_numpy(np.ascontiguousarray(t).view(np.int16)).to(dev).view(torch.float16)
    return torch.from_numpy(np.ascontiguousarray(t)).to(dev)


def _run(torch, variant: str, inputs_ready: bool):
    """Three requests back to back on the current stream, one synchronise behind them.  Returns the arenas and the groups
    (both as host bytes) and the launch reports."""
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec, tables, _values, requests = _case(variant)
    dev = torch.device("cuda", 0)
    symbols = np.asarray([ROWS], np.int32)
    d_tabs = [_device_table(torch, t, dev) for t in tables]
    op = FeatureColumnProcess(spec, 0)
    if inputs_ready:
        op.plan.set_inputs_ready(True)
    packed = [concat_inputs(inputs) for inputs in requests]
    assert all(np.array_equal(p[2], packed[0][2]) for p in packed)       # the same shapes: one descriptor install
    nbytes = max(op.plan.arena_bytes(packed[0][2], symbols), 128) + 256
    arenas = [torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev) for _ in requests]
    d_blobs = [torch.from_numpy(blob).to(dev) for blob, _, _ in packed]
    torch.cuda.synchronize()                                             # blobs complete, arenas unused: the inputs are ready
    outs, launches = [], []
    for (_, offsets, shapes), d_blob, arena in zip(packed, d_blobs, arenas):
        outs.append(op(d_blob, offsets, shapes, d_tabs, symbols, arena=arena))
        launches.append(op.plan.last_launch())
    torch.cuda.synchronize()
    groups = [[g.contiguous().view(torch.uint8).cpu().numpy() for g in out.groups] for out in outs]
    assert op.plan.read_bad_ids() == 0
    return [a.cpu().numpy() for a in arenas], groups, launches


@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_launch_carries_stop_event_and_any_order_flag(torch_cuda, oracle, variant):
    want = _expected(variant, oracle)
    runs = {ready: _run(torch_cuda, variant, ready) for ready in (False, True)}
    for ready, (arenas, groups, launches) in runs.items():
        for t, launch in enumerate(launches):
            what = (variant, "inputs_ready" if ready else "stream_order", t)
            assert launch["kernel"] == KERNEL[variant] and launch["vec"] == 4, (what, launch)
            assert launch["ragged_blocks"] >= 1 and (variant == "weighted" or launch["dense_blocks"] >= 1), (what, launch)
            assert launch["segment_offsets"] == "none", (what, launch)   # nothing queued in front of the fused kernel
            for g, w in enumerate(want[t]):
                got = groups[t][g].reshape(ROWS, -1)
                assert got.tobytes() == w.tobytes(), (what, "group", g, got.view(w.dtype), w)
            assert (arenas[t][-256:] == 0xFF).all(), (what, "bytes beyond the request's arena were written")
    for t in range(N_REQUESTS):
        assert runs[False][0][t].tobytes() == runs[True][0][t].tobytes(), (variant, t, "the two request orders wrote different arenas")
