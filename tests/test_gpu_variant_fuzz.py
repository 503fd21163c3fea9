"""Random plans through the fused-kernel variants beside float32 on the GPU: narrow output (bf16 / fp16; kernels:
recom_amd/csrc/fcp_narrow.hip), plan-wide bf16 / fp16 tables (fcp_tables16.hip), q8 tables (fcp_tables_q8.hip) and per-input
table formats (fcp_tables_mixed.hip).  The plans are tests/test_gpu_fuzz.py::random_model's — five forms, three id sources with
every bucketize tier, hashing, SELECT / FILTER, ids outside the vocabulary, three segment encodings with folded reshapes,
several concat groups with their own batches, V of 4 / 2 / 1, hundreds of columns, bags of hundreds of ids — which the
variants' own tests, built by hand, never combine.  Cases: tests/variant_fuzz_cases.py; that its fixed seed list reaches
these combinations is asserted on the CPU (tests/test_variant_fuzz_host.py).

One plan per test, three requests in stream order on the current stream, each into a caller's arena filled with 0xFF.  The
yardstick is exact: the C oracle's result for the float32 plan on the decoded tables, rounded once for narrow output — bit
patterns equal wherever the expectation is not NaN.  Private streams, the inputs-ready request order, the stager and
sharding are not run here (tests/test_gpu_variant_launch.py pins the launch tail the serving modes share).

The weighted variant is no target: random_model draws no per-id weights, and the C oracle has none.

FCP_VARIANT_FUZZ_SEEDS=<n> (from FCP_VARIANT_FUZZ_SEED0, default 0): longer soak runs over the seeds of that range that have
a lookup column and more than one table kind; the census holds for the default list only."""
import os

import numpy as np
import pytest

import narrow_output_cases as N
import table16_cases as T16
import variant_fuzz_cases as F

pytestmark = pytest.mark.gpu


def _seeds():
    n = os.environ.get("FCP_VARIANT_FUZZ_SEEDS")
    if n is None:
        return F.SEEDS
    first = int(os.environ.get("FCP_VARIANT_FUZZ_SEED0", "0"))
    return tuple(s for s in range(first, first + int(n)) if F.eligible(s))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _table_kinds(seed, target):
    n = F.plan(seed)[0].n_device_inputs
    return F.mixed_kinds(seed) if target == "tabmix" else (F.PLAN_WIDE.get(target, "f32"),) * n


def _device_table(torch, t, kind, dev):
    """The table on the device in its kind: 16-bit patterns as torch.bfloat16 / torch.float16 (the op checks the torch dtype,
    the bytes are what counts), q8 rows as uint8."""
    t = np.array(t, copy=True)          # (the cases' arrays are read-only and shared)
    if kind in ("bf16", "f16"):
        assert t.dtype == np.uint16
        return torch.from_numpy(t.view(np.int16)).to(dev).view(torch.bfloat16 if kind == "bf16" else torch.float16)
    assert t.dtype == (np.uint8 if kind == "q8" else np.float32)
    return torch.from_numpy(t).to(dev)


def _first_difference(got, want, nan_got, nan_want):
    """(row, element) of the first element that differs — patterns where the expectation is not NaN, NaN where it is — or
    None"""
    diff = np.where(nan_want, ~nan_got, got != want)
    return tuple(int(v) for v in np.argwhere(diff)[0]) if diff.any() else None


def _assert_group(torch, spec, target, group, tensor, want32, what):
    """One concat group against the expectation, with the column of the first differing element in the message."""
    dtype = F.NARROW.get(target)
    if dtype is None:
        assert tensor.dtype == torch.float32, (what, tensor.dtype)
        got = tensor.contiguous().cpu().numpy()
        want = np.ascontiguousarray(want32, np.float32)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        g, w = got.view(np.uint32), want.view(np.uint32)
        first = _first_difference(g, w, np.isnan(got), np.isnan(want))
        check, width = (lambda: T16.assert_same_bits(got, want, what)), 10
    else:
        assert tensor.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float16), (what, tensor.dtype)
        g = tensor.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        w = N.narrow(want32, dtype)
        assert g.shape == w.shape, (what, g.shape, w.shape)
        first = _first_difference(g, w, N.is_nan16(g, dtype), N.is_nan16(w, dtype))
        check, width = (lambda: N.assert_same16(g, want32, dtype, what)), 6
    if first is not None:
        k, form, ids, seg, kind = F.column_at(spec, group, first[1])
        where = (f"{what}: first differing element [{first[0]}, {first[1]}] lies in column {k} (form {form}, id source {ids}, "
                 f"seg kind {seg}, table kind {kind}, dim {spec.columns[k].dim}, vocab {spec.columns[k].vocab}): "
                 f"got {int(g[first]):#0{width}x} want {int(w[first]):#0{width}x}")
        try:
            check()
        except AssertionError as e:
            raise AssertionError(f"{where}\n{e}") from None
        raise AssertionError(where)
    check()


@pytest.mark.parametrize("target", F.TARGETS)
@pytest.mark.parametrize("seed", _seeds())
def test_random_plan_through_variant(torch_cuda, seed, target):
    torch = torch_cuda
    from recom_amd.ops import FeatureColumnProcess
    spec, tables, _decoded = F.twin(seed, target)
    kinds = _table_kinds(seed, target)
    dev = torch.device("cuda", 0)
    d_tabs = [_device_table(torch, t, k, dev) for t, k in zip(tables, kinds)]
    op = FeatureColumnProcess(spec, 0)
    assert op.plan.out_dtype() == F.NARROW.get(target, "f32"), (seed, target)
    assert op.plan.table_dtype() == ("mixed" if target == "tabmix" else F.PLAN_WIDE.get(target, "f32")), (seed, target)
    bad_total, fused = 0, 0
    for t, r in enumerate(F.requests(seed)):
        what = f"seed {seed} target {target} request {t} (batches {r.batches})"
        want, want_bad = F.expectation32(seed, target, t)
        d_blob = torch.from_numpy(r.blob).to(dev) if r.blob.size else torch.empty(0, dtype=torch.int8, device=dev)
        need = op.plan.arena_bytes(r.shapes, r.symbols)
        arena = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        arena.fill_(0xFF)
        out = op(d_blob, r.offsets, r.shapes, d_tabs, r.symbols, arena=arena)
        torch.cuda.synchronize()
        launch = op.plan.last_launch()
        assert len(out.groups) == len(want) == spec.n_groups, what
        for g, w in enumerate(want):
            assert tuple(out.groups[g].shape) == w.shape, (what, "group", g, tuple(out.groups[g].shape), w.shape)
            _assert_group(torch, spec, target, g, out.groups[g], w, f"{what} group {g} [{launch['kernel']}, {launch['segment_offsets']}]")
        assert bool((arena[need:] == 0xFF).all()), (what, "bytes beyond the request's arena were written")
        bad_total += want_bad
        assert op.plan.read_bad_ids() == bad_total, (what, op.plan.read_bad_ids(), bad_total)
        if launch["kernel"] != "none":           # a fused kernel ran: the variant's, not the float32 unit's
            assert launch["kernel"].endswith(F.SUFFIX[target]) and launch["vec"] == F.vec_of(spec), (what, launch)
            fused += 1
    assert fused > 0, (seed, target, "no request reached a fused kernel")
