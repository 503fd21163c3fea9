"""fcp_outputs_compare on the GPU, against the NumPy restatement of outputs_compare_cases.

The edge matrix goes through raw strided views: two torch tensors are the arenas, the pointer, stride and shape arrays are built
by hand — every dim x row count x layout of outputs_compare_cases, all nine pairs of element kinds, side B's layouts rotated
against side A's, every special pair at every corner of a column, bases at odd elements.  Counts, first rows and maxima equal the
restatement bit for bit, the two sums lie within elems * 2^-52 of it (relative; equal with one finite pair), out[n] is the fold
of the restated column records under the same bound, two calls leave the same bytes, a used workspace changes nothing, and
nothing but `out` and the workspace is written.  (The calls from another stream, and the compare enqueued behind its two
requests on a stream of its own, are in tests/test_zzz_gpu_outputs_compare_stream.py.)

The file sorts behind tests/test_z_gpu_private_streams.py, as the project's stream tests do.  It takes no stream from torch's pool,
yet run as a whole in front of that file it made one of its tests fail
(test_supervisor_re_admits_a_demoted_caller_when_the_private_streams_win_again: the caller stayed demoted), on every one of four
runs; no single test of this file in front of that test does, and that file alone passes with this library as with the
parent's.  What the file leaves behind in the process that the supervisor's timing windows see was not found; behind
the private-stream tests it disturbs nothing.

Through plans: one request of the variant cases (kernel_variant_cases, narrow_output_cases.DISCRIMINATION_KEYS: a dense, a
ragged — two groups whose rows the symbols give, 31 and 21 — and a hybrid plan) is served by the float32 plan and by its bf16,
fp16, q8 and mixed twins on converted tables, by the narrow-output twins and by the per-column layout, and
ops.compare_outputs is held to the restatement applied to the two results column by column."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import kernel_variant_cases as K
import narrow_output_cases as N
import outputs_compare_cases as OC
from recom_amd.plan import FORM_PASSTHROUGH, LAYOUT_PER_COLUMN

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A       # int64 words around out and the workspace


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _torch_elems(torch, arena: np.ndarray, dev):
    """a NumPy arena of uint32 / uint16 patterns as a device tensor of int32 / int16 (the bytes are what counts)"""
    return torch.from_numpy(arena.view(np.int32 if arena.dtype == np.uint32 else np.int16).copy()).to(dev)


class Buffers:
    """out [n + 1] and a workspace, each between two guard blocks of 32 words"""

    def __init__(self, torch, L, n, dev):
        self.n = n
        self.ws_words = int(L.fcp_outputs_compare_workspace_bytes(n)) // 8
        self.buf = torch.full((32 + 8 * (n + 1) + 32 + self.ws_words + 32,), GUARD, dtype=torch.int64, device=dev)
        self.out = self.buf[32:32 + 8 * (n + 1)]
        self.ws = self.buf[32 + 8 * (n + 1) + 32:][:self.ws_words]

    def records(self) -> np.ndarray:
        return np.frombuffer(self.out.cpu().numpy().tobytes(), OC.RECORD)

    def guards_intact(self) -> bool:
        b = self.buf.cpu().numpy()
        o = 32 + 8 * (self.n + 1)
        return bool((b[:32] == GUARD).all() and (b[o:o + 32] == GUARD).all() and (b[o + 32 + self.ws_words:] == GUARD).all())


def _side_arrays(side, tensor):
    eb = OC.ELEM_BYTES[side["kind"]]
    return [tensor.data_ptr() + off * eb for off, _ in side["where"]], [stride for _, stride in side["where"]]


@pytest.mark.parametrize("kinds", OC.KIND_PAIRS, ids=["-".join(p) for p in OC.KIND_PAIRS])
def test_edge_matrix(torch_cuda, kinds):
    torch = torch_cuda
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    m = OC.edge_matrix(*kinds)
    n = len(m["columns"])
    ta, tb = _torch_elems(torch, m["a"]["arena"], dev), _torch_elems(torch, m["b"]["arena"], dev)
    pa, sa = _side_arrays(m["a"], ta)
    pb, sb = _side_arrays(m["b"], tb)
    shapes = [v for rd in m["columns"] for v in rd]
    main = torch.cuda.current_stream(dev).cuda_stream

    def run(buffers, stream):
        status = OC.call(L, pa, sa, kinds[0], pb, sb, kinds[1], shapes, n, buffers.out.data_ptr(), buffers.ws.data_ptr(), 0, stream)
        assert status == 0, L.fcp_last_error().decode()

    first, second, third = (Buffers(torch, L, n, dev) for _ in range(3))
    run(first, main)
    run(second, main)
    torch.cuda.synchronize()
    got = first.records()
    OC.assert_records(got, m["want"], kinds, m["finite_pairs"])
    # out[n] is also the fold of what the DEVICE wrote for the columns (counts and maxima exactly)
    OC.assert_records(got[-1:], OC.restate_total(got[:-1]).reshape(1), (kinds, "total of the device's columns"))
    assert second.out.cpu().numpy().tobytes() == first.out.cpu().numpy().tobytes(), "two calls, different bytes"
    # the same workspace again, right behind on the same stream: its old content means nothing
    run(third, main)
    run(third, main)
    torch.cuda.synchronize()
    assert third.out.cpu().numpy().tobytes() == got.tobytes(), "a used workspace, different bytes"
    assert first.out.cpu().numpy().tobytes() == got.tobytes()
    for b in (first, second, third):
        assert b.guards_intact()
    for t, side_ in ((ta, m["a"]), (tb, m["b"])):
        assert t.cpu().numpy().tobytes() == side_["arena"].tobytes(), "an arena changed"


def _small_columns(n: int, kinds, seed: int):
    """n small columns of varying shape in two packed arenas: (element arrays a, b, shapes)"""
    rng = np.random.default_rng(seed)
    a, b, shapes = [], [], []
    for k in range(n):
        rows, dim = (k * 5 + 1) % 4, (1, 2, 3, 4, 6, 8)[k % 6]
        x = OC.widened(OC.encode(rng.standard_normal((rows, dim)), kinds[0]), kinds[0])
        y = x if k % 3 == 0 else x + np.float32(0.125) * (rng.random((rows, dim)) < 0.5)
        if kinds[0] != kinds[1] and k % 3 == 0:
            x = y = (np.round(x * 8) / 8).astype(np.float32)
        a.append(OC.encode(x, kinds[0]))
        b.append(OC.encode(y, kinds[1]))
        shapes += [rows, dim]
    return a, b, shapes


def _pack(torch, elems, kind, dev):
    """columns back to back (stride = dim): (device tensor, pointers, strides)"""
    dt = np.uint32 if kind == "f32" else np.uint16
    flat = np.concatenate([e.view(dt).reshape(-1) for e in elems] + [np.zeros(1, dt)])
    t = _torch_elems(torch, flat, dev)
    offs = np.concatenate([[0], np.cumsum([e.size for e in elems])])[:-1]
    return t, [t.data_ptr() + int(o) * flat.itemsize for o in offs], [e.shape[1] for e in elems]


@pytest.mark.parametrize("n", (0, 1, 2, 65, 1000, 4100))
def test_column_counts(torch_cuda, n):
    """n_columns 0 (one zero record, first_differ_row -1), 1 and 2 (T = 64), 65, 1000 (T = 5) and 4100 (T = 1)"""
    torch = torch_cuda
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    kinds = ("f32", "bf16") if n % 2 else ("f16", "f32")
    assert OC.tiles_per_column(n) == {0: 1, 1: 64, 2: 64, 65: 64, 1000: 5, 4100: 1}[n]
    a, b, shapes = _small_columns(n, kinds, n)
    ta, pa, sa = _pack(torch, a, kinds[0], dev)
    tb, pb, sb = _pack(torch, b, kinds[1], dev)
    bufs = [Buffers(torch, L, n, dev) for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    for buf in bufs:
        if n == 0 and buf is bufs[1]:      # null arrays are as good as empty ones
            status = OC.call(L, None, None, kinds[0], None, None, kinds[1], None, 0, buf.out.data_ptr(), buf.ws.data_ptr(), 0, stream)
        else:
            status = OC.call(L, pa, sa, kinds[0], pb, sb, kinds[1], shapes, n, buf.out.data_ptr(), buf.ws.data_ptr(), 0, stream)
        assert status == 0, L.fcp_last_error().decode()
    torch.cuda.synchronize()
    want = OC.restate(a, kinds[0], b, kinds[1])
    got = bufs[0].records()
    OC.assert_records(got, want, n)
    if n == 0:
        assert got.tobytes() == np.array([(0, 0, 0, -1, 0.0, 0.0, 0.0, 0.0, 0)], OC.RECORD).tobytes()
    elif n >= 65:
        assert want["differ"][-1] > 0 and (want["elems"][:-1] == 0).any()
    assert bufs[1].out.cpu().numpy().tobytes() == got.tobytes()
    assert all(buf.guards_intact() for buf in bufs)


# ---- through plans ------------------------------------------------------------------------------------------------------------
KEYS = N.DISCRIMINATION_KEYS
REQUEST = 1                      # 65 rows; 31 and 21 rows in the ragged plan's two groups; 63 rows
TWINS = ("bf16", "f16", "q8", "mixed", "out_bf16", "out_f16", "per_column")


def _elems_of(torch, outputs, k):
    """column k of a result as the restatement takes it: (element array, kind)"""
    col = outputs.column(k)
    if col.dtype == torch.float32:
        return col.cpu().numpy(), "f32"
    return col.cpu().contiguous().view(torch.int16).numpy().view(np.uint16), "bf16" if col.dtype == torch.bfloat16 else "f16"


def _restate_outputs(torch, a, b):
    n = len(a.output_ptrs)
    ea, eb = [_elems_of(torch, a, k) for k in range(n)], [_elems_of(torch, b, k) for k in range(n)]
    ka, kb = (ea[0][1], eb[0][1]) if n else ("f32", "f32")
    return OC.restate([e for e, _ in ea], ka, [e for e, _ in eb], kb)


@pytest.fixture(scope="module")
def served(torch_cuda):
    """per key: the request on the device, the float32 plan's result, and a function that serves a twin"""
    torch = torch_cuda
    from recom_amd import tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    cache = {}

    def get(key):
        if key in cache:
            return cache[key]
        case = K.build_case(*key)
        spec32 = case.spec
        tabs32 = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in case.tables]
        inputs, symbols = case.requests[REQUEST]
        blob, offsets, shapes = concat_inputs(inputs)
        d_blob = torch.from_numpy(blob).to(dev)
        ops = {}

        def serve(twin, stream=None):
            if twin not in ops:
                if twin == "f32":
                    spec, tabs = spec32, tabs32
                elif twin in ("bf16", "f16", "q8"):
                    spec, tabs = spec32.with_table_dtype(twin), tables.convert_tables(spec32, tabs32, twin)
                elif twin == "mixed":
                    kinds = [("f32", "bf16", "f16", "q8")[i % 4] for i in range(len(tabs32))]
                    spec, tabs = spec32.with_table_dtypes(kinds), [t if k == "f32" else tables.convert(t, k) for t, k in zip(tabs32, kinds)]
                elif twin.startswith("out_"):
                    spec, tabs = spec32.with_out_dtype(twin[4:]), tabs32
                else:
                    spec, tabs = dataclasses.replace(spec32, layout=LAYOUT_PER_COLUMN), tabs32
                torch.cuda.synchronize()
                ops[twin] = (FeatureColumnProcess(spec, 0), tabs)
            op, tabs = ops[twin]
            return op(d_blob, offsets, shapes, tabs, symbols, stream=stream)

        cache[key] = (case, serve, serve("f32"))
        return cache[key]

    return get


@pytest.mark.parametrize("twin", TWINS)
@pytest.mark.parametrize("key", KEYS, ids=[k[0] for k in KEYS])
def test_plans(torch_cuda, served, key, twin):
    torch = torch_cuda
    from recom_amd import ops
    case, serve, ref = served(key)
    out = serve(twin)
    got = ops.compare_outputs(ref, out)
    want = _restate_outputs(torch, ref, out)
    records = np.concatenate([np.asarray(got.columns).view(OC.RECORD).reshape(-1), np.asarray(got.total).view(OC.RECORD).reshape(1)])
    OC.assert_records(records, want, (key, twin))
    if twin == "per_column":       # the same values in another layout: strides differ, bits do not
        assert got.identical and not np.array_equal(ref.output_row_strides, out.output_row_strides)
        assert got.rel_rms() == 0.0
    else:
        assert not got.identical and 0.0 < got.rel_rms() < 0.05, got.rel_rms()
    # the other way round: side A narrow or on compact tables, side B float32
    back = ops.compare_outputs(out, ref)
    assert [int(v) for v in back.columns.differ] == [int(v) for v in got.columns.differ]
    if twin == "bf16":
        # every lookup column whose float32 output is not all zeros has read table rows that are not bf16-exact (drawn normal
        # values); PASSTHROUGH columns read no table
        for k, c in enumerate(case.spec.columns):
            if c.form == FORM_PASSTHROUGH:
                assert got.columns.differ[k] == 0, k
            elif np.any(ref.column(k).cpu().numpy() != 0):
                assert got.columns.differ[k] > 0, k
        assert key[0] == "ragged" or any(c.form == FORM_PASSTHROUGH for c in case.spec.columns)   # (the ragged case has none)


@pytest.mark.parametrize("key", KEYS, ids=[k[0] for k in KEYS])
def test_a_plan_against_itself(torch_cuda, served, key):
    torch = torch_cuda
    from recom_amd import ops
    case, serve, ref = served(key)
    same = ops.compare_outputs(ref, ref)
    assert same.identical and same.total.elems == sum(int(r) * int(d) for r, d in ref.output_shapes.reshape(-1, 2))
    assert same.total.sum_sq_err == 0.0 and same.total.max_abs_err == 0.0 and same.total.sum_sq_ref > 0.0
    again = ops.compare_outputs(ref, serve("f32"))         # a second arena, the same plan
    assert again.identical
