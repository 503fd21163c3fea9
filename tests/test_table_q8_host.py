"""8-bit row-quantised tables (FCP_FLAG_TABLES_Q8) without a GPU: the exactness of the dequantisation the GPU tests compare
with (tests/table_q8_cases.py) against quantized::embedding_bag_byte_unpack and rational arithmetic, the vocabulary and the
refusals through host-only plans and the Python mirror, table bytes and the placement gate, version-7 plan files through
both parsers, and the code object of fcp_tables_q8.hip against its float32 twins of fcp_kernels.hip."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kernel_variant_cases as K
import narrow_output_cases as N
import table_q8_cases as Q
from recom_amd import lib as _lib
from recom_amd import placement, plan_io, synth
from recom_amd.ops import Plan, concat_inputs
from recom_amd.plan import FLAG_TABLES_BF16, FLAG_TABLES_F16, FLAG_TABLES_Q8, PlanSpec, TablesQ8Unsupported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _specs():
    """A spread of existing plans: (name, spec, shapes, symbols) of one request each."""
    out = []
    for name, m in (("mixed", synth.model_mixed(batch=33, vocab=997)), ("s1", synth.model_s1(columns=6, batch=9)),
                    ("dlrm", synth.model_dlrm(batch=17)), ("ragged", synth.model_ragged(columns=5, batch=11, seg="indices"))):
        req = m.make_request(0)
        _, _, shapes = concat_inputs(req.inputs)
        out.append((name, m.spec, shapes, req.symbols))
    inputs, symbols = Q.xform_request()
    out.append(("xform", Q.xform_spec(), concat_inputs(inputs)[2], symbols))
    for key in N.DISCRIMINATION_KEYS:
        case = K.build_case(*key)
        inputs, symbols = case.requests[1]
        out.append(("-".join(map(str, key)), case.spec, concat_inputs(inputs)[2], symbols))
    return out


SPECS = _specs()


# ---- the value model ------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_dequantize_is_byte_unpack_on_arbitrary_bytes():
    """synth.dequantize_q8 against PyTorch-CPU's quantized::embedding_bag_byte_unpack, bit for bit, on drawn tables of dims
    1-64; and the two-rounding reading differs from both on 22-23 % of such elements (at least 0.15 is asserted)."""
    import torch
    op = getattr(getattr(torch.ops, "quantized", None), "embedding_bag_byte_unpack", None)
    total = differ = 0
    for dim in (1, 2, 3, 4, 6, 7, 12, 16, 33, 64):
        table = Q.draw_table(3000, dim, 700 + dim)
        got = Q.dequantize(table)
        assert got.dtype == np.float32 and got.shape == (3000, dim) and not np.isnan(got).any()
        if op is not None:
            want = op(torch.from_numpy(table)).numpy()
            assert np.array_equal(_bits(got), _bits(want)), dim
        two = Q.two_roundings(table)
        total += got.size
        differ += int((_bits(two) != _bits(got)).sum())
        # the layout is the prepacked tensor's: dim codes, scale, bias
        codes, scale, bias = synth.q8_fields(table)
        assert np.array_equal(Q.pack(codes, scale, bias), table)
    assert differ / total >= 0.15, differ / total
    if op is not None:      # and the field order of the tensor embedding_bag_byte_prepack returns
        w = torch.from_numpy(np.random.default_rng(1).standard_normal((50, 12)).astype(np.float32))
        packed = torch.ops.quantized.embedding_bag_byte_prepack(w)
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (50, 20)
        assert np.array_equal(_bits(Q.dequantize(packed.numpy())), _bits(op(packed).numpy()))


def test_dequantize_is_rational_arithmetic_on_the_edge_list_and_random_triples():
    """Every triple of the edge list and a few thousand random ones: synth.fma_f32 (round-to-odd in float64, then one cast)
    against exact rational arithmetic rounded once, to nearest-even, in integers.  NaN where that is NaN, bits elsewhere."""
    codes, scales, biases = Q.edge_triples()
    rng = np.random.default_rng(11)
    n = 3000
    r_scale = (rng.standard_normal(n) * np.exp(rng.normal(-5, 6, n))).astype(np.float32)
    r_bias = (rng.standard_normal(n) * np.exp(rng.normal(0, 6, n))).astype(np.float32)
    # (and biases within a few ulps of cancelling the product: the sums where a double rounding would show)
    r_code = rng.integers(0, 256, n)
    near = rng.random(n) < 0.3
    with np.errstate(all="ignore"):
        r_bias[near] = (-(r_code[near].astype(np.float32) * r_scale[near]) * (1 + rng.integers(-3, 4, int(near.sum())) * 2.0 ** -22)).astype(np.float32)
    codes = np.concatenate([codes, r_code])
    scales, biases = np.concatenate([scales, r_scale]), np.concatenate([biases, r_bias])
    got = synth.fma_f32(codes, scales, biases)
    want = np.asarray([Q.fma_exact(int(c), s, b) for c, s, b in zip(codes, scales, biases)], np.float32)
    nan = np.isnan(want)
    assert 0 < int(nan.sum()) < want.size // 2
    assert np.array_equal(np.isnan(got), nan)
    bad = np.flatnonzero(~nan & (_bits(got) != _bits(want)))
    assert bad.size == 0, [(int(codes[i]), float(scales[i]), float(biases[i]), float(got[i]), float(want[i])) for i in bad[:5]]
    # the named cases hold what they are named for
    f = lambda c, s, b: synth.fma_f32(np.asarray([c]), np.float32(s), np.float32(b))[0]      # noqa: E731
    assert f(2, Q.FLT_MAX, -Q.FLT_MAX) == np.float32(Q.FLT_MAX)            # the product overflows alone, the fused sum does not
    with np.errstate(all="ignore"):
        assert np.isinf(np.float32(2) * np.float32(Q.FLT_MAX))
    assert f(1, 2.0 ** -24, 1.0) == np.float32(1.0) and f(3, 2.0 ** -24, 1.0) == np.float32(1 + 2.0 ** -22)   # ties to even
    assert np.isnan(f(0, np.inf, 0.0)) and np.isnan(f(1, np.inf, -np.inf)) and f(1, np.inf, 1.0) == np.inf
    assert _bits(f(7, -0.0, -0.0))[()] == 0x80000000 and _bits(f(7, 0.0, -0.0))[()] == 0
    assert f(3, Q.SUBNORMAL, 0.0) == np.float32(3 * Q.SUBNORMAL)


def test_closed_form_q8_tables():
    for dim in (1, 3, 8, 64):
        t = synth.q8_table_numpy(5, 300, dim)
        assert t.dtype == np.uint8 and t.shape == (300, dim + 8)
        assert np.array_equal(t[[7, 250, 0]], synth.q8_rows(5, np.asarray([7, 250, 0]), dim))
        assert np.array_equal(synth.q8_table_torch(5, 300, dim, "cpu").numpy(), t)
        x = synth.dequantize_q8(t)
        assert np.isfinite(x).all() and len(np.unique(x)) > x.size // 2
        assert ((_bits(Q.two_roundings(t)) != _bits(x)).mean() > 0.05)
    for build in (lambda dt: synth.model_s2(columns=4, vocab=50, batch=8, table_dtype=dt),
                  lambda dt: synth.model_s1(columns=4, batch=8, table_dtype=dt), lambda dt: synth.model_dlrm(batch=8, table_dtype=dt),
                  lambda dt: synth.model_ragged(columns=3, batch=8, table_dtype=dt), lambda dt: synth.model_ae("E", batch=8, table_dtype=dt)):
        m, m32 = build("q8"), build("f32")
        assert m.spec.table_dtype == "q8" and m32.spec.table_dtype == "f32"
        assert m.table_bytes() == sum(t.vocab * (t.dim + 8) for t in m.tables)
    m = synth.model_s2(columns=4, vocab=50, batch=8, table_dtype="q8")
    for t, ts in zip(m.numpy_tables(), m.tables):
        assert t.dtype == np.uint8 and t.shape == (ts.vocab, ts.dim + 8)


@pytest.fixture(scope="module")
def cell_keys():
    return sorted({c.key for c in Q.variant_cells()})


def test_variant_cells_tell_the_two_readings_apart_and_expect_no_nan(oracle, cell_keys):
    """For every cell: no expected element is NaN (the GPU cells compare every element as a bit pattern), and the
    expectation on the fused dequantisation differs in bits from the expectation on the two-rounding dequantisation on at
    least 0.15 of the expected elements.  Counted are the expected elements that a table element reaches: an output also
    holds PASSTHROUGH / BATCH_COL_REDUCTION payloads and the +0.0 rows of ids outside the vocabulary and of empty bags,
    which no dequantisation can change.  Which elements those are is taken from the oracle itself, run on tables of NaN:
    an expected element is reached exactly where that run gives NaN."""
    assert len(Q.variant_cells()) == 117 and len(cell_keys) == 63
    for key in cell_keys:
        q8, fused = Q.case_tables(key)
        assert not any(np.isnan(f).any() for f in fused), key
        total = reached = differ = 0
        for t in range(K.N_REQUESTS):
            want, _ = Q.case_expectation(key, t)
            other, _ = Q.case_expectation_two_roundings(key, t)
            probe, _ = Q.case_expectation_on(key, [np.full_like(f, np.nan) for f in fused], t)
            assert not any(np.isnan(w).any() for w in want), (key, t)
            for w, o, p in zip(want, other, probe):
                hit = np.isnan(p)
                assert not (_bits(w) != _bits(o))[~hit].any(), (key, t)     # nothing else depends on the tables
                total += w.size
                reached += int(hit.sum())
                differ += int((_bits(w) != _bits(o))[hit].sum())
        print(f"{key}: the two readings differ on {differ / reached:.3f} of the {reached} expected elements a table element "
              f"reaches ({total} expected elements in all)")
        assert reached > 0 and differ / reached >= 0.15, (key, differ / reached)


# ---- vocabulary and refusals ----------------------------------------------------------------------------------------------
def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    assert re.search(r"FCP_FLAG_TABLES_Q8 = 1u << 5\b", text)
    assert re.search(r"^enum \{ FCP_TAB_Q8 = 3 \};$", text, re.M)
    assert re.search(r"FCP_LAUNCH_DENSE_TABQ8 = 11, FCP_LAUNCH_RAGGED_TABQ8 = 12, FCP_LAUNCH_HYBRID_TABQ8 = 13", text)
    assert re.search(r"#define FCP_ABI_VERSION 2\b", text)
    assert FLAG_TABLES_Q8 == _lib.FLAG_TABLES_Q8 == 32 and _lib.TAB_Q8 == 3
    assert _lib.ALL_TABLE_DTYPES == {0: "f32", 1: "bf16", 2: "f16", 3: "q8"}
    assert _lib.ALL_TABLE_DTYPE_FLAGS == {"f32": 0, "bf16": 8, "f16": 16, "q8": 32}
    assert [_lib.LAUNCH_KERNELS[k] for k in (11, 12, 13)] == ["dense_tabq8", "ragged_tabq8", "hybrid_tabq8"]


def _table_columns(spec):
    """(table_input -> (vocab, dim)) of the plan's lookups."""
    return {c.table_input: (c.vocab, c.dim) for c in spec.columns if c.form in (1, 2, 3)}


@pytest.mark.parametrize("name,spec,shapes,symbols", SPECS, ids=[s[0] for s in SPECS])
def test_host_only_plans_count_row_bytes_and_change_nothing_else(name, spec, shapes, symbols):
    """fcp_plan_table_dtype, fcp_plan_table_bytes (vocab * (dim + 8) per table), and the output side — arena bytes, group
    widths, column offsets — identical to the float32 twin's."""
    p32 = Plan(spec, host_only=True)
    tabs = _table_columns(spec)
    want = (sum(v * (d + 8) for v, d in tabs.values()), max(v * (d + 8) for v, d in tabs.values()))
    assert p32.table_bytes() == (sum(v * d * 4 for v, d in tabs.values()), max(v * d * 4 for v, d in tabs.values()))
    s = spec.with_table_dtype("q8")
    for p in (Plan(s, host_only=True), Plan(dataclasses.replace(spec, flags=spec.flags | FLAG_TABLES_Q8), host_only=True)):
        assert p.table_dtype() == "q8" and p.out_dtype() == "f32"
        assert p.table_bytes() == want, name
        assert p.arena_bytes(shapes, symbols) == p32.arena_bytes(shapes, symbols)
        for g in range(spec.n_groups):
            assert p.group_width(g) == p32.group_width(g)
        assert [p.column_offset(k) for k in range(spec.n_columns)] == [p32.column_offset(k) for k in range(spec.n_columns)]
    assert int(placement.table_bytes(s).sum()) == want[0]
    assert s.table_elem_size == 1 and s.table_row_bytes(12) == 20 and spec.table_row_bytes(12) == 48


def test_placement_gate_sees_the_row_bytes():
    """BASELINE's SHARD (4000 columns x 1 M rows, dims 8 / 16 / 32 / 64): 480 GB of float32 tables do not fit one 288 GB
    device, 152 GB of q8 tables do — REPLICATE, no exchange."""
    spec = Q.shard_spec()
    assert int(placement.table_bytes(spec).sum()) == 480 * 10 ** 9
    q8 = spec.with_table_dtype("q8")
    assert int(placement.table_bytes(q8).sum()) == 4000 * 10 ** 6 * (30 + 8) == 152 * 10 ** 9
    assert placement.decide_placement(spec, 8, hbm_bytes=288 * 10 ** 9).mode != placement.REPLICATE
    assert placement.decide_placement(q8, 8, hbm_bytes=288 * 10 ** 9).mode == placement.REPLICATE
    # the library's bytes, and the library's gate (fcp_placement_decide) on them
    p = Plan(q8, host_only=True)
    assert p.table_bytes() == (152 * 10 ** 9, 10 ** 6 * 72)
    L = _lib.load()
    for s_, mode_is_replicate in ((q8, True), (spec, False), (spec.with_table_dtype("bf16"), True)):
        tb = np.ascontiguousarray(placement.table_bytes(s_), np.int64)
        assert int(tb.sum()) == Plan(s_, host_only=True).table_bytes()[0]
        out = _lib.Placement()
        _lib.check(L.fcp_placement_decide(tb.ctypes.data, len(tb), 288 * 10 ** 9, placement.DEFAULT_RESERVE_BYTES, 8,
                                          placement.ROW_SHARD, C.byref(out)), "fcp_placement_decide")
        assert (out.mode == placement.REPLICATE) == mode_is_replicate, (s_.table_dtype, out.mode)


def test_algorithmic_bytes_charge_the_row_bytes():
    name, spec, shapes, symbols = SPECS[0]
    b32 = spec.algorithmic_bytes(shapes, symbols)
    b = spec.with_table_dtype("q8").algorithmic_bytes(shapes, symbols)
    so = spec.shape_offsets()
    rows32 = rows8 = 0
    for c in spec.columns:
        n = int(np.prod(shapes[so[c.ids_input]:so[c.ids_input] + spec.host_input_ranks[c.ids_input]])) if c.ids_input >= 0 else 0
        if c.form in (1, 2, 3):
            rows32 += n * c.dim * 4
            rows8 += n * (c.dim + 8)
        elif c.form in (4, 5):          # PASSTHROUGH / BATCH_COL_REDUCTION payloads stay float32
            rows32 += n * 4
            rows8 += n * 4
    assert b32["rows"] == rows32 and b["rows"] == rows8 and rows8 < rows32
    assert b["out"] == b32["out"] and b["ids"] == b32["ids"] and b["total"] == b32["total"] - (rows32 - rows8)


def _create_raw(spec: PlanSpec, flags: int):
    """fcp_plan_create[_ex] with these flag bits, past the Python mirror's own validation: (status, message)."""
    orig = PlanSpec.validate_table_dtype, PlanSpec.validate_out_dtype
    PlanSpec.validate_table_dtype = PlanSpec.validate_out_dtype = lambda self: None
    try:
        Plan(dataclasses.replace(spec, flags=flags), host_only=True)
    except _lib.FcpError as e:
        return e.status, str(e)
    finally:
        PlanSpec.validate_table_dtype, PlanSpec.validate_out_dtype = orig
    return _lib.FCP_OK, ""


def test_q8_with_a_16_bit_table_bit_is_an_invalid_argument():
    spec = SPECS[0][1]
    for other in (FLAG_TABLES_BF16, FLAG_TABLES_F16, FLAG_TABLES_BF16 | FLAG_TABLES_F16):
        status, msg = _create_raw(spec, FLAG_TABLES_Q8 | other)
        assert status == _lib.FCP_ERR_INVALID_ARGUMENT and "exclude" in msg
        with pytest.raises(ValueError, match="exclude"):
            dataclasses.replace(spec, flags=FLAG_TABLES_Q8 | other).validate()
    with pytest.raises(ValueError, match="exclude"):
        dataclasses.replace(spec, flags=FLAG_TABLES_F16, table_dtype="q8").validate()
    with pytest.raises(ValueError, match="table_dtype"):
        spec.with_table_dtype("q4").validate()
    assert _create_raw(spec, FLAG_TABLES_Q8)[0] == _lib.FCP_OK


@pytest.mark.parametrize("kind", sorted(Q.refused_specs()))
def test_unsupported_plan_kinds_are_refused_by_name(kind):
    spec, extra, word = Q.refused_specs()[kind]
    Plan(spec, host_only=True)                                          # the float32-table plan is fine
    status, msg = _create_raw(spec, FLAG_TABLES_Q8 | extra)
    assert status == _lib.FCP_ERR_UNSUPPORTED and word in msg and "8-bit tables" in msg, (status, msg)
    with pytest.raises(TablesQ8Unsupported, match=re.escape(word)) as e:
        dataclasses.replace(spec, flags=extra).with_table_dtype("q8").validate()
    assert "8-bit tables" in str(e.value)


def test_to_dict_carries_the_dtype_only_for_q8():
    spec = SPECS[0][1]
    assert "table_dtype" not in spec.to_dict() and spec.with_table_dtype("q8").to_dict()["table_dtype"] == "q8"


# ---- plan files -----------------------------------------------------------------------------------------------------------
def _lib_from_file(path, flags=0):
    L = _lib.load()
    h = C.c_void_p()
    rc = L.fcp_plan_create_from_file(str(path).encode(), 0, flags | _lib.FLAG_HOST_ONLY, C.byref(h))
    dt = None
    if rc == _lib.FCP_OK:
        v = C.c_int32(-1)
        assert L.fcp_plan_table_dtype(h, C.byref(v)) == _lib.FCP_OK
        dt = _lib.ALL_TABLE_DTYPES[v.value]
        L.fcp_plan_destroy(h)
    return rc, dt


def test_version_7_round_trips_through_both_parsers(tmp_path):
    for name, spec, shapes, symbols in SPECS:
        s = spec.with_table_dtype("q8")
        path = tmp_path / f"{name}.plan"
        plan_io.save_plan(s, str(path))
        lines = path.read_text().split("\n")
        assert lines[0] == "fcp_plan 7" and lines[1] == "table_dtype q8" and lines[2].startswith("layout ")
        back = plan_io.load_plan(str(path))
        assert back.table_dtype == "q8" and back.out_dtype == "f32"
        again = tmp_path / f"{name}.again.plan"
        plan_io.save_plan(back, str(again))
        assert again.read_bytes() == path.read_bytes()
        assert _lib_from_file(path) == (_lib.FCP_OK, "q8")
        p = Plan.from_file(str(path), host_only=True)
        assert p.table_dtype() == "q8" and p.spec.table_dtype == "q8"
        assert p.table_bytes() == Plan(s, host_only=True).table_bytes()
        assert p.arena_bytes(shapes, symbols) == Plan(spec, host_only=True).arena_bytes(shapes, symbols)
        # the float32 plan's file is what it was
        plan_io.save_plan(spec, str(path))
        assert "table_dtype" not in path.read_text() and _lib_from_file(path) == (_lib.FCP_OK, "f32")


def test_flags_and_the_table_dtype_line(tmp_path):
    name, spec, shapes, symbols = SPECS[0]
    f32, q8, bf = tmp_path / "f32.plan", tmp_path / "q8.plan", tmp_path / "bf16.plan"
    plan_io.save_plan(spec, str(f32))
    plan_io.save_plan(spec.with_table_dtype("q8"), str(q8))
    plan_io.save_plan(spec.with_table_dtype("bf16"), str(bf))
    # the bit on a file without the line selects the dtype
    assert _lib_from_file(f32, _lib.FLAG_TABLES_Q8) == (_lib.FCP_OK, "q8")
    assert Plan.from_file(str(f32), host_only=True, table_dtype="q8").spec.table_dtype == "q8"
    # the bit that names the file's dtype is fine, another dtype is an invalid argument
    assert _lib_from_file(q8, _lib.FLAG_TABLES_Q8) == (_lib.FCP_OK, "q8")
    assert _lib_from_file(q8, _lib.FLAG_TABLES_F16)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    assert _lib_from_file(q8, _lib.FLAG_TABLES_BF16 | _lib.FLAG_TABLES_Q8)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    assert _lib_from_file(bf, _lib.FLAG_TABLES_Q8)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    assert _lib_from_file(f32, _lib.FLAG_TABLES_F16 | _lib.FLAG_TABLES_Q8)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    # narrow output on top of a q8 file is the refused combination
    assert _lib_from_file(q8, _lib.FLAG_OUT_BF16)[0] == _lib.FCP_ERR_UNSUPPORTED


def test_malformed_table_dtype_lines_are_refused_by_both_parsers(tmp_path):
    name, spec, shapes, symbols = SPECS[0]
    good = tmp_path / "good.plan"
    plan_io.save_plan(spec.with_table_dtype("q8"), str(good))
    lines = good.read_text().split("\n")
    old = tmp_path / "old.plan"
    plan_io.save_plan(spec, str(old))
    old_lines = old.read_text().split("\n")
    v6 = tmp_path / "v6.plan"
    plan_io.save_plan(spec.with_out_dtype("f16"), str(v6))
    v6_lines = v6.read_text().split("\n")
    variants = {
        "line in a version <= 5 file": [old_lines[0], "table_dtype q8"] + old_lines[1:],
        "line at the end of a version <= 5 file": old_lines[:-1] + ["table_dtype q8", ""],
        "line in a version 6 file, in out_dtype's place": [v6_lines[0], "table_dtype q8"] + v6_lines[2:],
        "line in a version 6 file, behind out_dtype": v6_lines[:2] + ["table_dtype q8"] + v6_lines[2:],
        "out_dtype in a version 7 file, behind it": lines[:2] + ["out_dtype f16"] + lines[2:],
        "repeated line": lines[:2] + ["table_dtype q8"] + lines[2:],
        "repeated with another dtype": lines[:2] + ["table_dtype bf16"] + lines[2:],
        "repeated at the end": lines[:-1] + ["table_dtype q8", ""],
        "unknown name": [lines[0], "table_dtype q4"] + lines[2:],
        "version 7 without the line": [lines[0]] + lines[2:],
        "line after layout": [lines[0], lines[2], lines[1]] + lines[3:],
        "version 8": ["fcp_plan 8"] + lines[1:],
    }
    for what, text in variants.items():
        path = tmp_path / "bad.plan"
        path.write_text("\n".join(text))
        assert _lib_from_file(path)[0] == _lib.FCP_ERR_INVALID_ARGUMENT, what
        with pytest.raises((ValueError, AssertionError)):
            plan_io.load_plan(str(path))
    assert _lib_from_file(good) == (_lib.FCP_OK, "q8")


# ---- code object ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tabq8_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    out = {}
    procs = {}
    for src in ("fcp_tables_q8", "fcp_kernels"):
        asm = tmp_path_factory.mktemp("asm") / f"{src}.s"
        procs[src] = (asm, subprocess.Popen([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                                             os.path.join(ROOT, "recom_amd", "csrc", f"{src}.hip"), "-o", str(asm)],
                                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for src, (asm, proc) in procs.items():
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        out[src] = asm.read_text()
    return out


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}


def _field(desc, name):
    return int(re.search(r"\.amdhsa_" + name + r" (\d+)", desc).group(1))


def _waves_per_simd(vgprs: int) -> int:
    """gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_code_object_of_the_tabq8_kernels(tabq8_asm):
    text = tabq8_asm["fcp_tables_q8"]
    kernels = _kernels(text)
    names = Q.kernel_names()
    assert len(names) == 21
    # exactly the kernels the cells enumerate
    unmatched = [k for k in kernels if sum(frag in k for frag in names) != 1]
    assert not unmatched and len(kernels) == len(names), (unmatched, len(kernels))
    f32 = _kernels(tabq8_asm["fcp_kernels"])
    for name, desc in sorted(kernels.items()):
        (kernel, v, r), = [kv for frag, kv in names.items() if frag in name]
        twin = f"fcp_{kernel}_kernelILi{v}E" + (f"Li{r}E" if kernel != "ragged" else "") + "Lb0EE"
        (twin_desc,) = [d for k, d in f32.items() if twin in k]
        vgpr, twin_vgpr = _field(desc, "next_free_vgpr"), _field(twin_desc, "next_free_vgpr")
        lds, twin_lds = _field(desc, "group_segment_fixed_size"), _field(twin_desc, "group_segment_fixed_size")
        print(f"{kernel} V{v} R{r}: {vgpr} VGPRs (float32 twin {twin_vgpr}), {lds} B LDS (twin {twin_lds})")
        assert _field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        assert _waves_per_simd(vgpr) >= _waves_per_simd(twin_vgpr), f"{name}: {vgpr} VGPRs, its float32 twin {twin_vgpr}"
        assert lds <= twin_lds, name
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc), f"{name}: fp32 subnormals are flushed"
        assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", desc), f"{name}: fp16 subnormals are flushed"
        assert re.search(r"\.amdhsa_ieee_mode 1\b", desc), f"{name}: not in IEEE mode"
        label = re.search(r"^" + re.escape(name) + r":", text, re.M)
        assert label, name
        body = text[label.end():text.find(".amdhsa_kernel " + name)]
        # every fma of the body is the scalar fused one, and its multiplicand comes out of a byte-to-float conversion
        assert re.search(r"\bv_fma_f32\b", body) and "v_pk_fma_f32" not in body and "v_mac_f32" not in body, name
        cvt_src = set(re.findall(r"v_cvt_f32_ubyte[0-3](?:_e32|_e64)? v\d+, (v\d+)", body))
        assert cvt_src, name
        # the code read is V bytes per lane: a load of exactly that width whose result feeds those conversions
        load = {4: "global_load_dword", 2: "global_load_ushort", 1: "global_load_ubyte"}[v]
        code_dst = set(re.findall(r"\b" + load + r" (v\d+), ", body))
        assert code_dst & cvt_src, f"{name}: no {load} feeds a v_cvt_f32_ubyte"
        # scale and bias: one 8-byte load whose two halves are the fma's second and third operands
        pairs = {(int(a), int(b)) for a, b in re.findall(r"\bglobal_load_dwordx2 v\[(\d+):(\d+)\], ", body)}
        fma_ops = {(int(a), int(b)) for a, b in re.findall(r"\bv_fma_f32 v\d+, v\d+, v(\d+), v(\d+)", body)}
        assert pairs & fma_ops, f"{name}: no global_load_dwordx2 feeds scale and bias of a v_fma_f32"
