"""16-bit tables (FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16) without a GPU: the vocabulary and the refusals through
host-only plans and the Python mirror, version-7 plan files through both parsers, the widening restatement the GPU tests
compare with (tests/table16_cases.py) against torch's and NumPy's casts on all 65 536 patterns, and the code object of
fcp_tables16.hip against its float32 twins of fcp_kernels.hip."""
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
import table16_cases as T
from recom_amd import lib as _lib
from recom_amd import placement, plan_io, synth
from recom_amd.ops import Plan, concat_inputs
from recom_amd.plan import FLAG_TABLES_BF16, FLAG_TABLES_F16, PlanSpec, Tables16Unsupported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAB_FLAG = {"bf16": FLAG_TABLES_BF16, "f16": FLAG_TABLES_F16}


def _specs():
    """A spread of existing plans: (name, spec, shapes, symbols) of one request each."""
    out = []
    for name, m in (("mixed", synth.model_mixed(batch=33, vocab=997)), ("s1", synth.model_s1(columns=6, batch=9)),
                    ("dlrm", synth.model_dlrm(batch=17)), ("ragged", synth.model_ragged(columns=5, batch=11, seg="indices")),
                    ("per_column", T.mixed_spec(layout=1)[0]), ("xform", None)):
        if name == "xform":
            spec = T.xform_spec()
            inputs, symbols = T.xform_request()
        elif name == "per_column":
            spec = T.mixed_spec(layout=1)[1]
            req = m.make_request(0)
            inputs, symbols = req.inputs, req.symbols
        else:
            spec = m.spec
            req = m.make_request(0)
            inputs, symbols = req.inputs, req.symbols
        _, _, shapes = concat_inputs(inputs)
        out.append((name, spec, shapes, symbols))
    for key in N.DISCRIMINATION_KEYS:
        case = K.build_case(*key)
        inputs, symbols = case.requests[1]
        _, _, shapes = concat_inputs(inputs)
        out.append(("-".join(map(str, key)), case.spec, shapes, symbols))
    return out


SPECS = _specs()


# ---- vocabulary and refusals ----------------------------------------------------------------------------------------------
def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    assert re.search(r"FCP_FLAG_TABLES_BF16 = 1u << 3\b", text) and re.search(r"FCP_FLAG_TABLES_F16 = 1u << 4\b", text)
    assert re.search(r"enum \{ FCP_TAB_F32 = 0, FCP_TAB_BF16 = 1, FCP_TAB_F16 = 2 \}", text)
    assert re.search(r"FCP_LAUNCH_DENSE_TAB16 = 8, FCP_LAUNCH_RAGGED_TAB16 = 9, FCP_LAUNCH_HYBRID_TAB16 = 10", text)
    assert re.search(r"#define FCP_ABI_VERSION 2\b", text)
    assert (FLAG_TABLES_BF16, FLAG_TABLES_F16) == (_lib.FLAG_TABLES_BF16, _lib.FLAG_TABLES_F16) == (8, 16)
    assert _lib.TABLE_DTYPES == {0: "f32", 1: "bf16", 2: "f16"}
    assert [_lib.LAUNCH_KERNELS[k] for k in (8, 9, 10)] == ["dense_tab16", "ragged_tab16", "hybrid_tab16"]
    assert "fcp_plan_table_dtype" in _lib.EXPORTS
    L = _lib.load()
    assert all(hasattr(L, name) for name in _lib.EXPORTS)


@pytest.mark.parametrize("name,spec,shapes,symbols", SPECS, ids=[s[0] for s in SPECS])
def test_host_only_plans_halve_the_table_bytes_and_nothing_else(name, spec, shapes, symbols):
    """fcp_plan_table_dtype, fcp_plan_table_bytes (half the float32 value), and the output side — arena bytes, group
    widths, column offsets — identical to the float32 twin's."""
    p32 = Plan(spec, host_only=True)
    assert p32.table_dtype() == "f32" and spec.table_dtype == "f32"
    shard32, max32 = p32.table_bytes()
    assert shard32 > 0 and shard32 % 2 == 0 and max32 % 2 == 0
    assert int(placement.table_bytes(spec).sum()) == shard32
    for dt in T.DTYPES:
        s = spec.with_table_dtype(dt)
        p = Plan(s, host_only=True)
        assert p.table_dtype() == dt and p.out_dtype() == "f32"
        assert p.table_bytes() == (shard32 // 2, max32 // 2), (name, dt)
        assert int(placement.table_bytes(s).sum()) == shard32 // 2
        assert p.arena_bytes(shapes, symbols) == p32.arena_bytes(shapes, symbols)
        for g in range(spec.n_groups):
            assert p.group_width(g) == p32.group_width(g)
        assert [p.column_offset(k) for k in range(spec.n_columns)] == [p32.column_offset(k) for k in range(spec.n_columns)]
        # the same dtype chosen by the flag bit alone
        q = Plan(dataclasses.replace(spec, flags=spec.flags | TAB_FLAG[dt]), host_only=True)
        assert q.table_dtype() == dt and q.table_bytes() == (shard32 // 2, max32 // 2)


def test_placement_gate_sees_the_element_width():
    """A model whose float32 tables exceed one device's memory and whose 16-bit tables fit it: sharded, then REPLICATE."""
    spec = synth.model_s2(columns=8, batch=4).spec
    total = int(placement.table_bytes(spec).sum())
    hbm = total // 2 + total // 8
    assert placement.decide_placement(spec, 8, hbm_bytes=hbm, reserve_bytes=0).mode != placement.REPLICATE
    assert placement.decide_placement(spec.with_table_dtype("bf16"), 8, hbm_bytes=hbm, reserve_bytes=0).mode == placement.REPLICATE


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


def test_both_flags_are_an_invalid_argument():
    spec = SPECS[0][1]
    status, msg = _create_raw(spec, FLAG_TABLES_BF16 | FLAG_TABLES_F16)
    assert status == _lib.FCP_ERR_INVALID_ARGUMENT and "exclude" in msg
    with pytest.raises(ValueError, match="exclude"):
        dataclasses.replace(spec, flags=FLAG_TABLES_BF16 | FLAG_TABLES_F16).validate()
    with pytest.raises(ValueError, match="exclude"):
        dataclasses.replace(spec, flags=FLAG_TABLES_F16, table_dtype="bf16").validate()
    with pytest.raises(ValueError, match="table_dtype"):
        spec.with_table_dtype("fp8").validate()
    assert _create_raw(spec, FLAG_TABLES_BF16)[0] == _lib.FCP_OK and _create_raw(spec, FLAG_TABLES_F16)[0] == _lib.FCP_OK


@pytest.mark.parametrize("kind", sorted(T.refused_specs()))
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_unsupported_plan_kinds_are_refused_by_name(kind, dtype):
    spec, extra, word = T.refused_specs()[kind]
    Plan(spec, host_only=True)                                          # the float32-table plan is fine
    status, msg = _create_raw(spec, TAB_FLAG[dtype] | extra)
    assert status == _lib.FCP_ERR_UNSUPPORTED and word in msg and "16-bit tables" in msg, (status, msg)
    with pytest.raises(Tables16Unsupported, match=re.escape(word)):
        dataclasses.replace(spec, flags=extra).with_table_dtype(dtype).validate()


def test_to_dict_of_a_float32_plan_has_no_new_key():
    spec = SPECS[0][1]
    assert "table_dtype" not in spec.to_dict()
    assert spec.with_table_dtype("bf16").to_dict()["table_dtype"] == "bf16"
    twin = dict(spec.with_table_dtype("f16").to_dict())
    twin.pop("table_dtype")
    assert twin.keys() == spec.to_dict().keys()


def test_algorithmic_bytes_charge_two_bytes_per_table_element():
    name, spec, shapes, symbols = SPECS[0]
    b32 = spec.algorithmic_bytes(shapes, symbols)
    payload = 0                     # PASSTHROUGH / BATCH_COL_REDUCTION payloads stay float32
    so = spec.shape_offsets()
    for c in spec.columns:
        if c.form in (4, 5):
            payload += int(np.prod(shapes[so[c.ids_input]:so[c.ids_input] + spec.host_input_ranks[c.ids_input]])) * 4
    assert payload > 0
    for dt in T.DTYPES:
        b = spec.with_table_dtype(dt).algorithmic_bytes(shapes, symbols)
        assert (b["rows"] - payload) * 2 == b32["rows"] - payload
        assert b["out"] == b32["out"] and b["ids"] == b32["ids"] and b["total"] == b32["total"] - (b32["rows"] - b["rows"])


def test_synth_builders_take_table_dtype():
    for dt in T.DTYPES:
        m = synth.model_s2(columns=4, vocab=50, batch=8, table_dtype=dt)
        assert m.spec.table_dtype == dt and m.table_bytes() * 2 == synth.model_s2(columns=4, vocab=50, batch=8).table_bytes()
        f32 = synth.model_s2(columns=4, vocab=50, batch=8).numpy_tables()
        for bits, x in zip(m.numpy_tables(), f32):
            assert bits.dtype == np.uint16 and np.array_equal(bits, N.narrow(x, dt))
            assert np.array_equal(synth.table_values(bits, dt).view(np.uint32), T.widen(bits, dt).view(np.uint32))
    assert synth.model_ragged(columns=3, batch=8, table_dtype="f16").spec.table_dtype == "f16"
    assert synth.model_ae("E", batch=8, table_dtype="bf16").spec.table_dtype == "bf16"
    assert synth.model_dlrm(batch=8, table_dtype="f16").spec.table_dtype == "f16"
    assert synth.model_s1(columns=4, batch=8, table_dtype="bf16").spec.table_dtype == "bf16"
    assert synth.model_s2(columns=4, batch=8).spec.table_dtype == "f32"


# ---- plan files -----------------------------------------------------------------------------------------------------------
def _lib_from_file(path, flags=0):
    L = _lib.load()
    h = C.c_void_p()
    rc = L.fcp_plan_create_from_file(str(path).encode(), 0, flags | _lib.FLAG_HOST_ONLY, C.byref(h))
    dt = None
    if rc == _lib.FCP_OK:
        v = C.c_int32(-1)
        assert L.fcp_plan_table_dtype(h, C.byref(v)) == _lib.FCP_OK
        dt = _lib.TABLE_DTYPES[v.value]
        L.fcp_plan_destroy(h)
    return rc, dt


@pytest.mark.parametrize("name,spec,shapes,symbols", SPECS, ids=[s[0] for s in SPECS])
def test_float32_plan_files_are_byte_identical(tmp_path, name, spec, shapes, symbols):
    """The file of a float32-table plan is what the same spec gives with table_dtype never mentioned, and keeps its old
    version header."""
    fields = {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec) if f.name != "table_dtype"}
    never = PlanSpec(**fields)
    a, b = tmp_path / "a.plan", tmp_path / "b.plan"
    plan_io.save_plan(spec, str(a))
    plan_io.save_plan(never, str(b))
    assert a.read_bytes() == b.read_bytes()
    head = a.read_text().split("\n", 1)[0]
    assert head in ("fcp_plan 2", "fcp_plan 3", "fcp_plan 4", "fcp_plan 5") and "table_dtype" not in a.read_text()
    assert _lib_from_file(a) == (_lib.FCP_OK, "f32") and plan_io.load_plan(str(a)).table_dtype == "f32"
    # a narrow-output plan keeps its version-6 file too
    if spec.layout == 0 and not any(c.form == 6 for c in spec.columns):
        plan_io.save_plan(spec.with_out_dtype("bf16"), str(a))
        assert a.read_text().startswith("fcp_plan 6\nout_dtype bf16\n") and _lib_from_file(a) == (_lib.FCP_OK, "f32")


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_version_7_round_trips_through_both_parsers(tmp_path, dtype):
    for name, spec, shapes, symbols in SPECS:
        s = spec.with_table_dtype(dtype)
        path = tmp_path / f"{name}.plan"
        plan_io.save_plan(s, str(path))
        lines = path.read_text().split("\n")
        assert lines[0] == "fcp_plan 7" and lines[1] == f"table_dtype {dtype}" and lines[2].startswith("layout ")
        back = plan_io.load_plan(str(path))
        assert back.table_dtype == dtype and back.out_dtype == "f32"
        assert dataclasses.replace(back, flags=spec.flags).to_dict().keys() == s.to_dict().keys()
        again = tmp_path / f"{name}.again.plan"
        plan_io.save_plan(back, str(again))
        assert again.read_bytes() == path.read_bytes()
        assert _lib_from_file(path) == (_lib.FCP_OK, dtype)
        p = Plan.from_file(str(path), host_only=True)
        assert p.table_dtype() == dtype and p.spec.table_dtype == dtype
        assert p.table_bytes() == Plan(s, host_only=True).table_bytes()
        assert p.arena_bytes(shapes, symbols) == Plan(spec, host_only=True).arena_bytes(shapes, symbols)


def test_flags_and_the_table_dtype_line(tmp_path):
    name, spec, shapes, symbols = SPECS[0]
    f32, bf = tmp_path / "f32.plan", tmp_path / "bf16.plan"
    plan_io.save_plan(spec, str(f32))
    plan_io.save_plan(spec.with_table_dtype("bf16"), str(bf))
    # table bits on a file without the line select the dtype
    assert _lib_from_file(f32, _lib.FLAG_TABLES_BF16) == (_lib.FCP_OK, "bf16")
    assert _lib_from_file(f32, _lib.FLAG_TABLES_F16) == (_lib.FCP_OK, "f16")
    assert Plan.from_file(str(f32), host_only=True, table_dtype="f16").spec.table_dtype == "f16"
    # bits that name the file's dtype are fine, another dtype is an invalid argument
    assert _lib_from_file(bf, _lib.FLAG_TABLES_BF16) == (_lib.FCP_OK, "bf16")
    assert _lib_from_file(bf, _lib.FLAG_TABLES_F16)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    assert _lib_from_file(bf, _lib.FLAG_TABLES_F16 | _lib.FLAG_TABLES_BF16)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    assert _lib_from_file(f32, _lib.FLAG_TABLES_F16 | _lib.FLAG_TABLES_BF16)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    # narrow output on top of a version-7 file is the refused combination
    assert _lib_from_file(bf, _lib.FLAG_OUT_BF16)[0] == _lib.FCP_ERR_UNSUPPORTED


def test_malformed_table_dtype_lines_are_refused_by_both_parsers(tmp_path):
    name, spec, shapes, symbols = SPECS[0]
    good = tmp_path / "good.plan"
    plan_io.save_plan(spec.with_table_dtype("f16"), str(good))
    lines = good.read_text().split("\n")
    old = tmp_path / "old.plan"
    plan_io.save_plan(spec, str(old))
    old_lines = old.read_text().split("\n")
    v6 = tmp_path / "v6.plan"
    plan_io.save_plan(spec.with_out_dtype("f16"), str(v6))
    v6_lines = v6.read_text().split("\n")
    variants = {
        "line in a version <= 5 file": [old_lines[0], "table_dtype f16"] + old_lines[1:],
        "line at the end of a version <= 5 file": old_lines[:-1] + ["table_dtype f16", ""],
        "line in a version 6 file, in out_dtype's place": [v6_lines[0], "table_dtype f16"] + v6_lines[2:],
        "line in a version 6 file, behind out_dtype": v6_lines[:2] + ["table_dtype f16"] + v6_lines[2:],
        "out_dtype in a version 7 file, in its place": [lines[0], "out_dtype f16"] + lines[2:],
        "out_dtype in a version 7 file, behind it": lines[:2] + ["out_dtype f16"] + lines[2:],
        "repeated line": lines[:2] + ["table_dtype f16"] + lines[2:],
        "repeated at the end": lines[:-1] + ["table_dtype f16", ""],
        "unknown name": [lines[0], "table_dtype fp8"] + lines[2:],
        "f32 is not a 16-bit dtype": [lines[0], "table_dtype f32"] + lines[2:],
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
    assert _lib_from_file(good) == (_lib.FCP_OK, "f16")


# ---- the widening restatement ---------------------------------------------------------------------------------------------
def test_widen_is_torch_and_numpy_on_every_pattern():
    import torch
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for dt, td in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        got = T.widen(h, dt)
        nan = T.nan_patterns(dt)
        assert int(nan.sum()) == (254 if dt == "bf16" else 2046)
        want = torch.from_numpy(h.view(np.int16).copy()).view(td).to(torch.float32).numpy()
        assert np.array_equal(np.isnan(want), nan) and np.array_equal(np.isnan(got), nan), dt
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), dt
        if dt == "f16":
            want = h.view(np.float16).astype(np.float32)
            assert np.array_equal(np.isnan(want), nan)
            assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
            assert got[1] == np.float32(2.0 ** -24) and got[0x03FF] == np.float32(1023 * 2.0 ** -24) and got[0x0400] == np.float32(2.0 ** -14)
        else:                       # bf16 is the pattern moved up, NaNs included
            assert np.array_equal(got.view(np.uint32), h.astype(np.uint32) << 16)
        assert got.view(np.uint32)[0x8000] == 0x80000000          # -0.0 stays -0.0
    # and it undoes the narrowing the tests build their tables with
    for dt in T.DTYPES:
        fin = ~T.nan_patterns(dt)
        assert np.array_equal(N.narrow(T.widen(h, dt), dt)[fin], h[fin])


def test_variant_cells_expect_no_nan(oracle):
    """No expected element of the reused variant cells is NaN on the rounded tables: the GPU cells compare every element
    as a bit pattern."""
    for key in sorted({c.cell.key for c in T.variant_cells()}):
        for dt in T.DTYPES:
            for t in range(K.N_REQUESTS):
                want, _ = T.case_expectation(key, dt, t)
                assert not any(np.isnan(w).any() for w in want), (key, dt, t)


# ---- code object ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tab16_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    out = {}
    for src in ("fcp_tables16", "fcp_kernels"):
        asm = tmp_path_factory.mktemp("asm") / f"{src}.s"
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                            os.path.join(ROOT, "recom_amd", "csrc", f"{src}.hip"), "-o", str(asm)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out[src] = asm.read_text()
    return out


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}


def _field(desc, name):
    return int(re.search(r"\.amdhsa_" + name + r" (\d+)", desc).group(1))


def _waves_per_simd(vgprs: int) -> int:
    """gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_code_object_of_the_tab16_kernels(tab16_asm):
    text = tab16_asm["fcp_tables16"]
    kernels = _kernels(text)
    names = T.kernel_names()
    assert len(names) == 21
    # exactly the kernels the cells enumerate
    unmatched = [k for k in kernels if sum(frag in k for frag in names) != 1]
    assert not unmatched and len(kernels) == len(names), (unmatched, len(kernels))
    f32 = _kernels(tab16_asm["fcp_kernels"])
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
        assert "v_cvt_f32_f16" in body, name
        # the table read is 2 * V bytes per lane
        load = {4: "global_load_dwordx2", 2: "global_load_dword ", 1: "global_load_ushort"}[v]
        assert load in body, name
