"""Narrow output (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16) without a GPU: the vocabulary and the refusals through host-only
plans and the Python mirror, version-6 plan files through both parsers, the narrowing restatement the GPU tests compare
with (tests/narrow_output_cases.py) against torch's and NumPy's casts, how sharply the reused variant cases tell rounding
from truncation, and the code object of fcp_narrow.hip."""
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
from recom_amd import lib as _lib
from recom_amd import plan_io, synth
from recom_amd.ops import Plan, concat_inputs
from recom_amd.plan import FLAG_OUT_BF16, FLAG_OUT_F16, NarrowOutputUnsupported, PlanSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _specs():
    """A spread of existing plans: (name, spec, shapes, symbols) of one request each."""
    out = []
    for name, m in (("mixed", synth.model_mixed(batch=33, vocab=997)), ("s1", synth.model_s1(columns=6, batch=9)),
                    ("dlrm", synth.model_dlrm(batch=17)), ("ragged", synth.model_ragged(columns=5, batch=11, seg="indices"))):
        req = m.make_request(0)
        _, _, shapes = concat_inputs(req.inputs)
        out.append((name, m.spec, shapes, req.symbols))
    for key in N.DISCRIMINATION_KEYS:
        case = K.build_case(*key)
        inputs, symbols = case.requests[1]
        _, _, shapes = concat_inputs(inputs)
        out.append(("-".join(map(str, key)), case.spec, shapes, symbols))
    return out


SPECS = _specs()


def _out_region(spec: PlanSpec, shapes, symbols, elem: int) -> int:
    """Bytes of the output region of a CONCAT plan: every group rows x width x elem, 128-byte aligned."""
    return sum(-(-spec.group_rows(g, shapes, symbols) * spec.group_width(g) * elem // 128) * 128 for g in range(spec.n_groups))


# ---- vocabulary and refusals ----------------------------------------------------------------------------------------------
def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    assert re.search(r"FCP_FLAG_OUT_BF16 = 1u << 1\b", text) and re.search(r"FCP_FLAG_OUT_F16 = 1u << 2\b", text)
    assert re.search(r"FCP_OUT_F32 = 0, FCP_OUT_BF16 = 1, FCP_OUT_F16 = 2", text)
    assert re.search(r"FCP_LAUNCH_DENSE_NARROW = 5, FCP_LAUNCH_RAGGED_NARROW = 6, FCP_LAUNCH_HYBRID_NARROW = 7", text)
    assert (FLAG_OUT_BF16, FLAG_OUT_F16) == (_lib.FLAG_OUT_BF16, _lib.FLAG_OUT_F16) == (2, 4)
    assert _lib.OUT_DTYPES == {0: "f32", 1: "bf16", 2: "f16"}
    assert {_lib.LAUNCH_KERNELS[k] for k in (5, 6, 7)} == {"dense_narrow", "ragged_narrow", "hybrid_narrow"}
    assert "fcp_plan_out_dtype" in _lib.EXPORTS


@pytest.mark.parametrize("name,spec,shapes,symbols", SPECS, ids=[s[0] for s in SPECS])
def test_narrow_plans_halve_the_output_region(name, spec, shapes, symbols):
    """fcp_plan_out_dtype, arena bytes and the position of the CSR scratch of host-only plans: the narrow plan's output
    region is exactly the 2-byte layout, the scratch behind it is what the float32 twin's is."""
    p32 = Plan(spec, host_only=True)
    assert p32.out_dtype() == "f32" and spec.out_dtype == "f32"
    a32 = p32.arena_bytes(shapes, symbols)
    out32 = _out_region(spec, shapes, symbols, 4)
    scratch = a32 - out32
    assert scratch >= 0 and scratch % 4 == 0
    for dt in N.DTYPES:
        s = spec.with_out_dtype(dt)
        p = Plan(s, host_only=True)
        assert p.out_dtype() == dt
        out16 = _out_region(spec, shapes, symbols, 2)
        assert p.arena_bytes(shapes, symbols) == out16 + scratch, (name, dt)
        assert out16 % 4 == 0                       # the CSR scratch starts 4-byte (128-byte) aligned
        for g in range(spec.n_groups):              # geometry in elements is unchanged
            assert p.group_width(g) == p32.group_width(g)
        assert [p.column_offset(k) for k in range(spec.n_columns)] == [p32.column_offset(k) for k in range(spec.n_columns)]
        # the same dtype chosen by the flag bit alone
        q = Plan(dataclasses.replace(spec, flags=spec.flags | (FLAG_OUT_BF16 if dt == "bf16" else FLAG_OUT_F16)), host_only=True)
        assert q.out_dtype() == dt and q.arena_bytes(shapes, symbols) == out16 + scratch
    if all(spec.group_rows(g, shapes, symbols) * spec.group_width(g) % 64 == 0 for g in range(spec.n_groups)):
        assert 2 * _out_region(spec, shapes, symbols, 2) == out32


def test_group_byte_sizes_are_half():
    """Two groups: the second group's base (read from the arena sizes of plans cut after the first group) halves too."""
    case = K.build_case("dense", 4, 4, 1)
    assert case.spec.n_groups == 2
    inputs, symbols = case.requests[0]
    _, _, shapes = concat_inputs(inputs)
    rows = [case.spec.group_rows(g, shapes, symbols) for g in range(2)]
    widths = [case.spec.group_width(g) for g in range(2)]
    for dt in N.DTYPES:
        p = Plan(case.spec.with_out_dtype(dt), host_only=True)
        want = sum(-(-r * w * 2 // 128) * 128 for r, w in zip(rows, widths))
        assert p.arena_bytes(shapes, symbols) == want


def _create_raw(spec: PlanSpec, flags: int):
    """fcp_plan_create[_ex] with these flag bits, past the Python mirror's own validation: (status, message)."""
    orig = PlanSpec.validate_out_dtype
    PlanSpec.validate_out_dtype = lambda self: None
    try:
        Plan(dataclasses.replace(spec, flags=flags), host_only=True)
    except _lib.FcpError as e:
        return e.status, str(e)
    finally:
        PlanSpec.validate_out_dtype = orig
    return _lib.FCP_OK, ""


def test_both_flags_are_an_invalid_argument():
    spec = SPECS[0][1]
    status, msg = _create_raw(spec, FLAG_OUT_BF16 | FLAG_OUT_F16)
    assert status == _lib.FCP_ERR_INVALID_ARGUMENT and "exclude" in msg
    with pytest.raises(ValueError, match="exclude"):
        dataclasses.replace(spec, flags=FLAG_OUT_BF16 | FLAG_OUT_F16).validate()
    with pytest.raises(ValueError, match="exclude"):
        dataclasses.replace(spec, flags=FLAG_OUT_F16, out_dtype="bf16").validate()
    with pytest.raises(ValueError, match="out_dtype"):
        spec.with_out_dtype("fp8").validate()
    assert _create_raw(spec, FLAG_OUT_BF16)[0] == _lib.FCP_OK and _create_raw(spec, FLAG_OUT_F16)[0] == _lib.FCP_OK


@pytest.mark.parametrize("kind", sorted(N.refused_specs()))
@pytest.mark.parametrize("dtype", N.DTYPES)
def test_unsupported_plan_kinds_are_refused_by_name(kind, dtype):
    spec, word = N.refused_specs()[kind]
    Plan(spec, host_only=True)                                          # the float32 plan is fine
    status, msg = _create_raw(spec, FLAG_OUT_BF16 if dtype == "bf16" else FLAG_OUT_F16)
    assert status == _lib.FCP_ERR_UNSUPPORTED and word in msg, (status, msg)
    with pytest.raises(NarrowOutputUnsupported, match=re.escape(word)):
        spec.with_out_dtype(dtype).validate()


def test_to_dict_of_a_float32_plan_has_no_new_key():
    spec = SPECS[0][1]
    assert "out_dtype" not in spec.to_dict()
    assert spec.with_out_dtype("bf16").to_dict()["out_dtype"] == "bf16"
    twin = dict(spec.with_out_dtype("f16").to_dict())
    twin.pop("out_dtype")
    assert twin.keys() == spec.to_dict().keys()


def test_algorithmic_bytes_charge_two_bytes_per_written_element():
    name, spec, shapes, symbols = SPECS[0]
    b32 = spec.algorithmic_bytes(shapes, symbols)
    for dt in N.DTYPES:
        b = spec.with_out_dtype(dt).algorithmic_bytes(shapes, symbols)
        assert b["out"] * 2 == b32["out"] and b["read"] == b32["read"] and b["total"] == b32["read"] + b["out"]


def test_synth_builders_take_out_dtype():
    assert synth.model_s2(columns=4, batch=8, out_dtype="bf16").spec.out_dtype == "bf16"
    assert synth.model_ragged(columns=3, batch=8, out_dtype="f16").spec.out_dtype == "f16"
    assert synth.model_ae("E", batch=8, out_dtype="bf16").spec.out_dtype == "bf16"
    assert synth.model_dlrm(batch=8, out_dtype="f16").spec.out_dtype == "f16"
    assert synth.model_s2(columns=4, batch=8).spec.out_dtype == "f32"


# ---- plan files -----------------------------------------------------------------------------------------------------------
def _lib_from_file(path, flags=0):
    L = _lib.load()
    h = C.c_void_p()
    rc = L.fcp_plan_create_from_file(str(path).encode(), 0, flags | _lib.FLAG_HOST_ONLY, C.byref(h))
    dt = None
    if rc == _lib.FCP_OK:
        v = C.c_int32(-1)
        assert L.fcp_plan_out_dtype(h, C.byref(v)) == _lib.FCP_OK
        dt = _lib.OUT_DTYPES[v.value]
        L.fcp_plan_destroy(h)
    return rc, dt


@pytest.mark.parametrize("name,spec,shapes,symbols", SPECS, ids=[s[0] for s in SPECS])
def test_float32_plan_files_are_byte_identical(tmp_path, name, spec, shapes, symbols):
    """The file of a float32 plan is what the same spec gives with out_dtype never mentioned (a PlanSpec built without
    the field), and keeps its old version header."""
    fields = {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec) if f.name != "out_dtype"}
    never = PlanSpec(**fields)
    a, b = tmp_path / "a.plan", tmp_path / "b.plan"
    plan_io.save_plan(spec, str(a))
    plan_io.save_plan(never, str(b))
    assert a.read_bytes() == b.read_bytes()
    head = a.read_text().split("\n", 1)[0]
    assert head in ("fcp_plan 2", "fcp_plan 3", "fcp_plan 4", "fcp_plan 5") and "out_dtype" not in a.read_text()
    assert _lib_from_file(a) == (_lib.FCP_OK, "f32") and plan_io.load_plan(str(a)).out_dtype == "f32"


@pytest.mark.parametrize("dtype", N.DTYPES)
def test_version_6_round_trips_through_both_parsers(tmp_path, dtype):
    for name, spec, shapes, symbols in SPECS:
        s = spec.with_out_dtype(dtype)
        path = tmp_path / f"{name}.plan"
        plan_io.save_plan(s, str(path))
        lines = path.read_text().split("\n")
        assert lines[0] == "fcp_plan 6" and lines[1] == f"out_dtype {dtype}" and lines[2].startswith("layout ")
        back = plan_io.load_plan(str(path))
        assert back.out_dtype == dtype
        assert dataclasses.replace(back, flags=spec.flags).to_dict().keys() == s.to_dict().keys()
        again = tmp_path / f"{name}.again.plan"
        plan_io.save_plan(back, str(again))
        assert again.read_bytes() == path.read_bytes()
        assert _lib_from_file(path) == (_lib.FCP_OK, dtype)
        p = Plan.from_file(str(path), host_only=True)
        assert p.out_dtype() == dtype and p.spec.out_dtype == dtype
        assert p.arena_bytes(shapes, symbols) == Plan(s, host_only=True).arena_bytes(shapes, symbols)


def test_flags_and_the_out_dtype_line(tmp_path):
    name, spec, shapes, symbols = SPECS[0]
    f32, bf = tmp_path / "f32.plan", tmp_path / "bf16.plan"
    plan_io.save_plan(spec, str(f32))
    plan_io.save_plan(spec.with_out_dtype("bf16"), str(bf))
    # narrow bits on a file without the line select the dtype
    assert _lib_from_file(f32, _lib.FLAG_OUT_BF16) == (_lib.FCP_OK, "bf16")
    assert _lib_from_file(f32, _lib.FLAG_OUT_F16) == (_lib.FCP_OK, "f16")
    assert Plan.from_file(str(f32), host_only=True, out_dtype="f16").spec.out_dtype == "f16"
    # bits that name the file's dtype are fine, another dtype is an invalid argument
    assert _lib_from_file(bf, _lib.FLAG_OUT_BF16) == (_lib.FCP_OK, "bf16")
    assert _lib_from_file(bf, _lib.FLAG_OUT_F16)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    assert _lib_from_file(bf, _lib.FLAG_OUT_F16 | _lib.FLAG_OUT_BF16)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
    assert _lib_from_file(f32, _lib.FLAG_OUT_F16 | _lib.FLAG_OUT_BF16)[0] == _lib.FCP_ERR_INVALID_ARGUMENT


def test_malformed_out_dtype_lines_are_refused_by_both_parsers(tmp_path):
    name, spec, shapes, symbols = SPECS[0]
    good = tmp_path / "good.plan"
    plan_io.save_plan(spec.with_out_dtype("f16"), str(good))
    lines = good.read_text().split("\n")
    old = tmp_path / "old.plan"
    plan_io.save_plan(spec, str(old))
    old_lines = old.read_text().split("\n")
    variants = {
        "line in a version <= 5 file": [old_lines[0], "out_dtype f16"] + old_lines[1:],
        "line at the end of a version <= 5 file": old_lines[:-1] + ["out_dtype f16", ""],
        "repeated line": lines[:2] + ["out_dtype f16"] + lines[2:],
        "repeated at the end": lines[:-1] + ["out_dtype f16", ""],
        "unknown name": [lines[0], "out_dtype fp8"] + lines[2:],
        "f32 is not a narrow dtype": [lines[0], "out_dtype f32"] + lines[2:],
        "version 6 without the line": [lines[0]] + lines[2:],
        "line after layout": [lines[0], lines[2], lines[1]] + lines[3:],
    }
    for what, text in variants.items():
        path = tmp_path / "bad.plan"
        path.write_text("\n".join(text))
        assert _lib_from_file(path)[0] == _lib.FCP_ERR_INVALID_ARGUMENT, what
        with pytest.raises((ValueError, AssertionError)):
            plan_io.load_plan(str(path))
    assert _lib_from_file(good) == (_lib.FCP_OK, "f16")


# ---- the narrowing restatement --------------------------------------------------------------------------------------------
def _patterns():
    rng = np.random.default_rng(20240607)
    rand = rng.integers(0, 1 << 32, 10 ** 6, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([np.asarray([e[0] for e in N.EDGES] + list(N.NAN_EDGES), np.uint32), rand])


def _same16(got, want, dtype):
    nan = N.is_nan16(want, dtype)
    return np.where(nan, N.is_nan16(got, dtype), got == want)


def test_edge_list_is_what_the_specification_says():
    for f32, bf, h in N.EDGES:
        x = np.asarray([f32], np.uint32).view(np.float32)
        assert (int(N.narrow(x, "bf16")[0]), int(N.narrow(x, "f16")[0])) == (bf, h), hex(f32)
    nans = np.asarray(N.NAN_EDGES, np.uint32).view(np.float32)
    assert N.is_nan16(N.narrow(nans, "bf16"), "bf16").all() and N.is_nan16(N.narrow(nans, "f16"), "f16").all()
    # the ones the issue names
    named = {0x3F808000: ("bf16", 0x3F80), 0x3F818000: ("bf16", 0x3F82), 0x7F7FFFFF: ("bf16", 0x7F80)}
    for f32, (dt, want) in named.items():
        assert int(N.narrow(np.asarray([f32], np.uint32).view(np.float32), dt)[0]) == want
    x = np.asarray([65519.9, 65520.0, N.FLT_MAX, -0.0], np.float32)
    assert N.narrow(x, "f16").tolist() == [0x7BFF, 0x7C00, 0x7C00, 0x8000] and int(N.narrow(x, "bf16")[3]) == 0x8000


def test_narrow_is_torch_and_numpy_and_the_integer_formula():
    import torch
    u = _patterns()
    x = u.view(np.float32)
    t = torch.from_numpy(x)
    for dt, td in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        want = t.to(td).view(torch.int16).numpy().view(np.uint16)
        assert _same16(N.narrow(x, dt), want, dt).all(), dt
    with np.errstate(all="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    assert _same16(N.narrow(x, "f16"), want, "f16").all()
    # the integer form the issue writes down, with its NaN guard
    w = u.astype(np.uint64)
    formula = ((w + 0x7FFF + ((w >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    got = N.narrow(x, "bf16")
    assert np.array_equal(got[~nan], formula[~nan]) and N.is_nan16(got[nan], "bf16").all()


def test_edge_plans_land_on_their_outcomes(oracle):
    """The pooled columns of the edge plans reach the ties, the fp16 overflow edge, both subnormal ranges, -0.0, +-inf and
    NaN as FLOAT32 results of the oracle (so that the narrow store is what decides), beside rows without ids; the share
    of elements compared as "is NaN" stays below a quarter."""
    for vec in K.VECS:
        case = N.edge_case(vec)
        assert all(c.dim % vec == 0 for c in case.spec.columns) and any(c.dim % (2 * vec) for c in case.spec.columns)
        for t, (inputs, symbols) in enumerate(case.requests):
            blob, offsets, shapes = concat_inputs(inputs)
            want, bad = oracle.process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, case.tables, symbols)
            assert bad == 0
            g1 = want[1].view(np.uint32)
            seen = set()
            for r, name in case.outcome_rows[t].items():
                seen.add(name)
                if name not in N.OUTCOME_BITS:
                    continue
                s, m = g1[r, case.sum_cols[0]:case.sum_cols[1]], g1[r, case.mean_cols[0]:case.mean_cols[1]]
                bits = N.OUTCOME_BITS[name]
                if bits is None:
                    assert np.isnan(want[1][r, case.sum_cols[0]:case.mean_cols[1]]).all(), name
                    continue
                assert (s == bits).all(), (vec, t, name, hex(int(s[0])))
                # the mean divides the scaled addends by their count: the same value — but -2^-149 / 2, a tie, is the
                # float32 -0.0, and 2 x FLT_MAX has overflowed before the division
                mean_bits = {"neg0": 0x80000000, "flt_max": 0x7F800000}.get(name, bits)
                assert (m == mean_bits).all(), (vec, t, name, hex(int(m[0])))
            assert seen == {n for n, _ in N.OUTCOMES}
            empty = [r for r in range(want[1].shape[0]) if r not in case.outcome_rows[t]]
            assert len(empty) >= 7 and not g1[empty, case.sum_cols[0]:case.mean_cols[1]].any()
            for dt in N.DTYPES:
                share = np.mean([N.is_nan16(N.narrow(w, dt), dt).mean() for w in want])
                assert 0 < share <= 0.25, (vec, t, dt, share)
            # the copy columns carry the whole edge list
            for g in (0, 1):
                assert set(N.EDGE_VALUES.view(np.uint32).tolist()) <= set(want[g].view(np.uint32).ravel().tolist())


# ---- discrimination -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", N.DISCRIMINATION_KEYS, ids=["-".join(map(str, k)) for k in N.DISCRIMINATION_KEYS])
def test_variant_cases_tell_rounding_from_truncation(oracle, key):
    """Over the oracle's float32 outputs of a reused variant case: at least 40 % of the finite non-zero elements differ
    between round-to-nearest-even and truncation to bf16, none overflows or vanishes in fp16, and none is NaN: a kernel
    that truncates cannot pass the GPU cells, and the cells compare no element as "is NaN".  The fp16 property is asserted
    on the fp16 patterns themselves; the largest magnitude is printed (227.3 in ("hybrid", 2, 2, 2), whose 1000-id bags
    sum that high; below 170 in the other two cases)."""
    case = K.build_case(*key)
    differ = total = 0
    top = 0.0
    for inputs, symbols in case.requests:
        blob, offsets, shapes = concat_inputs(inputs)
        want, _ = oracle.process_feature_columns(case.spec.to_dict(), blob, offsets, shapes, case.tables, symbols)
        for w in want:
            assert not np.isnan(w).any()
            live = np.isfinite(w) & (w != 0)
            x = w[live]
            top = max(top, float(np.abs(x).max(initial=0.0)))
            h = N.narrow(x, "f16")
            assert ((h & 0x7FFF) != 0).all() and ((h & 0x7FFF) < 0x7C00).all()       # neither vanished nor overflowed
            differ += int((N.narrow(x, "bf16") != N.truncate_bf16(x)).sum())
            total += int(x.size)
    share = differ / total
    print(f"{key}: round-to-nearest-even and truncation to bf16 differ on {share:.3f} of {total} elements, max |x| {top:.1f}")
    assert top < 65504.0
    assert share >= 0.40, share



# ---- code object ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    out = {}
    for src in ("fcp_narrow", "fcp_kernels"):
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


def test_code_object_of_the_narrow_kernels(narrow_asm):
    text = narrow_asm["fcp_narrow"]
    kernels = _kernels(text)
    names = N.kernel_names()
    assert len(names) == 21
    # exactly the kernels the cells enumerate
    unmatched = [k for k in kernels if sum(frag in k for frag in names) != 1]
    assert not unmatched and len(kernels) == len(names), (unmatched, len(kernels))
    f32 = _kernels(narrow_asm["fcp_kernels"])
    for name, desc in kernels.items():
        (kernel, v, r), = [kv for frag, kv in names.items() if frag in name]
        vgpr = _field(desc, "next_free_vgpr")
        headline = kernel == "ragged" or (v == 4 and r == 4)
        assert vgpr <= (64 if headline else 72), f"{name}: {vgpr} VGPRs"
        assert _field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        twin = f"fcp_{kernel}_kernelILi{v}E" + (f"Li{r}E" if kernel != "ragged" else "") + "Lb0EE"
        (twin_desc,) = [d for k, d in f32.items() if twin in k]
        assert _field(desc, "group_segment_fixed_size") <= _field(twin_desc, "group_segment_fixed_size"), name
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc), f"{name}: fp32 subnormals are flushed"
        assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", desc), f"{name}: fp16 subnormals are flushed"
        assert re.search(r"\.amdhsa_ieee_mode 1\b", desc), f"{name}: not in IEEE mode"
        label = re.search(r"^" + re.escape(name) + r":", text, re.M)
        assert label, name
        body = text[label.end():text.find(".amdhsa_kernel " + name)]
        if kernel != "dense":
            assert "v_div_scale_f32" in body and "v_div_fixup_f32" in body, f"{name}: the mean is not an IEEE division"
        assert "v_cvt_f16_f32" in body, name
        # the store is 2 * V bytes per lane, and nothing wider is written
        store = {4: "global_store_dwordx2", 2: "global_store_dword", 1: "global_store_short"}[v]
        stores = re.findall(r"(global_store_\w+) [^\n]*?off([^\n]*)", body)
        kinds = {"sc1 nt": 0, "nt": 0, "plain": 0}
        for op, tail in stores:
            if op == store:
                tail = tail.strip()
                kinds["sc1 nt" if tail.startswith("sc1 nt") else "nt" if tail.startswith("nt") else "plain"] += 1
        need = r if kernel == "dense" else 1
        assert min(kinds.values()) >= need, (name, kinds)
        assert "global_store_dwordx4" not in body and "global_store_dwordx3" not in body, name
        if kernel == "dense" and (v, r) == (4, 4):
            assert min(kinds.values()) >= 4, kinds
