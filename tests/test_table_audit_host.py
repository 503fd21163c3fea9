"""fcp_table_audit / fcp_table_formats_choose without a GPU: the C ABI's surface, the two structs' layout against a compiled C99
snippet, the audit's status order, and the chooser — within budget, admissible, deterministic, monotone, optimal for the
bytes it uses against brute force — through ctypes and, in a stand-alone program, under the address and undefined-behaviour
sanitizers.  (The kernels themselves: tests/test_gpu_table_audit.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import table_audit_cases as TA
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
CSRC = os.path.join(ROOT, "recom_amd", "csrc")
INV, UNS, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_UNSUPPORTED, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_three_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint64_t fcp_table_audit_workspace_bytes\(void\);", text)
    assert re.search(r"\bint fcp_table_audit\(const float \*src, int64_t rows, int32_t dim, fcp_table_audit_t \*out, void \*workspace, "
                     r"int32_t device,\s+void \*stream\);", text)
    assert re.search(r"\bint fcp_table_formats_choose\(const fcp_table_audit_t \*audits, const int64_t \*rows, const int32_t \*dims, "
                     r"int32_t n_tables,\s+int64_t budget_bytes, uint32_t allowed_kinds, const double \*table_weight, int32_t \*kinds_out,\s+"
                     r"int64_t \*bytes_out, double \*error_out\);", text)
    names = {"fcp_table_audit_workspace_bytes", "fcp_table_audit", "fcp_table_formats_choose"}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names)
    ws = L.fcp_table_audit_workspace_bytes()
    assert ws > 0 and ws % 8 == 0 and ws == L.fcp_table_audit_workspace_bytes()


def test_struct_layout_matches_a_compiled_c99_snippet(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = {"fcp_table_audit_kind_t": ("rows_bad", "first_bad_row", "sum_sq_err", "max_abs_err", "reserved"),
              "fcp_table_audit_t": ("rows", "rows_nonfinite", "first_nonfinite_row", "sum_sq", "kind")}
    prints = "".join(f'  printf("{t} %zu\\n", sizeof({t}));\n' + "".join(f'  printf("{t}.{f} %zu\\n", offsetof({t}, {f}));\n' for f in fs)
                     for t, fs in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fcp_hip.h"\nint main(void) {\n' + prints + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", exe], check=True, capture_output=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for t, cls in (("fcp_table_audit_kind_t", _lib.TableAuditKind), ("fcp_table_audit_t", _lib.TableAudit)):
        assert int(got[t]) == C.sizeof(cls), t
        assert [f for f, _ in cls._fields_] == list(fields[t])
        for f in fields[t]:
            assert int(got[f"{t}.{f}"]) == getattr(cls, f).offset, (t, f)
    assert C.sizeof(_lib.TableAudit) == 160 and C.sizeof(_lib.TableAuditKind) == 32


def _audit(src, rows, dim, out, workspace, device=0):
    L = _lib.load()
    status = L.fcp_table_audit(C.c_void_p(src), rows, dim, C.c_void_p(out), C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def test_status_codes_arrive_in_the_stated_order():
    """No GPU here: valid arguments end in FCP_ERR_NO_DEVICE, rows == 0 included (the fold still runs, so `out` is defined) —
    after every argument check.  (Pointers are never dereferenced on the host: plain numbers serve.)"""
    import torch
    no_gpu = not torch.cuda.is_available()      # (with a GPU valid arguments would run: only the device-free statuses are checked)
    A = 1 << 20
    for args, word in (((A, -1, 64, A, A), "rows"), ((A, 2 ** 32 - 3, 64, A, A), "rows"), ((A, 2 ** 40, 64, A, A), "rows"),
                       ((A, 5, 0, A, A), "dim"), ((A, 5, -3, A, A), "dim"),
                       ((A, 5, 64, 0, A), "out"), ((A, 5, 64, A, 0), "workspace"), ((A, 0, 64, 0, A), "out"), ((0, 0, 64, A, 0), "workspace"),
                       ((0, 5, 64, A, A), "src"),
                       ((A + 4, 5, 64, A, A), "src"), ((A + 8, 5, 64, A, A), "src"),      # V 4: 16 bytes
                       ((A + 4, 5, 62, A, A), "src"),                                     # V 2: 8 bytes
                       ((A + 2, 5, 61, A, A), "src"),                                     # V 1: 4 bytes
                       ((A, 5, 64, A + 4, A), "out"), ((A, 5, 64, A, A + 4), "workspace")):
        status, msg = _audit(*args)
        assert status == INV and word in msg, (args, status, msg)
    # the order of fcp_table_convert: rows < 0, dim, null pointers, the row limit, alignment
    assert "rows" in _audit(0, -1, 0, 0, 0)[1]
    assert "dim" in _audit(0, 5, 0, 0, 0)[1]
    assert "out" in _audit(0, 2 ** 32, 64, 0, 0)[1]
    assert "workspace" in _audit(0, 2 ** 32, 64, A, 0)[1]
    assert "src" in _audit(0, 2 ** 32, 64, A, A)[1]
    assert "rows" in _audit(A + 4, 2 ** 32, 64, A, A)[1]
    assert "src" in _audit(A + 4, 5, 64, A + 4, A + 4)[1]
    if no_gpu:
        # alignments that ARE enough, a null src with no rows, the last row count below the limit
        for args in ((A + 16, 5, 64, A + 8, A + 8), (A + 8, 5, 62, A, A), (A + 4, 5, 61, A, A), (0, 0, 64, A, A), (A, 0, 7, A, A),
                     (A, 2 ** 32 - 4, 64, A, A)):
            assert _audit(*args)[0] == NODEV, args


# ---- code object -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audit_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("asm") / "fcp_table_audit.s"
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                           os.path.join(CSRC, "fcp_table_audit.hip"), "-o", str(asm)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return asm.read_text()


def test_code_object_of_the_audit_kernels(audit_asm):
    """fcp_table_audit.hip compiles for gfx950: 3 V x 7 G x {unweighted, weighted} audit kernels and the fold; no scratch; LDS
    only for the four wave records of a block's fold (384 bytes), none in the fold kernel; denormals kept, IEEE mode.  A lane
    passes n = V * (S + 1 if G == 64 else S) elements per row through `judge` (S: slots_in_registers; the + 1: the tail loop's
    body) and loads S + (2 if G == 64 else 0) slots (the tail in both passes); a weighted kernel loads the row's count besides
    and nothing else.  Each element is one float64 fused multiply-add into each of the four sums (nothing else is fused in
    float64: the fold adds), and ONE float32 fma, ld_q8's — every other float32 fma belongs to the two divisions' expansions
    (five each, as in fcp_convert.hip): nothing is contracted, nothing packed."""
    kernels = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", audit_asm, re.S)}
    field = lambda desc, name: int(re.search(r"\.amdhsa_" + name + r" (\d+)", desc).group(1))

    def body(name):
        label = re.search(r"^" + re.escape(name) + r":", audit_asm, re.M)
        assert label, name
        text = audit_asm[label.end():audit_asm.find(".amdhsa_kernel " + name)]
        code = (ln.split(";")[0].split() for ln in text.splitlines() if ln.startswith("\t"))        # (labels start in column 0)
        return [words[0] for words in code if words and not words[0].startswith(".")]

    audit = {k for k in kernels if "fcp_table_audit_kernel" in k}
    (fold,) = [k for k in kernels if "fcp_table_audit_fold_kernel" in k]
    assert len(audit) == 42 and len(kernels) == 43, sorted(kernels)
    for name, desc in sorted(kernels.items()):
        assert field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        assert field(desc, "group_segment_fixed_size") == (0 if name == fold else 384), name
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc), f"{name}: fp32 subnormals are flushed"
        assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", desc), f"{name}: fp16 / fp64 subnormals are flushed"
        assert re.search(r"\.amdhsa_ieee_mode 1\b", desc), f"{name}: not in IEEE mode"
        assert not any(op.startswith("scratch_") for op in body(name)), name
    for v in (1, 2, 4):
        for g in (1, 2, 4, 8, 16, 32, 64):
            ops = {}
            for weighted in (0, 1):
                (name,) = [k for k in audit if f"fcp_table_audit_kernelILi{v}ELi{g}ELb{weighted}EE" in k]
                ops[weighted] = body(name)
            kept = 4 if g == 64 else 3 if g == 1 else 1
            loads = [sum(op.startswith("global_load") for op in ops[w]) for w in (0, 1)]
            assert loads == [kept + (2 if g == 64 else 0), kept + (2 if g == 64 else 0) + 1], (v, g, loads)
            n = v * (kept + (g == 64))
            for w in (0, 1):
                assert sum(bool(re.match(r"v_fmac?_f64", op)) for op in ops[w]) == 4 * n, (v, g, w)
                assert not any(re.match(r"v_pk_fma_f32|v_mac_f32|v_mad_f32", op) for op in ops[w]), (v, g, w)
                assert ops[w].count("v_div_fixup_f32") == 2 and ops[w].count("v_div_fmas_f32") == 2, (v, g, w)
                assert sum(bool(re.match(r"v_fmac?_f32", op)) for op in ops[w]) == 5 * 2 + n, (v, g, w)


# ---- the chooser ---------------------------------------------------------------------------------------------------------------
def _raw_audits(inst):
    arr = (_lib.TableAudit * len(inst["tables"]))()
    for a, tab in zip(arr, inst["tables"]):
        a.rows, a.rows_nonfinite, a.first_nonfinite_row, a.sum_sq = tab["rows"], tab["rows_nonfinite"], -1 if not tab["rows_nonfinite"] else 0, tab["sum_sq"]
        for k in range(4):
            a.kind[k].rows_bad, a.kind[k].first_bad_row, a.kind[k].sum_sq_err = tab["bad"][k], -1 if not tab["bad"][k] else 0, tab["sse"][k]
    return arr


def choose(inst, budget):
    """(status, kinds, bytes, error, message) of fcp_table_formats_choose on a synthetic instance"""
    L = _lib.load()
    n = len(inst["tables"])
    rows = (C.c_int64 * n)(*[t["rows"] for t in inst["tables"]])
    dims = (C.c_int32 * n)(*[t["dim"] for t in inst["tables"]])
    w = None if inst["weights"] is None else (C.c_double * n)(*inst["weights"])
    kinds = (C.c_int32 * n)(*([-1] * n))
    nbytes, err = C.c_int64(-1), C.c_double(-1.0)
    status = L.fcp_table_formats_choose(_raw_audits(inst), rows, dims, n, budget, inst["allowed"], w, kinds, C.byref(nbytes), C.byref(err))
    return status, tuple(kinds), nbytes.value, err.value, L.fcp_last_error().decode()


def test_chooser_against_brute_force_on_random_instances():
    """Per instance (<= 6 tables, continuous errors: no ties) and budget: the answer is within the budget, uses admissible kinds
    only, is the same when asked again, reports the bytes and the error of its kinds, and NO admissible assignment within the
    bytes it used has a lower weighted error (every greedy state minimises error + lambda * bytes).  Errors are sums of at most
    6 non-negative float64 terms formed in another order: equal to within 6 * 2^-53 relative, compared with 1e-12.  An
    impossible budget is FCP_ERR_UNSUPPORTED and names the bytes of the smallest admissible assignment."""
    n_ok = n_uns = 0
    for inst in TA.instances():
        every = list(TA.all_assignments(inst))
        smallest = min(b for _, (b, _) in every)
        last_err = None
        for budget in TA.budgets(inst):
            status, kinds, nbytes, err, msg = choose(inst, budget)
            if budget < smallest:
                assert status == UNS and str(smallest) in msg and nbytes == smallest, (budget, smallest, status, msg)
                n_uns += 1
                continue
            n_ok += 1
            assert status == OK, msg
            assert choose(inst, budget)[:4] == (status, kinds, nbytes, err)
            assert all(k in TA.admissible(inst, t) for t, k in enumerate(kinds)), kinds
            want_bytes, want_err = TA.assignment_cost(inst, kinds)
            assert nbytes == want_bytes <= budget and err == pytest.approx(want_err, rel=1e-12, abs=0)
            better = [(k, c) for k, c in every if c[0] <= nbytes and c[1] < err * (1 - 1e-12)]
            assert not better, (inst, budget, kinds, nbytes, err, better[:3])
            assert last_err is None or err <= last_err                   # budgets ascend: the error does not rise
            last_err = err
        assert choose(inst, sum(t["rows"] * 4 * t["dim"] for t in inst["tables"]))[1] == (0,) * len(inst["tables"])   # all float32 fits
    assert n_ok > 300 and n_uns >= 60


def _one(dim, rows=1000, sse=(0.0, 3e-3, 2e-3, 1e-3), bad=(0, 0, 0, 0), nonfinite=0, sum_sq=10.0):
    return {"rows": rows, "dim": dim, "sum_sq": sum_sq, "rows_nonfinite": nonfinite, "sse": list(sse), "bad": list(bad)}


def test_chooser_named_cases():
    BF16, F16, Q8 = 1, 2, 3
    # a dim-1 column never gets q8 (9 bytes a row against 4), nor a dim-2 one (10 against 8): 16 bits is their smallest
    for dim in (1, 2):
        inst = {"tables": [_one(dim)], "weights": None, "allowed": 15}
        for budget in (1000 * 2 * dim, 1000 * 3 * dim, 1000 * 4 * dim - 1):
            assert choose(inst, budget)[1] == (F16,)                    # equal bytes: the lower error wins
        status, _, nbytes, _, msg = choose(inst, 1000 * 2 * dim - 1)
        assert status == UNS and nbytes == 2000 * dim and str(2000 * dim) in msg
    # equal bytes and equal error: the lower FCP_TAB_*
    inst = {"tables": [_one(8, sse=(0.0, 2e-3, 2e-3, 9.0))], "weights": None, "allowed": 0b0111}
    assert choose(inst, 16000)[1] == (BF16,)
    # a table with a bad fp16 row never gets fp16, whatever its error
    inst = {"tables": [_one(8, sse=(0.0, 3e-3, 1e-9, 5.0), bad=(0, 0, 2, 0))], "weights": None, "allowed": 0b0111}
    assert choose(inst, 16000)[1] == (BF16,) and choose(inst, 16000 - 1)[0] == UNS
    # a table with a NaN row stays float32; the other table pays for the budget
    inst = {"tables": [_one(64, nonfinite=1), _one(64)], "weights": None, "allowed": 15}
    status, kinds, nbytes, _, _ = choose(inst, 256000 + 72000)
    assert status == OK and kinds == (0, Q8) and nbytes == 256000 + 72000
    assert choose(inst, 256000 + 72000 - 1)[0] == UNS
    # allowed_kinds without a bit: that kind is never chosen; float32 needs no bit
    inst = {"tables": [_one(64)], "weights": None, "allowed": 0}
    assert choose(inst, 256000)[1] == (0,) and choose(inst, 255999)[0] == UNS
    inst["allowed"] = 0b0100
    assert choose(inst, 200000)[1] == (F16,)
    # a point above the hull is skipped: bf16 (128 bytes a row, error 3.0) lies above the line from float32 to q8 (72 bytes, 3.1)
    inst = {"tables": [_one(64, sse=(0.0, 3.0, 3.0, 3.1))], "weights": [1.0], "allowed": 15}
    assert choose(inst, 200000)[1] == (Q8,)
    # weights steer: the heavy table keeps its bytes (q8 has the lowest error here, so the hull goes from float32 straight to it)
    two = [_one(64), _one(64)]
    assert choose({"tables": two, "weights": [100.0, 1.0], "allowed": 15}, 256000 + 128000)[1] == (0, Q8)
    assert choose({"tables": two, "weights": [1.0, 100.0], "allowed": 15}, 256000 + 128000)[1] == (Q8, 0)
    assert choose({"tables": two, "weights": None, "allowed": 15}, 256000 + 128000)[1] == (Q8, 0)           # a tie: the lower table index
    # invalid arguments
    L = _lib.load()
    for bad_inst, budget in (({"tables": [_one(0)], "weights": None, "allowed": 15}, 10), ({"tables": [_one(8, rows=-1)], "weights": None, "allowed": 15}, 10),
                             ({"tables": [_one(8)], "weights": [-1.0], "allowed": 15}, 10), ({"tables": [_one(8)], "weights": [float("nan")], "allowed": 15}, 10),
                             ({"tables": [_one(8)], "weights": [float("inf")], "allowed": 15}, 10), ({"tables": [_one(8, sse=(0.0, 1e5, 1e5, 1e5))], "weights": [1e308], "allowed": 15}, 10),
                             ({"tables": [_one(8, sse=(0.0, float("inf"), 1.0, 1.0))], "weights": None, "allowed": 15}, 10),
                             ({"tables": [_one(8)], "weights": None, "allowed": 15}, -1)):
        assert choose(bad_inst, budget)[0] == INV
    # a sum of squares whose reciprocal overflows weighs like a table of zeros: no NaN reaches the ordering of the steps
    tiny = {"tables": [_one(64, sum_sq=5e-324, sse=(0.0, 0.0, 0.0, 0.0)), _one(64)], "weights": None, "allowed": 15}
    status, kinds, nbytes, err, _ = choose(tiny, 256000 + 72000)
    assert status == OK and kinds == (Q8, 0) and err == 0.0 and choose(tiny, 2 * 72000)[1] == (Q8, Q8)
    assert L.fcp_table_formats_choose(None, None, None, 1, 10, 15, None, None, None, None) == INV
    assert L.fcp_table_formats_choose(None, None, None, 0, 0, 15, None, None, None, None) == OK


def test_python_wrappers_refuse_what_they_can_see():
    import torch
    from recom_amd import tables
    import table_mixed_cases as TM
    with pytest.raises(ValueError, match="device to device"):
        tables.audit(torch.zeros((4, 8)))
    with pytest.raises(ValueError, match="no table format"):
        tables.audit(torch.zeros((4, 8), dtype=torch.float64))
    spec = TM.small_mixed_spec()
    with pytest.raises(ValueError, match="audits names"):
        tables.choose_dtypes(spec, [None], 100)
    with pytest.raises(ValueError, match="no audit"):
        tables.choose_dtypes(spec, [None, None, None], 100)


def test_choose_dtypes_on_host_made_audits():
    """tables.choose_dtypes maps the library's answer onto the plan's device inputs: "-" for an input no column reads."""
    import dataclasses
    from recom_amd import tables
    import table_mixed_cases as TM
    spec = TM.small_mixed_spec()
    spec = dataclasses.replace(spec, n_device_inputs=4)                       # a fourth device input nothing reads
    dims = {c.table_input: c.dim for c in spec.columns}
    inst = {"tables": [_one(dims[t], rows=TM.VOCAB) for t in range(3)], "weights": None, "allowed": 15}
    raw = _raw_audits(inst)
    audits = [tables._audit_of(raw[t], dims[t]) for t in range(3)] + [None]
    f32_bytes = sum(TM.VOCAB * 4 * dims[t] for t in range(3))
    names, nbytes, err = tables.choose_dtypes(spec, audits, f32_bytes)
    assert names == ("f32", "f32", "f32", "-") and nbytes == f32_bytes and err == 0.0
    names, nbytes, err = tables.choose_dtypes(spec, audits, f32_bytes, allowed=("bf16",), weights=[1.0, 1.0, 1.0, 5.0])
    assert names == ("f32", "f32", "f32", "-")
    names, nbytes, err = tables.choose_dtypes(spec, audits, f32_bytes // 2, allowed=("bf16", "f16"))
    assert names == ("f16", "f16", "f16", "-") and nbytes == f32_bytes // 2 and err == pytest.approx(3 * 2e-3 / 10.0)
    assert spec.with_table_dtypes(names).table_dtype == "f16"
    with pytest.raises(_lib.FcpError) as e:
        tables.choose_dtypes(spec, audits, 10)
    assert e.value.status == UNS
    assert audits[0].admissible("q8") and audits[0].kinds["q8"].sum_sq_err == 1e-3


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------
def test_the_chooser_alone_under_address_and_undefined_sanitizers(tmp_path):
    """recom_amd/csrc/fcp_plan_desc.cc links without the GPU runtime; a stand-alone program (tests/native/table_formats_san.cc),
    both built with -fsanitize=address,undefined, runs the chooser over the instances of the brute-force test and prints what it
    chose: the same answers as the library's, and no sanitizer report.  Nothing is loaded into python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "table_formats_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "native", "table_formats_san.cc"), os.path.join(CSRC, "fcp_plan_desc.cc"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        pytest.skip("libasan / libubsan not installed")
    assert build.returncode == 0, build.stderr
    path = str(tmp_path / "instances.txt")
    cases = TA.write_instances(path)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases) > 300
    for line, (inst, budget) in zip(lines, cases):
        status, kinds, nbytes, err, _ = choose(inst, budget)
        got = line.split()
        assert int(got[0]) == status and int(got[1]) == nbytes, (line, status, nbytes)
        if status == OK:
            assert float.fromhex(got[2]) == err and tuple(int(k) for k in got[3:]) == kinds, (line, kinds, err)
