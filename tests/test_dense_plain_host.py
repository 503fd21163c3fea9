"""CPU-only checks of the plain dense kernel (recom_amd/csrc/fcp_dense_plain.hip): the limits its code object must keep,
read from the gfx950 assembly, and which cells of the kernel matrix its gate can reach."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 4   # rows per wave of the one instantiation


def test_code_object_of_the_plain_dense_kernel(tmp_path):
    """fcp_dense_kernel_plain<4>: at most 64 VGPRs (eight waves per SIMD), no scratch, LDS for eight blocks per CU (160 KiB),
    fp32 subnormals kept and IEEE mode like every fused kernel, its arguments preloaded into SGPRs, and the three output
    stores — `sc1 nt`, `nt` and plain global_store_dwordx4 — each at least R times (st_out must not merge two policies)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    make = open(os.path.join(ROOT, "recom_amd", "csrc", "Makefile")).read()
    extra = re.search(r"fcp_dense_plain\.o: FLAGS \+= (.*)", make)
    assert extra, "the Makefile no longer gives fcp_dense_plain.o its own flags"
    asm = tmp_path / "plain.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S"] + extra.group(1).split() +
                       [os.path.join(ROOT, "recom_amd", "csrc", "fcp_dense_plain.hip"), "-o", str(asm)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert len(kernels) == 1 and "fcp_dense_kernel_plain" in kernels[0][0] and "ILi4E" in kernels[0][0], [k for k, _ in kernels]
    name, desc = kernels[0]
    assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc) and re.search(r"\.amdhsa_ieee_mode 1\b", desc)
    assert int(re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", desc).group(1)) >= 14
    meta = text[text.index("amdhsa.kernels:"):]
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta).group(1)) <= 160 * 1024 // 8
    assert int(re.search(r"\.kernarg_segment_size:\s+(\d+)", meta).group(1)) <= 16 * 4
    label = re.search(r"^" + re.escape(name) + r":", text, re.M)
    body = text[label.end():text.index(".amdhsa_kernel " + name)]
    stores = re.findall(r"^\s*global_store_dwordx4\s+[^\n]*?off([^\n]*)$", body, re.M)
    kinds = [" ".join(s.split("//")[0].split()) for s in stores]
    assert kinds.count("sc1 nt") >= R and kinds.count("nt") >= R and kinds.count("") >= R, kinds
    assert "scratch_" not in body and "flat_load" not in body and "flat_store" not in body


def test_no_cell_of_the_kernel_matrix_qualifies_for_the_plain_kernel():
    """tests/kernel_variant_cases.py pins fcp_dense_kernel<4, 4, false>: its dense V 4 / R 4 plans must stay on that
    instantiation.  Each of them has passthrough columns and gathers with an id filter, which the plain kernel's gate
    refuses, so none of those cells moves to fcp_dense_kernel_plain."""
    import kernel_variant_cases as K
    from recom_amd.plan import FORM_GATHER, XFORM_NONE
    keys = {c.key for c in K.cells() if c.kernel == "dense" and c.vec == 4 and c.rpw == 4}
    assert keys
    for key in keys:
        cols = K.build_case(*key).spec.columns
        assert any(c.form != FORM_GATHER or c.xform_mode != XFORM_NONE for c in cols), key
