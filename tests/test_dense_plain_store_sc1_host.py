"""CPU-only: the gfx950 code object of the plain dense kernel (recom_amd/csrc/fcp_dense_plain.hip) keeps its four output
store forms as four instructions — `sc1`, `sc1 nt`, `nt` and plain, one of each per row of a lane — and its footprint: at
most 64 VGPRs, no scratch, 7 760 bytes of LDS, 14 argument dwords preloaded into SGPRs.  (Written as C++ branches the
compiler once merged two of the forms into one and dropped the hint: tests/test_host.py,
test_hot_kernels_keep_full_occupancy.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_dense_kernel_has_four_store_forms_and_its_footprint(tmp_path):
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
    assert len(kernels) == 1 and "fcp_dense_kernel_plain" in kernels[0][0], [k for k, _ in kernels]
    name, desc = kernels[0]

    def field(key):
        return int(re.search(r"\.amdhsa_" + key + r" (\d+)", desc).group(1))
    assert field("next_free_vgpr") <= 64
    assert field("private_segment_fixed_size") == 0
    assert field("group_segment_fixed_size") == 7760
    assert field("user_sgpr_kernarg_preload_length") == 14

    label = re.search(r"^" + re.escape(name) + r":", text, re.M)
    body = text[label.end():text.index(".amdhsa_kernel " + name)]
    kinds = {"sc1": 0, "sc1 nt": 0, "nt": 0, "plain": 0}
    for st in re.findall(r"global_store_dwordx4 [^\n]*", body):
        tail = st.split(";")[0].split("off", 1)[1].split()
        kinds[" ".join(tail) if tail else "plain"] += 1
    assert all(n >= 4 for n in kinds.values()), kinds
