"""CPU-only checks of the plain dense kernel's front (recom_amd/csrc/fcp_dense_plain.hip), read from the gfx950 assembly:
the id facts come through a 16-byte scalar load, no LDS read stands in front of the first id load, and DESIGN.md states
the kernel's instruction count."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _body(tmp_path):
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
    name = re.search(r"\.amdhsa_kernel (\S*fcp_dense_kernel_plain\S*)", text).group(1)
    label = re.search(r"^" + re.escape(name) + r":", text, re.M)
    body = text[label.end():text.index(".amdhsa_kernel " + name)]
    return [ln.split(";")[0].strip() for ln in body.splitlines()]


def test_front_of_the_plain_dense_kernel(tmp_path):
    lines = _body(tmp_path)
    insns = [ln for ln in lines if re.match(r"[a-z]\w*(\s|$)", ln)]
    mnem = [ln.split()[0] for ln in insns]
    # the id facts: a 16-byte scalar load from the span record (the kernel arguments are preloaded or read at 0x0 .. 0x28
    # from the kernarg pointer s[0:1]: not those)
    facts = [ln for ln in insns if ln.startswith("s_load_dwordx4") and not re.search(r"s\[0:1\]", ln)]
    assert facts, "no 16-byte scalar load of id facts"
    # the first id load: the first 4-byte or 8-byte vector load (the record is read 16 bytes per thread)
    first_id = next(i for i, m in enumerate(mnem) if m in ("global_load_dword", "global_load_dwordx2"))
    assert insns.index(facts[0]) < first_id
    assert "global_load_dwordx4" in mnem[:first_id], "the record's vector read is no longer issued before the id loads"
    lds_reads = [m for m in mnem[:first_id] if m.startswith("ds_read")]
    assert not lds_reads, lds_reads
    assert "s_barrier" not in mnem[:first_id]
    # the record goes to LDS behind the id loads, then the barrier
    assert "ds_write_b128" in mnem[first_id:] and mnem.index("s_barrier") > first_id

    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    stated = re.search(r"fcp_dense_kernel_plain<4> is (\d+) instructions", design)
    assert stated, "DESIGN.md does not state the plain kernel's instruction count"
    assert int(stated.group(1)) == len(insns), (int(stated.group(1)), len(insns))
