"""CPU-only check of the plain dense kernel's block mapping (recom_amd/csrc/fcp_plain_map.h): tests/native/plain_map_check.cc
includes the header the kernel includes and enumerates every block of the grid for 1, 7, 8, 9, 15, 16, 17, 23 and 118 spans
by 1, 2, 3, 5 and 32 row tiles.  Conditions, not measurements: every (span, row tile) pair is owned by exactly one block,
the dead blocks number grid - spans * tiles, a block of a full group of eight spans maps as the generic kernel maps it, and
the live blocks of any two XCDs differ by at most one.  The generic mapping fails the last condition at 118 spans by 32
tiles (480 against 448 blocks per XCD), which the program asserts as well."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recom_amd", "csrc")


def test_every_block_of_the_grid_under_both_mappings(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "plain_map_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined",
                            "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "native", "plain_map_check.cc"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "118 spans x 32 tiles: even deal 472..472 live blocks per XCD, generic mapping 448..480" in run.stdout, run.stdout


def test_the_kernel_and_the_probe_call_the_header():
    """One mapping: the plain kernel and `fcp_bench --mix-probe` both call fcp_plain_locate and restate nothing."""
    for name in ("fcp_dense_plain.hip", "fcp_bench_main.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "fcp_plain_map.h"' in text and "fcp_plain_locate(blockIdx.x, nsp8, nlist, deal_tiles, idx, tile)" in text, name
        assert "% nsp8" not in text and "/ nsp8" not in text, name
