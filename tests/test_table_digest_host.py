"""fcp_table_digest / fcp_table_digest_rows / fcp_table_digest_host without a GPU: the ABI's surface and the struct's layout,
fcp_table_digest_host against the NumPy reference of the header's value model (known answers, every kind and dim, every q8 tail),
the shard and chunk identities, what the digest is sensitive to, every FCP_ERR_INVALID_ARGUMENT of both device entries in
the documented order, what the Python wrappers refuse, and the host unit alone under the address and undefined-behaviour
sanitizers.  (The kernels: tests/test_gpu_table_digest.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import table_digest_cases as TD
from recom_amd import lib as _lib
from recom_amd import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
CSRC = os.path.join(ROOT, "recom_amd", "csrc")
INV, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK
A = 1 << 20          # (pointers are never dereferenced on the host: plain numbers serve)
I64_MAX = (1 << 63) - 1


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_four_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint64_t fcp_table_digest_workspace_bytes\(void\);", text)
    assert re.search(r"\bint fcp_table_digest\(const void \*first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step,\s+"
                     r"fcp_table_digest_t \*out, void \*workspace, int32_t device, void \*stream\);", text)
    assert re.search(r"\bint fcp_table_digest_rows\(const void \*table, int32_t kind, int64_t table_rows, int32_t dim, int64_t row0, "
                     r"int64_t row_step,\s+const int64_t \*row_ids, int64_t n, fcp_table_digest_t \*out, void \*workspace, int32_t device, "
                     r"void \*stream\);", text)
    assert re.search(r"\buint64_t fcp_table_digest_host\(const void \*first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, "
                     r"int64_t row_step\);", text)
    assert "not a mac" in text.lower()
    names = {"fcp_table_digest_workspace_bytes", "fcp_table_digest", "fcp_table_digest_rows", "fcp_table_digest_host"}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names)
    ws = L.fcp_table_digest_workspace_bytes()
    assert ws > 0 and ws % 8 == 0 and ws == L.fcp_table_digest_workspace_bytes()
    # the header's surface and the mirror agree (tests/test_host.py holds the same for every entry)
    assert set(re.findall(r"\b(fcp_[a-z_0-9]+)\s*\(", text)) - {"fcp_alloc_fn"} == set(_lib.EXPORTS)


def test_struct_is_32_bytes_and_matches_a_compiled_c99_snippet(tmp_path):
    assert C.sizeof(_lib.TableDigest) == 32
    assert [(f, getattr(_lib.TableDigest, f).offset) for f, _ in _lib.TableDigest._fields_] == [("sum", 0), ("rows", 8), ("skipped", 16), ("reserved", 24)]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ("sum", "rows", "skipped", "reserved")
    prints = '  printf("size %zu\\n", sizeof(fcp_table_digest_t));\n' + "".join(
        f'  printf("{f} %zu\\n", offsetof(fcp_table_digest_t, {f}));\n' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fcp_hip.h"\nint main(void) {\n' + prints + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", exe], check=True, capture_output=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == 32
    for f in fields:
        assert int(got[f]) == getattr(_lib.TableDigest, f).offset, f


# ---- the host digest against the reference --------------------------------------------------------------------------------------
def test_the_reference_on_itself():
    assert int(TD.mix(1)[0]) == 0xb456bcfc34c2cb2c
    for raw, kind, dim, want in TD.KNOWN:
        assert TD.digest(raw, kind, dim) == want, (kind, dim)


def test_known_answers():
    for raw, kind, dim, want in TD.KNOWN:
        got = tables.digest_host(np.frombuffer(raw, np.uint8), kind, dim=dim)
        assert got == want, (kind, dim, hex(got), hex(want))
    assert tables.digest_host(np.arange(9, dtype=np.float32).reshape(3, 3), "f32") == 0xb3c088b12d9a2c7b
    assert tables.digest_host(np.arange(26, dtype=np.uint8).reshape(2, 13), "q8") == 0xf02c1c2d5524c510


def test_random_tables_of_every_kind_and_dim():
    cases = TD.host_cases()
    assert {(k, d) for k, d, *_ in cases} >= {(k, d) for k in TD.KINDS for d in TD.DIMS}
    assert {TD.row_bytes("q8", d) for k, d, *_ in cases if k == "q8"} >= set(range(9, 17))
    for kind, dim, rows, row0, step, raw in cases:
        want = TD.digest(raw.tobytes(), kind, dim, row0, step)
        got = tables.digest_host(raw, kind, dim=dim, row0=row0, row_step=step)
        assert got == want, (kind, dim, rows, row0, step, hex(got), hex(want))
        assert (got == 0) == (rows == 0)


def test_torch_host_tensors_in_their_own_dtype():
    import torch
    x = torch.randn((6, 10), generator=torch.Generator().manual_seed(3))
    for kind, t in (("f32", x), ("bf16", x.to(torch.bfloat16)), ("f16", x.to(torch.float16)),
                    ("q8", torch.arange(6 * 18, dtype=torch.uint8).reshape(6, 18))):
        raw = t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        assert tables.digest_host(t, kind) == TD.digest(raw, kind, 10), kind
        assert tables.digest_host(t[2:], kind, row0=2) == TD.digest(raw, kind, 10) - TD.digest(raw[:2 * len(raw) // 6], kind, 10) & TD.M64


@pytest.mark.parametrize("kind", TD.KINDS)
def test_shards_and_chunks_add_up(kind):
    dim, rows = 5, 23                        # 23: divisible by none of the worlds
    raw = TD.draw_raw(kind, dim, rows, 11)
    whole = tables.digest_host(raw, kind, dim=dim)
    assert whole == TD.digest(raw.tobytes(), kind, dim)
    for world in (2, 3, 8):
        parts = [tables.digest_host(np.ascontiguousarray(raw[g::world]), kind, dim=dim, row0=g, row_step=world) for g in range(world)]
        assert sum(parts) & TD.M64 == whole, world
    for chunk in (1, 7, rows):
        parts = [tables.digest_host(raw[a:a + chunk], kind, dim=dim, row0=a) for a in range(0, rows, chunk)]
        assert sum(parts) & TD.M64 == whole, chunk


def test_what_the_digest_is_sensitive_to():
    raw = TD.draw_raw("f32", 6, 9, 13)       # rows of 24 bytes: three words
    base = tables.digest_host(raw, "f32", dim=6)
    seen = {base}
    flipped = raw.copy()
    flipped[4, 17] ^= 0x10                   # one bit
    seen.add(tables.digest_host(flipped, "f32", dim=6))
    swapped = raw.copy()
    swapped[[2, 7]] = raw[[7, 2]]            # two rows
    seen.add(tables.digest_host(swapped, "f32", dim=6))
    words = raw.copy()
    words[3, 0:8], words[3, 8:16] = raw[3, 8:16], raw[3, 0:8]      # two words of a row
    seen.add(tables.digest_host(words, "f32", dim=6))
    seen.add(tables.digest_host(raw, "f32", dim=6, row0=1))          # the rows one index further
    seen.add(tables.digest_host(raw.reshape(-1), "f32", dim=3))      # the same bytes at another dim
    seen.add(tables.digest_host(raw.reshape(-1), "bf16", dim=12))    # ... and as another kind of the same row bytes
    seen.add(tables.digest_host(raw.reshape(-1), "f16", dim=12))     # bf16 against fp16
    assert len(seen) == 8


# ---- status codes ----------------------------------------------------------------------------------------------------------------
def _digest(first_row, kind, rows, dim, row0, step, out, workspace, device=0):
    L = _lib.load()
    status = L.fcp_table_digest(C.c_void_p(first_row), kind, rows, dim, row0, step, C.c_void_p(out), C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def _digest_rows(table, kind, table_rows, dim, row0, step, row_ids, n, out, workspace, device=0):
    L = _lib.load()
    status = L.fcp_table_digest_rows(C.c_void_p(table), kind, table_rows, dim, row0, step, C.c_void_p(row_ids), n, C.c_void_p(out),
                                     C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def test_digest_status_codes_arrive_in_the_stated_order():
    import torch
    no_gpu = not torch.cuda.is_available()      # (with a GPU valid arguments would run: only the device-free statuses are checked)
    for args, word in (((A, 0, -1, 64, 0, 1, A, A), "`rows`"), ((A, 0, 2 ** 32 - 3, 64, 0, 1, A, A), "`rows`"), ((A, 0, 2 ** 40, 64, 0, 1, A, A), "`rows`"),
                       ((A, 0, 5, 0, 0, 1, A, A), "`dim`"), ((A, 0, 5, -3, 0, 1, A, A), "`dim`"),
                       ((A, 4, 5, 64, 0, 1, A, A), "`kind`"), ((A, -1, 5, 64, 0, 1, A, A), "`kind`"), ((A, 255, 5, 64, 0, 1, A, A), "`kind`"),
                       ((A, 0, 5, 2 ** 29, 0, 1, A, A), "`dim`"),                                   # float32 rows of 2 GiB
                       ((A, 0, 5, 64, -1, 1, A, A), "`row0`"),
                       ((A, 0, 5, 64, 0, 0, A, A), "`row_step`"), ((A, 0, 5, 64, 0, -2, A, A), "`row_step`"),
                       ((A, 0, 2, 64, I64_MAX, 1, A, A), "overflows"), ((A, 0, 3, 64, 0, I64_MAX, A, A), "overflows"),
                       ((A, 0, 3, 64, I64_MAX - 3, 2, A, A), "overflows"),
                       ((A, 0, 5, 64, 0, 1, 0, A), "`out`"), ((A, 0, 0, 64, 0, 1, 0, A), "`out`"),
                       ((A, 0, 5, 64, 0, 1, A, 0), "`workspace`"), ((0, 0, 0, 64, 0, 1, A, 0), "`workspace`"),
                       ((0, 0, 5, 64, 0, 1, A, A), "`first_row`"), ((0, 3, 1, 1, 0, 1, A, A), "`first_row`"),
                       ((A + 8, 0, 5, 64, 0, 1, A, A), "`first_row`"), ((A + 4, 0, 5, 62, 0, 1, A, A), "`first_row`"),     # float32: 16, 8
                       ((A + 2, 0, 5, 61, 0, 1, A, A), "`first_row`"),                                                   # ... 4
                       ((A + 4, 1, 5, 64, 0, 1, A, A), "`first_row`"), ((A + 2, 2, 5, 62, 0, 1, A, A), "`first_row`"),     # 16-bit: 8, 4
                       ((A + 1, 1, 5, 61, 0, 1, A, A), "`first_row`"),                                                   # ... 2
                       ((A, 0, 5, 64, 0, 1, A + 4, A), "`out`"), ((A + 3, 3, 5, 64, 0, 1, A + 4, A), "`out`"),
                       ((A, 0, 5, 64, 0, 1, A, A + 4), "`workspace`")):
        status, msg = _digest(*args)
        assert status == INV and word in msg and msg.startswith("fcp_table_digest: "), (args, status, msg)
    # the order: rows, dim, kind, row0, row_step, the overflow, null out / workspace / first_row, alignment of first_row / out / workspace
    assert "`rows`" in _digest(0, 9, -1, 0, -1, 0, 0, 0)[1]
    assert "`dim`" in _digest(0, 9, 5, 0, -1, 0, 0, 0)[1]
    assert "`kind`" in _digest(0, 9, 5, 3, -1, 0, 0, 0)[1]
    assert "`row0`" in _digest(0, 0, 5, 3, -1, 0, 0, 0)[1]
    assert "`row_step`" in _digest(0, 0, 5, 3, I64_MAX, 0, 0, 0)[1]
    assert "overflows" in _digest(0, 0, 5, 3, I64_MAX, 1, 0, 0)[1]
    assert "`out`" in _digest(0, 0, 5, 3, 0, 1, 0, 0)[1]
    assert "`workspace`" in _digest(0, 0, 5, 3, 0, 1, A + 4, 0)[1]
    assert "`first_row`" in _digest(0, 0, 5, 3, 0, 1, A + 4, A + 4)[1]
    assert "`first_row`" in _digest(A + 2, 0, 5, 3, 0, 1, A + 4, A + 4)[1]
    assert "`out`" in _digest(A + 4, 0, 5, 3, 0, 1, A + 4, A + 4)[1]
    assert "`workspace`" in _digest(A + 4, 0, 5, 3, 0, 1, A, A + 4)[1]
    if no_gpu:
        # alignments that ARE enough (q8: any byte), rows == 0 with a null first_row, the ends of rows, row0 and row_step
        for args in ((A + 16, 0, 5, 64, 0, 1, A, A), (A + 8, 0, 5, 62, 0, 1, A, A), (A + 4, 0, 5, 61, 0, 1, A + 8, A + 8),
                     (A + 8, 1, 5, 64, 0, 1, A, A), (A + 4, 2, 5, 62, 0, 1, A, A), (A + 2, 1, 5, 61, 0, 1, A, A),
                     (A + 1, 3, 5, 64, 0, 1, A, A), (A + 7, 3, 5, 1, 0, 1, A, A), (0, 0, 0, 64, 0, 1, A, A),
                     (A, 0, 2 ** 32 - 4, 64, 0, 1, A, A), (A, 0, 2, 64, I64_MAX - 1, 1, A, A), (A, 0, 1, 64, I64_MAX, I64_MAX, A, A)):
            assert _digest(*args)[0] == NODEV, args


def test_digest_rows_status_codes_arrive_in_the_stated_order():
    import torch
    no_gpu = not torch.cuda.is_available()
    for args, word in (((A, 0, 9, 64, 0, 1, A, -1, A, A), "`n`"), ((A, 0, 9, 64, 0, 1, A, 2 ** 32 - 3, A, A), "`n`"),
                       ((A, 0, -1, 64, 0, 1, A, 3, A, A), "`table_rows`"), ((A, 0, 2 ** 32 - 3, 64, 0, 1, A, 3, A, A), "`table_rows`"),
                       ((A, 0, 9, 0, 0, 1, A, 3, A, A), "`dim`"),
                       ((A, 4, 9, 64, 0, 1, A, 3, A, A), "`kind`"), ((A, 255, 9, 64, 0, 1, A, 3, A, A), "`kind`"),
                       ((A, 0, 9, 64, -1, 1, A, 3, A, A), "`row0`"), ((A, 0, 9, 64, 0, 0, A, 3, A, A), "`row_step`"),
                       ((A, 0, 9, 64, I64_MAX - 7, 1, A, 3, A, A), "overflows"), ((A, 0, 3, 64, 0, I64_MAX, A, 0, A, A), "overflows"),
                       ((A, 0, 9, 64, 0, 1, A, 3, 0, A), "`out`"), ((0, 0, 9, 64, 0, 1, 0, 0, 0, A), "`out`"),
                       ((A, 0, 9, 64, 0, 1, A, 3, A, 0), "`workspace`"),
                       ((0, 0, 9, 64, 0, 1, A, 3, A, A), "`table`"), ((A, 0, 9, 64, 0, 1, 0, 3, A, A), "`row_ids`"),
                       ((A + 8, 0, 9, 64, 0, 1, A, 3, A, A), "`table`"), ((A + 1, 2, 9, 61, 0, 1, A, 3, A, A), "`table`"),
                       ((A, 0, 9, 64, 0, 1, A + 4, 3, A, A), "`row_ids`"), ((A + 5, 3, 9, 64, 0, 1, A + 4, 0, A, A), "`row_ids`"),
                       ((A, 0, 9, 64, 0, 1, A, 3, A + 4, A), "`out`"), ((A, 0, 9, 64, 0, 1, A, 3, A, A + 4), "`workspace`")):
        status, msg = _digest_rows(*args)
        assert status == INV and word in msg and msg.startswith("fcp_table_digest_rows: "), (args, status, msg)
    assert "`n`" in _digest_rows(0, 9, -1, 0, -1, 0, 0, -1, 0, 0)[1]
    assert "`table_rows`" in _digest_rows(0, 9, -1, 0, -1, 0, 0, 3, 0, 0)[1]
    assert "`dim`" in _digest_rows(0, 9, 9, 0, -1, 0, 0, 3, 0, 0)[1]
    assert "`kind`" in _digest_rows(0, 9, 9, 3, -1, 0, 0, 3, 0, 0)[1]
    assert "`row0`" in _digest_rows(0, 1, 9, 3, -1, 0, 0, 3, 0, 0)[1]
    assert "`row_step`" in _digest_rows(0, 1, 9, 3, I64_MAX, 0, 0, 3, 0, 0)[1]
    assert "overflows" in _digest_rows(0, 1, 9, 3, I64_MAX, 1, 0, 3, 0, 0)[1]
    assert "`out`" in _digest_rows(0, 1, 9, 3, 0, 1, 0, 3, 0, 0)[1]
    assert "`workspace`" in _digest_rows(0, 1, 9, 3, 0, 1, 0, 3, A + 4, 0)[1]
    assert "`table`" in _digest_rows(0, 1, 9, 3, 0, 1, 0, 3, A + 4, A + 4)[1]
    assert "`row_ids`" in _digest_rows(A + 1, 1, 9, 3, 0, 1, 0, 3, A + 4, A + 4)[1]
    assert "`table`" in _digest_rows(A + 1, 1, 9, 3, 0, 1, A + 4, 3, A + 4, A + 4)[1]
    assert "`row_ids`" in _digest_rows(A + 2, 1, 9, 3, 0, 1, A + 4, 3, A + 4, A + 4)[1]
    assert "`out`" in _digest_rows(A + 2, 1, 9, 3, 0, 1, A + 8, 3, A + 4, A + 4)[1]
    assert "`workspace`" in _digest_rows(A + 2, 1, 9, 3, 0, 1, A + 8, 3, A, A + 4)[1]
    if no_gpu:
        # a table of no rows may have no address; n == 0 may have no ids; q8 at any byte; the ends of the ranges
        for args in ((A, 0, 9, 64, 0, 1, A, 3, A, A), (0, 0, 0, 64, 0, 1, A, 3, A, A), (0, 0, 9, 64, 0, 1, 0, 0, A, A),
                     (A + 3, 3, 9, 64, 0, 1, A + 8, 3, A, A), (A, 0, 2 ** 32 - 4, 64, 5, 7, A, 2 ** 32 - 4, A, A),
                     (A, 0, 2, 64, I64_MAX - 1, 1, A, 3, A, A)):
            assert _digest_rows(*args)[0] == NODEV, args


def test_python_wrappers_refuse_what_they_can_see():
    import torch
    t = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="device to device"):
        tables.digest(t)
    with pytest.raises(ValueError, match="device to device"):
        tables.digest_rows(t, torch.zeros((3,), dtype=torch.int64))
    with pytest.raises(ValueError, match="device to device"):
        tables.update_rows_tracked(t, torch.zeros((3,), dtype=torch.int64), torch.zeros((3, 8)), 0)
    with pytest.raises(ValueError, match="no table format"):
        tables.digest(torch.zeros((4, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match="unknown table dtype"):
        tables.digest_host(np.zeros((4, 8), np.float32), "f64")
    with pytest.raises(ValueError, match="needs dim="):
        tables.digest_host(np.zeros(32, np.float32), "f32")
    with pytest.raises(ValueError, match="no whole number"):
        tables.digest_host(np.zeros(33, np.uint8), "f32", dim=2)
    with pytest.raises(ValueError, match="no rows of a q8 table"):
        tables.digest_host(np.zeros((3, 8), np.uint8), "q8")
    with pytest.raises(ValueError, match="row_step"):
        tables.digest_host(np.zeros((3, 8), np.float32), "f32", row_step=0)


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------
def test_the_host_unit_alone_under_address_and_undefined_sanitizers(tmp_path):
    """recom_amd/csrc/fcp_table_digest_host.cc links without the GPU runtime and without any other unit; a stand-alone program
    (tests/native/table_digest_san.cc), both built with -fsanitize=address,undefined, digests the case file — every row block a
    heap block of exactly rows * row bytes — and prints `0 failures`, with no sanitizer report.  Nothing is loaded into python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "table_digest_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "native", "table_digest_san.cc"), os.path.join(CSRC, "fcp_table_digest_host.cc"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        pytest.skip("libasan / libubsan not installed")
    assert build.returncode == 0, build.stderr
    path = str(tmp_path / "cases.txt")
    n = TD.write_cases(path)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-2:] == [f"{n} cases", "0 failures"] and n == len(TD.KNOWN) + len(TD.host_cases()) >= 170, lines[-5:]
