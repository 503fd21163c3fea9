"""fcp_tables_digest / fcp_tables_digest_launches / fcp_tables_digest_workspace_bytes without a GPU: the C ABI's surface, the
workspace formula, the status order with its `entry k` messages, the launch count and the deal of blocks against their Python
restatement (tests/tables_digest_cases.py), the Python wrappers' refusals, the code object of
recom_amd/csrc/fcp_tables_digest.hip, and the host-only plan unit (recom_amd/csrc/fcp_tables_digest_plan.cc) alone under the
sanitizers.  (The kernels themselves: tests/test_zzz_gpu_tables_digest.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import table_digest_cases as TD
import tables_digest_cases as GD
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
CSRC = os.path.join(ROOT, "recom_amd", "csrc")
F32, BF16, F16, Q8 = (TD.KIND[k] for k in ("f32", "bf16", "f16", "q8"))
A = 1 << 20                                                   # an address aligned for everything
NAMES = ("fcp_tables_digest_workspace_bytes", "fcp_tables_digest_launches", "fcp_tables_digest")
INV, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK
WHO = "fcp_tables_digest: "


def _rows(kind=Q8, dim=64, rows=100, table=A, row0=0, step=1, n=0, reserved=0):
    """an entry of rows back to back"""
    return _lib.TableDigestEntry(table, None, rows, n, row0, step, kind, dim, reserved)


def _ids(kind=Q8, dim=64, n=5, table_rows=100, table=A, ids=A, row0=0, step=1, reserved=0):
    """an entry by id"""
    return _lib.TableDigestEntry(table, ids, table_rows, n, row0, step, kind, dim, reserved)


def _array(entries):
    return (_lib.TableDigestEntry * max(len(entries), 1))(*entries)


def _call(entries, n_tables=None, out=A, workspace=A, device=0):
    L = _lib.load()
    status = L.fcp_tables_digest(_array(entries) if entries is not None else None, len(entries) if n_tables is None else n_tables,
                                 C.c_void_p(out), C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def _launches(entries, n_tables=None, want_blocks=False):
    n = len(entries) if n_tables is None else n_tables
    blocks = (C.c_int32 * max(len(entries), 1))(*([-7] * max(len(entries), 1)))
    got = int(_lib.load().fcp_tables_digest_launches(_array(entries), n, blocks if want_blocks else None))
    return (got, list(blocks[:len(entries)])) if want_blocks else got


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert "int64_t fcp_tables_digest_workspace_bytes(int32_t n_tables);" in text
    assert ("int32_t fcp_tables_digest_launches(const fcp_table_digest_entry_t *entries, int32_t n_tables, "
            "int32_t *blocks /* host [n_tables] or NULL */);") in text
    assert ("int fcp_tables_digest(const fcp_table_digest_entry_t *entries, int32_t n_tables, fcp_table_digest_t *out /* device [n_tables] */, "
            "void *workspace, int32_t device, void *stream);") in text
    assert "} fcp_table_digest_entry_t;" in text
    assert set(NAMES) <= set(_lib.EXPORTS)
    L = _lib.load()
    for name in NAMES:
        assert hasattr(L, name), name
    # behind the single-table digest, and the ABI is append-only
    assert text.index("uint64_t fcp_table_digest_host(") < text.index("typedef struct fcp_table_digest_entry {")
    assert re.search(r"#define FCP_ABI_VERSION 2\b", text) and _lib.FCP_ABI_VERSION == 2 and L.fcp_abi_version() == 2


def test_the_entry_struct_is_64_bytes_in_c_and_in_python(tmp_path):
    assert C.sizeof(_lib.TableDigestEntry) == 64
    offsets = {f: getattr(_lib.TableDigestEntry, f).offset for f, _t in _lib.TableDigestEntry._fields_}
    assert offsets == {"table": 0, "row_ids": 8, "rows": 16, "n": 24, "row0": 32, "row_step": 40, "kind": 48, "dim": 52, "reserved": 56}
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fcp_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(fcp_table_digest_entry_t), offsetof(fcp_table_digest_entry_t, n), offsetof(fcp_table_digest_entry_t, row_step), '
                   'offsetof(fcp_table_digest_entry_t, dim), offsetof(fcp_table_digest_entry_t, reserved)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["64", "24", "40", "52", "56"]


def test_workspace_formula():
    """A function of n_tables alone: -1 outside [0, 65536], a multiple of 8, non-decreasing, and room for one 64-byte record, one
    first-block value, one run and one 32-byte partial record per entry, and for the 8192 partial records of the deal."""
    ws = _lib.load().fcp_tables_digest_workspace_bytes
    assert ws(-1) == -1 and ws(65537) == -1 and ws(-2 ** 31) == -1 and ws(2 ** 31 - 1) == -1
    sizes = [int(ws(n)) for n in range(0, 65537)]
    assert all(s > 0 and s % 8 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(s >= 16 + (64 + 4 + 8 + 32) * n + 32 * GD.DEAL_BLOCKS for n, s in enumerate(sizes))
    assert sizes[65536] < 8 << 20


# ---- status order ------------------------------------------------------------------------------------------------------------
def test_status_codes_arrive_in_the_stated_order():
    """n_tables; `entries`; the entries in ascending order, each by the matching single-table entry's own order, then `reserved`,
    then `n` without `row_ids`; `out`; `workspace`.  Then FCP_OK for n_tables == 0, without a device; then, on a machine without
    a GPU, FCP_ERR_NO_DEVICE.  (Pointers are never dereferenced on the host: plain numbers serve.)"""
    import torch
    no_gpu = not torch.cuda.is_available()
    good, good_ids = _rows(), _ids()
    for n_tables in (-1, 65537, -2 ** 31, 2 ** 31 - 1):
        status, msg = _call([good], n_tables=n_tables)
        assert status == INV and "`n_tables`" in msg and msg.startswith(WHO), (n_tables, status, msg)
    status, msg = _call(None, n_tables=3)
    assert status == INV and "`entries`" in msg, msg
    assert "`n_tables`" in _call(None, n_tables=-5)[1]                  # n_tables comes before entries
    # per entry, the matching single-table entry's checks, named as it names them, with `entry k`
    limit = 2 ** 32 - 3
    bads = ((_rows(rows=-1), "rows"), (_rows(rows=limit), "rows"), (_rows(dim=0), "dim"), (_rows(kind=4), "kind"), (_rows(kind=-1), "kind"),
            (_rows(kind=F32, dim=2 ** 29), "dim"), (_rows(row0=-1), "row0"), (_rows(step=0), "row_step"),
            (_rows(rows=3, row0=2 ** 62, step=2 ** 62), "row0"), (_rows(table=0), "first_row"), (_rows(kind=BF16, dim=2, table=A + 2), "first_row"),
            (_rows(kind=F32, dim=1, table=A + 2), "first_row"), (_rows(reserved=1), "reserved"), (_rows(rows=0, reserved=-1), "reserved"),
            (_rows(n=3), "n"), (_rows(rows=0, table=0, n=-1), "n"),
            (_ids(n=-1), "n"), (_ids(n=limit), "n"), (_ids(table_rows=-1), "table_rows"), (_ids(table_rows=limit), "table_rows"),
            (_ids(dim=-3), "dim"), (_ids(kind=9), "kind"), (_ids(row0=-2), "row0"), (_ids(step=-1), "row_step"), (_ids(table=0), "table"),
            (_ids(kind=F16, dim=4, table=A + 4), "table"), (_ids(ids=A + 4), "row_ids"), (_ids(reserved=2), "reserved"),
            (_ids(n=0, reserved=2), "reserved"))
    for bad, word in bads:
        for k in (0, 1, 4):
            entries = [good, good_ids, good_ids, good][:k] + [bad] + [good_ids] * 2
            status, msg = _call(entries)
            assert status == INV and msg.startswith(f"{WHO}entry {k}: ") and f"`{word}`" in msg, (word, k, status, msg)
            assert _launches(entries) == -INV
    # the text behind `entry k: ` is the single-table entry's own, without its name
    L = _lib.load()
    assert L.fcp_table_digest(C.c_void_p(A), Q8, -1, 64, 0, 1, C.c_void_p(A), C.c_void_p(A), 0, None) == INV
    single = L.fcp_last_error().decode()
    assert single.startswith("fcp_table_digest: ") and _call([good, _rows(rows=-1)])[1] == f"{WHO}entry 1: " + single[len("fcp_table_digest: "):]
    assert L.fcp_table_digest_rows(C.c_void_p(A), Q8, 2 ** 32, 64, 0, 1, C.c_void_p(A), 5, C.c_void_p(A), C.c_void_p(A), 0, None) == INV
    single = L.fcp_last_error().decode()
    assert _call([_ids(table_rows=2 ** 32)])[1] == f"{WHO}entry 0: " + single[len("fcp_table_digest_rows: "):]
    # inside an entry the order is rows, dim, kind, row0, row_step, the pointer, its alignment, reserved, n
    for bad, word in ((_rows(rows=-1, dim=0, kind=9, row0=-1, step=0, table=0, reserved=1, n=1), "rows"),
                      (_rows(dim=0, kind=9, row0=-1, step=0, table=0, reserved=1, n=1), "dim"),
                      (_rows(kind=9, row0=-1, step=0, table=0, reserved=1, n=1), "kind"),
                      (_rows(row0=-1, step=0, table=0, reserved=1, n=1), "row0"),
                      (_rows(step=0, table=0, reserved=1, n=1), "row_step"),
                      (_rows(table=0, reserved=1, n=1), "first_row"),
                      (_rows(kind=F32, table=A + 1, reserved=1, n=1), "first_row"),
                      (_rows(reserved=1, n=1), "reserved"),
                      (_rows(n=1), "n"),
                      (_ids(n=-1, table_rows=-1, dim=0, kind=9, row0=-1, step=0, table=0, ids=A + 1, reserved=1), "n"),
                      (_ids(table_rows=-1, dim=0, kind=9, row0=-1, step=0, table=0, ids=A + 1, reserved=1), "table_rows"),
                      (_ids(dim=0, kind=9, row0=-1, step=0, table=0, ids=A + 1, reserved=1), "dim"),
                      (_ids(kind=9, row0=-1, step=0, table=0, ids=A + 1, reserved=1), "kind"),
                      (_ids(row0=-1, step=0, table=0, ids=A + 1, reserved=1), "row0"),
                      (_ids(step=0, table=0, ids=A + 1, reserved=1), "row_step"),
                      (_ids(table=0, ids=A + 1, reserved=1), "table"),
                      (_ids(kind=F32, table=A + 1, ids=A + 1, reserved=1), "table"),
                      (_ids(ids=A + 1, reserved=1), "row_ids"),
                      (_ids(reserved=1), "reserved")):
        status, msg = _call([bad], out=0, workspace=0)
        assert status == INV and msg.startswith(f"{WHO}entry 0: ") and f"`{word}`" in msg.split(": ", 2)[2].split(" ")[0], (word, status, msg)
    # the first bad entry wins; an entry wins over out and the workspace
    status, msg = _call([good, _rows(dim=0), _ids(n=-1)], out=A + 4, workspace=A + 4)
    assert status == INV and "entry 1: " in msg and "`dim`" in msg, msg
    # out: null with entries, misaligned; then the workspace
    for out, ws, word in ((0, 0, "out"), (A + 4, 0, "out"), (0, A + 4, "out"), (A, 0, "workspace"), (A, A + 4, "workspace")):
        status, msg = _call([good], out=out, workspace=ws)
        assert status == INV and f"`{word}`" in msg and "entry" not in msg and msg.startswith(WHO), (out, ws, msg)
    assert _call([], out=A + 4)[0] == INV and _call([], workspace=A + 2)[0] == INV      # an invalid argument wins over "nothing to do"
    # nothing to do: FCP_OK with no device, null pointers included
    assert _call([], out=0, workspace=0, device=12345)[0] == OK
    assert _call(None, n_tables=0, out=0, workspace=0, device=12345)[0] == OK
    assert _call([good], n_tables=0, device=12345)[0] == OK
    # entries: a device is needed even when none has rows (out is written on the device)
    if no_gpu:
        empty = [_rows(kind=k, dim=d, rows=0, table=0) for k in (F32, BF16, F16, Q8) for d in (64, 7)] + [_ids(n=0), _ids(table_rows=0, table=0)]
        assert _call(empty)[0] == NODEV
        for kind in (F32, BF16, F16, Q8):
            for dim in (64, 62, 61):
                assert _call([_rows(kind=kind, dim=dim), _ids(kind=kind, dim=dim)])[0] == NODEV
        assert _call([_rows(rows=limit - 1), _ids(n=limit - 1, table_rows=limit - 1)])[0] == NODEV      # the last values below the limits
        assert _call([_rows(kind=Q8, dim=1, table=A + 3), _ids(kind=Q8, dim=5, table=A + 1)])[0] == NODEV   # q8 rows start at any byte
        assert _call([good] * 65536)[0] == NODEV                            # the last n_tables


# ---- the launch count and the deal -----------------------------------------------------------------------------------------------
def _random_entries(rng):
    """entries and their description (address, kind, dim, count, by_id): every kind, the dims of TD.DIMS and the q8 tails, addresses
    of every alignment the kind allows, counts from 0 to beyond the fixed grid, both modes"""
    entries, described = [], []
    dims = TD.DIMS + TD.Q8_TAIL_DIMS + (16, 62)
    for _k in range(int(rng.integers(1, 60))):
        kind = KIND_NAMES[int(rng.integers(0, 4))]
        dim = int(rng.choice(dims))
        count = int(rng.choice((0, 0, 1, 63, 64, 65, 257, 5000, 100000, 600000, 2 ** 31)))
        elem = {"f32": 4, "bf16": 2, "f16": 2, "q8": 1}[kind] * (4 if dim % 4 == 0 else 2 if dim % 2 == 0 else 1)
        table = A + elem * int(rng.integers(0, 16)) if kind != "q8" else A + int(rng.integers(0, 16))
        if rng.integers(0, 2):
            entries.append(_ids(kind=TD.KIND[kind], dim=dim, n=count, table_rows=int(rng.integers(1, 2 ** 31)), table=table))
        else:
            entries.append(_rows(kind=TD.KIND[kind], dim=dim, rows=count, table=table))
        described.append((table, kind, dim, count, bool(entries[-1].row_ids)))
    return entries, described


KIND_NAMES = TD.KINDS


def test_launches_and_blocks_match_the_restated_rules():
    """One upload, one launch per class (A, G, by-id) present, one fold; blocks[k] is at least 1 exactly when the entry has rows,
    no more than the lone grid, the sum within 8192 + n_tables, and a single entry takes the lone grid."""
    assert _launches([]) == 0 and _launches([_rows()], n_tables=0) == 0
    assert _launches([_rows(rows=0)] * 7, want_blocks=True) == (2, [0] * 7)
    assert _launches([_rows()]) == 3 and _launches([_rows(), _ids()]) == 4
    rng = np.random.default_rng(5)
    scaled = 0
    for _ in range(60):
        entries, described = _random_entries(rng)
        got, blocks = _launches(entries, want_blocks=True)
        assert got == GD.launches(described) <= GD.MAX_LAUNCHES, described
        shapes = [(kind, dim, count) for _t, kind, dim, count, _b in described]
        assert blocks == GD.deal(shapes), described
        lone = [GD.lone_blocks(*s) for s in shapes]
        assert all((b >= 1) == (s[2] > 0) and b <= l for b, l, s in zip(blocks, lone, shapes))
        assert sum(blocks) <= GD.DEAL_BLOCKS + len(entries)
        scaled += sum(lone) > GD.DEAL_BLOCKS
        for e, l in zip(entries, lone):
            assert _launches([e], want_blocks=True) == (2 + (l > 0), [l])
    assert 5 <= scaled <= 55                                           # both branches of the deal were drawn
    # blocks is optional, and is left alone by a refused call
    assert _launches([_rows(), _rows(dim=0)], want_blocks=True) == (-INV, [-7, -7])
    assert "entry 1: " in _lib.load().fcp_last_error().decode()
    assert _launches([_rows()], n_tables=-1) == -INV


def test_launches_do_not_grow_with_the_number_of_entries():
    base = [_rows(kind=Q8, dim=64, rows=16384), _rows(kind=BF16, dim=16, rows=16384), _ids(kind=F16, dim=6, n=3), _rows(kind=F32, dim=7, rows=1),
            _ids(kind=Q8, dim=5, n=9), _rows(kind=Q8, dim=5, rows=9, table=A + 1)]
    one = _launches(base)
    assert one == 2 + 6
    assert _launches(base * 10) == one and _launches(base * 1000) == one
    got, blocks = _launches(base * 1000, want_blocks=True)
    assert sum(blocks) <= GD.DEAL_BLOCKS + 6000 and min(blocks) >= 1
    # the most entries: every one gets a block, and the sum stays inside the workspace's partial records
    got, blocks = _launches([_rows(kind=BF16, dim=1, rows=10 ** 6)] * 65536, want_blocks=True)
    assert got == 3 and set(blocks) == {1}


# ---- the Python wrappers -----------------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_what_they_can_see(monkeypatch):
    import torch
    from recom_amd import tables
    t, ids = torch.zeros((10, 8)), torch.arange(4)
    with pytest.raises(ValueError, match="entry 0: .*device to device"):              # host tensors
        tables.digests_grouped([t])
    with pytest.raises(ValueError, match="entry 0: .*device to device"):
        tables.digest_rows_grouped([t], [ids])
    with pytest.raises(ValueError, match="row_ids 1"):                                # sequences of different lengths
        tables.digest_rows_grouped([t, t], [ids])
    with pytest.raises(ValueError, match="row0 3"):
        tables.digests_grouped([t, t], row0=[0, 1, 2])
    with pytest.raises(ValueError, match="row_step 1"):
        tables.digests_grouped([t, t], row_step=(2,))
    with pytest.raises(ValueError, match="digests 1"):
        tables.update_rows_grouped_tracked([t, t], [ids, ids], [t, t], [0])
    with pytest.raises(ValueError, match="row_ids"):
        tables.digest_rows_grouped([t], None)
    assert tables.digests_grouped([]) == [] and tables.digest_rows_grouped([], []) == []
    assert tables.update_rows_grouped_tracked([], [], [], []) == []

    # behind the device check: the per-entry validation of digest_rows, with the wrapper's one device test looked past
    def kind_and_dim(t, what):
        names = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.uint8: "q8"}
        return names[t.dtype], int(t.shape[1]) - (8 if t.dtype == torch.uint8 else 0)
    monkeypatch.setattr(tables, "_kind_and_dim", kind_and_dim)
    monkeypatch.setattr(tables._lib, "load", lambda: pytest.fail("the library was reached"))
    q = torch.zeros((10, 16), dtype=torch.uint8)
    with pytest.raises(ValueError, match="entry 1: .*int64"):
        tables.digest_rows_grouped([t, q], [ids, ids.to(torch.int32)])
    with pytest.raises(ValueError, match="entry 1: .*int64"):
        tables.update_rows_grouped_tracked([t, q], [ids, ids.to(torch.int32)], [t, t], [0, 0])


# ---- code object -----------------------------------------------------------------------------------------------------------
def _asm(tmp, unit):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc) or shutil.which("hipcc"), "no hipcc"
    asm = tmp / (unit + ".s")
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                           os.path.join(CSRC, unit + ".hip"), "-o", str(asm)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return asm.read_text()


@pytest.fixture(scope="module")
def grouped_asm(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    return _asm(tmp, "fcp_tables_digest"), _asm(tmp, "fcp_table_digest")


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}


def _field(desc, name):
    return int(re.search(r"\.amdhsa_" + name + r" (\d+)", desc).group(1))


def _body(text, name):
    label = re.search(r"^" + re.escape(name) + r":", text, re.M)
    assert label, name
    return text[label.end():text.find(".amdhsa_kernel " + name)]


def test_code_object_of_the_grouped_kernels(grouped_asm):
    """56 digest kernels, one per class, and the fold.  No kernel has scratch; LDS is the block fold's four wave records (128
    bytes) and nothing in the fold kernel; integer code only; no atomic; every access a global or a scalar one.  The front stays on
    the scalar side: the first-block table and the record arrive by scalar loads, and in front of the first vector memory access
    there is no vector load.  Every kernel needs no more VGPRs than its single-table twin plus 4, and stays in the twin's
    occupancy step (64 / 72 / 80 / 96 registers: 8 / 7 / 6 / 5 waves per SIMD)."""
    grouped, single = grouped_asm
    kernels, twins = _kernels(grouped), _kernels(single)
    walk = {k for k in kernels if "fcp_tables_digest_kernel" in k}
    fold = {k for k in kernels if "fcp_tables_digest_fold_kernel" in k}
    assert len(walk) == 56 and len(fold) == 1 and len(kernels) == 57, sorted(kernels)
    steps = (64, 72, 80, 96, 128)
    for name, desc in sorted(kernels.items()):
        assert _field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        assert _field(desc, "group_segment_fixed_size") == (128 if name in walk else 0), f"{name}: LDS"
        body = _body(grouped, name)
        assert not re.search(r"\bscratch_|\bflat_|\bbuffer_", body), name
        assert not re.search(r"\b(global|ds|flat)_atomic|\bds_(add|cmpst|wrxchg)", body), f"{name}: an atomic"
        assert not re.search(r"\bv_(add|mul|fma|mac|mad|sub|div|rcp|cvt)[a-z_]*_f(16|32|64)\b", body), f"{name}: floating point"
        first_vmem = re.search(r"\bglobal_(load|store)", body)
        assert first_vmem, name
        if name in walk:
            front = body[:first_vmem.start()]
            assert re.search(r"\bs_load_dword\b", front), f"{name}: the search does not read the first-block table by scalar loads"
            assert len(re.findall(r"\bs_load_dwordx(4|8|16)\b", front)) >= 2, f"{name}: the record does not arrive by wide scalar loads"
            assert not re.search(r"\bv_readfirstlane_b32\b", front), f"{name}: the entry is found on the vector side"
            assert not re.search(r"\bs_waitcnt vmcnt", front), name
            m = re.search(r"fcp_tables_digest_kernelILi(\d+)ELi(\d+)ELb([01])EEE", name)
            (twin,) = [k for k in twins if f"fcp_table_digest_kernelILi{m.group(1)}ELi{m.group(2)}ELb{m.group(3)}EEE" in k]
            mine, theirs = _field(desc, "next_free_vgpr"), _field(twins[twin], "next_free_vgpr")
            print(name, "vgpr", mine, "twin", theirs)
            assert mine <= theirs + 4, (name, mine, theirs)
            assert next(s for s in steps if mine <= s) <= next(s for s in steps if theirs <= s), (name, mine, theirs)


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------
def test_the_plan_unit_alone_under_address_and_undefined_sanitizers(tmp_path):
    """recom_amd/csrc/fcp_tables_digest_plan.cc links without the GPU runtime, with nothing beside it but the host half of the
    single-table digest whose checks it takes (fcp_table_digest_host.cc); a stand-alone program
    (tests/native/tables_digest_plan_san.cc), all built with -fsanitize=address,undefined, drives the builder over random entry
    lists and the refusals, and prints `0 failures` with no sanitizer report.  Nothing is loaded into python."""
    assert shutil.which("g++") is not None, "no g++"
    exe = str(tmp_path / "tables_digest_plan_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "native", "tables_digest_plan_san.cc"), os.path.join(CSRC, "fcp_tables_digest_plan.cc"),
                            os.path.join(CSRC, "fcp_table_digest_host.cc"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "20261021", "400"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-2:] == ["400 sets", "0 failures"], run.stdout[-2000:]
