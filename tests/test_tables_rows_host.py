"""fcp_tables_update_rows / fcp_tables_read_rows / fcp_tables_rows_launches without a GPU: the C ABI's surface, the workspace
formula, the status order with its `entry k` messages, the launch count — the point of the feature: it does not grow with the
number of entries — the Python wrappers' refusals, the code object of recom_amd/csrc/fcp_tables_rows.hip, and the host-only
launch-list builder (recom_amd/csrc/fcp_tables_rows_plan.cc) alone under the sanitizers.  (The kernels themselves:
tests/test_zzz_gpu_tables_rows.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import table_convert_cases as TC
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
CSRC = os.path.join(ROOT, "recom_amd", "csrc")
F32, BF16, F16, Q8 = (TC.KINDS[k] for k in ("f32", "bf16", "f16", "q8"))
A = 1 << 20                                                   # an address aligned for everything
NAMES = ("fcp_tables_rows_workspace_bytes", "fcp_tables_rows_launches", "fcp_tables_update_rows", "fcp_tables_read_rows")
INV, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK


def _entry(kind=Q8, dim=64, n=5, table_rows=100, table=A, ids=A, rows=A, reserved=(0, 0)):
    return _lib.TableRows(table, ids, rows, table_rows, n, kind, dim, (C.c_int64 * 2)(*reserved))


def _array(entries):
    return (_lib.TableRows * max(len(entries), 1))(*entries)


def _update(entries, n_tables=None, skipped=0, workspace=A, device=0):
    L = _lib.load()
    status = L.fcp_tables_update_rows(_array(entries) if entries is not None else None, len(entries) if n_tables is None else n_tables,
                                      C.c_void_p(skipped), C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def _read(entries, n_tables=None, skipped=0, workspace=A, device=0):
    assert skipped == 0
    L = _lib.load()
    status = L.fcp_tables_read_rows(_array(entries) if entries is not None else None, len(entries) if n_tables is None else n_tables,
                                    C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def _launches(entries, n_tables=None):
    return int(_lib.load().fcp_tables_rows_launches(_array(entries), len(entries) if n_tables is None else n_tables))


ENTRIES = {"fcp_tables_update_rows": _update, "fcp_tables_read_rows": _read}


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert "int64_t fcp_tables_rows_workspace_bytes(int32_t n_tables);" in text
    assert "int32_t fcp_tables_rows_launches(const fcp_table_rows_t *entries, int32_t n_tables);" in text
    assert ("int fcp_tables_update_rows(const fcp_table_rows_t *entries, int32_t n_tables, int64_t *skipped /* device [n_tables] or NULL */, "
            "void *workspace, int32_t device, void *stream);") in text
    assert "int fcp_tables_read_rows(const fcp_table_rows_t *entries, int32_t n_tables, void *workspace, int32_t device, void *stream);" in text
    assert "} fcp_table_rows_t;" in text
    assert set(NAMES) <= set(_lib.EXPORTS)
    L = _lib.load()
    for name in NAMES:
        assert hasattr(L, name), name
    # behind the rows-by-id section, and the ABI is append-only
    assert text.index("int fcp_table_read_rows(") < text.index("typedef struct fcp_table_rows {") < text.index("int fcp_table_delta_distinct(")
    assert re.search(r"#define FCP_ABI_VERSION 2\b", text) and _lib.FCP_ABI_VERSION == 2 and L.fcp_abi_version() == 2


def test_the_entry_struct_is_64_bytes_in_c_and_in_python(tmp_path):
    assert C.sizeof(_lib.TableRows) == 64
    offsets = {f: getattr(_lib.TableRows, f).offset for f, _t in _lib.TableRows._fields_}
    assert offsets == {"table": 0, "row_ids": 8, "rows": 16, "table_rows": 24, "n": 32, "kind": 40, "dim": 44, "reserved": 48}
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fcp_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(fcp_table_rows_t), offsetof(fcp_table_rows_t, n), offsetof(fcp_table_rows_t, dim), '
                   'offsetof(fcp_table_rows_t, reserved)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["64", "32", "44", "48"]


def test_workspace_formula():
    """A function of n_tables alone: -1 outside [0, 65536], a multiple of 8, non-decreasing, and room for one 64-byte record and
    one first-block value per entry."""
    ws = _lib.load().fcp_tables_rows_workspace_bytes
    assert ws(-1) == -1 and ws(65537) == -1 and ws(-2 ** 31) == -1 and ws(2 ** 31 - 1) == -1
    sizes = [int(ws(n)) for n in range(0, 65537)]
    assert all(s > 0 and s % 8 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert all(s >= 16 + 68 * n for n, s in enumerate(sizes))
    assert sizes[65536] < 8 << 20


# ---- status order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_status_codes_arrive_in_the_stated_order(entry):
    """n_tables; `entries`; the entries in ascending order, each by the single-table entry's own order, then `reserved`;
    `workspace`; `skipped`.  Then FCP_OK for no work, without a device; then, on a machine without a GPU, FCP_ERR_NO_DEVICE.
    (Pointers are never dereferenced on the host: plain numbers serve.)"""
    import torch
    no_gpu = not torch.cuda.is_available()
    call = ENTRIES[entry]
    good = _entry()
    for n_tables in (-1, 65537, -2 ** 31, 2 ** 31 - 1):
        status, msg = call([good], n_tables=n_tables)
        assert status == INV and "`n_tables`" in msg and msg.startswith(entry + ":"), (n_tables, status, msg)
    status, msg = call(None, n_tables=3)
    assert status == INV and "`entries`" in msg, msg
    # n_tables comes before entries
    assert "`n_tables`" in call(None, n_tables=-5)[1]
    # per entry, the single-table entry's checks, named, with `entry k`
    for bad, word in ((_entry(n=-1), "n"), (_entry(n=2 ** 32 - 3), "n"), (_entry(table_rows=0), "table_rows"),
                      (_entry(table_rows=2 ** 32 - 3), "table_rows"), (_entry(dim=0), "dim"), (_entry(kind=F32, dim=-3), "dim"),
                      (_entry(kind=4), "kind"), (_entry(kind=-1), "kind"), (_entry(table=0), "table"), (_entry(kind=BF16, ids=0), "row_ids"),
                      (_entry(kind=F16, rows=0), "rows"), (_entry(dim=63, table=A + 2), "table"), (_entry(ids=A + 4), "row_ids"),
                      (_entry(rows=A + 8), "rows"), (_entry(reserved=(1, 0)), "reserved"), (_entry(reserved=(0, -1)), "reserved"),
                      (_entry(n=0, reserved=(0, 7)), "reserved")):
        for k in (0, 1, 4):
            entries = [good] * k + [bad] + [good] * 2
            status, msg = call(entries)
            assert status == INV and msg.startswith(f"{entry}: entry {k}: ") and f"`{word}`" in msg, (word, k, status, msg)
    # inside an entry the order is n, table_rows, dim, kind, null pointers, alignment, reserved
    for bad, word in ((_entry(kind=9, dim=0, table_rows=0, n=-1, table=0, ids=0, rows=0, reserved=(1, 1)), "n"),
                      (_entry(kind=9, dim=0, table_rows=0, table=0, ids=0, rows=0, reserved=(1, 1)), "table_rows"),
                      (_entry(kind=9, dim=0, table=0, ids=0, rows=0, reserved=(1, 1)), "dim"),
                      (_entry(kind=9, table=0, ids=0, rows=0, reserved=(1, 1)), "kind"),
                      (_entry(table=0, ids=0, rows=0, reserved=(1, 1)), "table"),
                      (_entry(table=A + 1, ids=0, rows=0, reserved=(1, 1)), "row_ids"),
                      (_entry(table=A + 1, ids=A + 1, rows=0, reserved=(1, 1)), "rows"),
                      (_entry(table=A + 1, ids=A + 1, rows=A + 1, reserved=(1, 1)), "table"),
                      (_entry(ids=A + 1, rows=A + 1, reserved=(1, 1)), "rows"),
                      (_entry(ids=A + 1, reserved=(1, 1)), "row_ids"),
                      (_entry(reserved=(1, 1)), "reserved")):
        status, msg = call([bad], workspace=0)
        assert status == INV and "entry 0: " in msg and f"`{word}`" in msg, (word, status, msg)
    # the first bad entry wins; an entry wins over the workspace and over skipped
    status, msg = call([good, _entry(dim=0), _entry(n=-1)], workspace=A + 4)
    assert status == INV and "entry 1: " in msg and "`dim`" in msg, msg
    # the workspace: null with entries, misaligned; then skipped
    status, msg = call([good], workspace=0)
    assert status == INV and "`workspace`" in msg and "entry" not in msg, msg
    status, msg = call([good], workspace=A + 4)
    assert status == INV and "`workspace`" in msg, msg
    assert call([_entry(n=0)], workspace=0)[0] == INV                   # an invalid argument wins over "nothing to do"
    if entry == "fcp_tables_update_rows":
        status, msg = call([good], skipped=A + 4, workspace=A + 4)
        assert status == INV and "`workspace`" in msg, msg
        status, msg = call([good], skipped=A + 4)
        assert status == INV and "`skipped`" in msg, msg
        assert call([_entry(n=0)], skipped=A + 4)[0] == INV
    # nothing to do: FCP_OK with no device, null pointers inside empty entries included
    assert call([], workspace=0, device=12345)[0] == OK
    assert call(None, n_tables=0, workspace=0, device=12345)[0] == OK
    empty = [_entry(kind=k, dim=d, n=0, table=0, ids=0, rows=0) for k in (F32, BF16, F16, Q8) for d in (64, 7)]
    assert call(empty, device=12345)[0] == OK
    assert call([_entry(n=0)] * 65536, device=12345)[0] == OK          # the last n_tables
    if entry == "fcp_tables_update_rows":
        assert call(empty, skipped=A + 8, device=12345)[0] == OK
    # work: no device here; no valid combination is unsupported without a capturing stream
    if no_gpu:
        for kind in (F32, BF16, F16, Q8):
            for dim in (64, 62, 61):
                assert call([_entry(kind=kind, dim=dim)])[0] == NODEV
        assert call(empty + [good] + empty)[0] == NODEV
        assert call([_entry(n=2 ** 32 - 4, table_rows=2 ** 32 - 4)])[0] == NODEV      # the last values below both limits
        if entry == "fcp_tables_update_rows":
            assert call([good, good], skipped=A + 8)[0] == NODEV


def test_a_call_names_at_most_2_to_the_40_elements():
    """The one limit of the grouped entries that a single-table call has not: n * dim summed over the entries stays within 2^40
    (4 TiB of float32 rows), which is what lets the workspace depend on n_tables alone."""
    big = _entry(kind=F32, dim=256, n=2 ** 31)                       # 2^39 elements
    assert _launches([big, big, _entry(n=0)]) == 1 + 2 * 128            # 2^40 itself passes (host only: nothing is launched)
    for call in ENTRIES.values():
        status, msg = call([big, big, _entry(kind=F32, dim=1, n=1)])
        assert status == INV and "`entries`" in msg and "2^40" in msg, msg
    assert _launches([big, big, _entry(kind=F32, dim=1, n=1)]) == -INV


# ---- the launch count --------------------------------------------------------------------------------------------------------
def _class_of(kind, dim):
    """A q8 update's class is its (V, G); everything else is classed by V alone."""
    return (TC.vec_of(dim), TC.group_of(dim)) if kind == Q8 else (TC.vec_of(dim), 0)


def test_launches_is_one_upload_plus_one_launch_per_class():
    assert _launches([]) == 0 and _launches([_entry()], n_tables=0) == 0
    assert _launches([_entry(n=0)] * 7) == 0
    assert _launches([_entry()]) == 2
    rng = np.random.default_rng(3)
    for _ in range(40):
        entries, classes = [], set()
        for _k in range(int(rng.integers(1, 60))):
            kind, dim, n = int(rng.integers(0, 4)), int(rng.choice(TC.QUANT_DIMS)), int(rng.choice((0, 0, 1, 63, 64, 65, 257, 100000)))
            entries.append(_entry(kind=kind, dim=dim, n=n))
            if n:
                classes.add(_class_of(kind, dim))
        assert _launches(entries) == (1 + len(classes) if classes else 0), [(e.kind, e.dim, e.n) for e in entries]
    # empty entries take no part, wherever they stand
    mixed = [_entry(kind=Q8, dim=64), _entry(kind=BF16, dim=64), _entry(kind=F32, dim=6), _entry(kind=Q8, dim=3)]
    assert _launches(mixed) == 5                                       # q8 (4, 16), streaming V 4, streaming V 2, q8 (1, 1)
    assert _launches([_entry(n=0)] + mixed[:2] + [_entry(n=0, dim=5)] * 2 + mixed[2:] + [_entry(n=0)]) == 5
    # invalid arguments: the negative of the status, and the message names the entry
    assert _launches([_entry()], n_tables=-1) == -INV and _launches([_entry(), _entry(dim=0)]) == -INV
    assert "entry 1: " in _lib.load().fcp_last_error().decode()


def test_launches_do_not_grow_with_the_number_of_entries():
    """The same entries repeated 1, 10 and 1000 times enqueue the same launches; an update of every format at every dim of
    TC.QUANT_DIMS — every class there is — stays at 25 or below."""
    base = [_entry(kind=kind, dim=dim, n=n) for kind, dim, n in ((Q8, 64, 1024), (Q8, 16, 16), (BF16, 16, 1024), (F16, 6, 3), (F32, 7, 1), (Q8, 5, 9))]
    one = _launches(base)
    assert one == 1 + len({_class_of(e.kind, e.dim) for e in base}) == 7
    assert _launches(base * 10) == one and _launches(base * 1000) == one
    every = [_entry(kind=kind, dim=dim, n=1 + dim % 5) for dim in TC.QUANT_DIMS for kind in (F32, BF16, F16, Q8)]
    assert len({_class_of(e.kind, e.dim) for e in every}) <= 24
    assert _launches(every) == 1 + len({_class_of(e.kind, e.dim) for e in every}) <= 25
    assert _launches(every * 100) == _launches(every)
    rng = np.random.default_rng(11)
    for _ in range(20):
        picks = [every[i] for i in rng.integers(0, len(every), int(rng.integers(1, 400)))]
        assert 2 <= _launches(picks) <= 25
    # every (V, G) a dim can have — 18 of the 21: a dim above 4 has at least three slots of V 2 or five of V 1, so (2, 2), (1, 2)
    # and (1, 4) have no dim — and all 3 V: the most launches an unsplit update can take
    dims = {}
    for dim in list(TC.QUANT_DIMS) + list(range(1, 300)):
        dims.setdefault(_class_of(Q8, dim), dim)
    assert len(dims) == 18 and not {(2, 2), (1, 2), (1, 4)} & set(dims)
    full = [_entry(kind=Q8, dim=d) for d in dims.values()] + [_entry(kind=F32, dim=d) for d in (4, 2, 1)]
    assert _launches(full) == 22 and _launches(full * 50) == 22


def test_a_class_of_more_than_2_to_the_30_threads_splits_as_the_single_table_host_does():
    """2^26 + 1 q8 rows of dim 64 (G 16): 2^30 + 16 threads, two launches where fcp_table_update_rows enqueues two; small entries
    of the class ride along.  A streaming entry of 2^32 slots: four launches of 2^30 threads."""
    assert _launches([_entry(kind=Q8, dim=64, n=2 ** 26)]) == 2
    assert _launches([_entry(kind=Q8, dim=64, n=2 ** 26 + 1)]) == 3
    # (a small entry in front: a launch of its own, the full piece does not fit behind it; the one behind joins the tail)
    assert _launches([_entry(kind=Q8, dim=64, n=7), _entry(kind=Q8, dim=64, n=2 ** 26 + 1), _entry(kind=Q8, dim=64, n=9)]) == 4
    assert _launches([_entry(kind=BF16, dim=64, n=2 ** 28)]) == 1 + 4
    assert _launches([_entry(kind=BF16, dim=64, n=2 ** 28), _entry(kind=F32, dim=4, n=3)]) == 1 + 5


# ---- the Python wrappers -----------------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_what_they_can_see(monkeypatch):
    import torch
    from recom_amd import tables
    t, ids, rows = torch.zeros((10, 8)), torch.arange(4), torch.zeros((4, 8))
    with pytest.raises(ValueError, match="entry 0: .*device to device"):              # host tensors
        tables.update_rows_grouped([t], [ids], [rows])
    with pytest.raises(ValueError, match="entry 0: .*device to device"):
        tables.read_rows_grouped([t], [ids])
    with pytest.raises(ValueError, match="row_ids 1"):                                # sequences of different lengths
        tables.update_rows_grouped([t, t], [ids], [rows, rows])
    with pytest.raises(ValueError, match="rows 1"):
        tables.update_rows_grouped([t, t], [ids, ids], [rows])
    with pytest.raises(ValueError, match="row_ids 0"):
        tables.read_rows_grouped([t], [])
    assert tables.update_rows_grouped([], [], []) == [] and tables.read_rows_grouped([], []) == []

    # behind the device check: the per-entry validation of update_rows / read_rows, with the wrapper's one device test looked past
    def kind_and_dim(t, what):
        names = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.uint8: "q8"}
        return names[t.dtype], int(t.shape[1]) - (8 if t.dtype == torch.uint8 else 0)
    monkeypatch.setattr(tables, "_kind_and_dim", kind_and_dim)
    monkeypatch.setattr(tables._lib, "load", lambda: pytest.fail("the library was reached"))
    q = torch.zeros((10, 16), dtype=torch.uint8)
    with pytest.raises(ValueError, match="entry 1: .*int64"):
        tables.update_rows_grouped([t, q], [ids, ids.to(torch.int32)], [rows, rows])
    with pytest.raises(ValueError, match="entry 1: .*float32"):
        tables.update_rows_grouped([t, q], [ids, ids], [rows, rows.half()])
    with pytest.raises(ValueError, match="entry 0: .*row_ids names 4"):
        tables.update_rows_grouped([t, q], [ids, ids], [torch.zeros((5, 8)), rows])
    with pytest.raises(ValueError, match="entry 1: .*of dim 7"):
        tables.update_rows_grouped([t, q], [ids, ids], [rows, torch.zeros((4, 7))])
    with pytest.raises(ValueError, match="entry 1: .*row_ids names 4"):
        tables.read_rows_grouped([t, q], [ids, ids], out=[rows, torch.zeros((3, 8))])
    with pytest.raises(ValueError, match="skipped"):
        tables.update_rows_grouped([t, q], [ids, ids], [rows, rows], skipped=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="skipped"):
        tables.update_rows_grouped([t, q], [ids, ids], [rows, rows], skipped=torch.zeros(2, dtype=torch.int32))


# ---- code object -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grouped_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("asm") / "fcp_tables_rows.s"
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                           os.path.join(CSRC, "fcp_tables_rows.hip"), "-o", str(asm)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return asm.read_text()


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}


def _field(desc, name):
    return int(re.search(r"\.amdhsa_" + name + r" (\d+)", desc).group(1))


def _body(text, name):
    label = re.search(r"^" + re.escape(name) + r":", text, re.M)
    assert label, name
    return text[label.end():text.find(".amdhsa_kernel " + name)]


def test_code_object_of_the_grouped_kernels(grouped_asm):
    """21 q8 updaters, three streaming updaters, three readers.  No kernel has scratch or LDS; the modes are the other units'.
    The front stays on the scalar side: the first-block table and the record arrive by scalar loads (one dword per search step,
    the 64-byte record as wide loads), and in front of the first vector memory access there is no vector load at all.  The
    bodies are the single-table kernels': one vector atomic add per updater, none per reader, the quantiser's two correctly
    rounded divisions, nothing contracted, every access a global one."""
    kernels = _kernels(grouped_asm)
    quant = {k for k in kernels if "fcp_tables_update_q8_kernel" in k}
    stream = {k for k in kernels if "fcp_tables_update_rows_kernel" in k}
    read = {k for k in kernels if "fcp_tables_read_rows_kernel" in k}
    assert len(quant) == 21 and len(stream) == 3 and len(read) == 3 and len(kernels) == 27, sorted(kernels)
    for name, desc in sorted(kernels.items()):
        assert _field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        assert _field(desc, "group_segment_fixed_size") == 0, f"{name}: uses LDS"
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc) and re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", desc), name
        assert re.search(r"\.amdhsa_ieee_mode 1\b", desc), f"{name}: not in IEEE mode"
        assert _field(desc, "next_free_vgpr") <= 64, name
        body = _body(grouped_asm, name)
        assert not re.search(r"\b(scratch_|ds_read|ds_write|ds_load|ds_store)", body), name
        assert not re.search(r"\bflat_", body), name
        assert len(re.findall(r"\bglobal_atomic_add_x2\b", body)) == (0 if name in read else 1), name
        # the front: scalar loads only, and a search loop whose one load is a scalar dword
        first_vmem = re.search(r"\bglobal_(load|store|atomic)", body)
        assert first_vmem, name
        front = body[:first_vmem.start()]
        assert re.search(r"\bs_load_dword\b", front), f"{name}: the search does not read the first-block table by scalar loads"
        assert len(re.findall(r"\bs_load_dwordx(4|8|16)\b", front)) >= 2, f"{name}: the record does not arrive by wide scalar loads"
        assert not re.search(r"\bv_readfirstlane_b32\b", front), f"{name}: the entry is found on the vector side"
        assert not re.search(r"\bs_waitcnt vmcnt", front), name
    for name in quant:
        body = _body(grouped_asm, name)
        assert len(re.findall(r"\bv_div_fixup_f32\b", body)) == 2 and len(re.findall(r"\bv_div_fmas_f32\b", body)) == 2, name
        assert not re.search(r"\bv_pk_fma_f32|\bv_mac_f32|\bv_mad_f32", body), name
        assert len(re.findall(r"\bv_fma_f32|\bv_fmac_f32", body)) == 5 * 2, name
    for v in (1, 2, 4):
        (rd,) = [k for k in read if f"fcp_tables_read_rows_kernelILi{v}EE" in k]
        assert len(re.findall(r"\bv_fma_f32\b", _body(grouped_asm, rd))) == v, rd           # q8: one fma per element


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------
def test_the_launch_list_builder_alone_under_address_and_undefined_sanitizers(tmp_path):
    """recom_amd/csrc/fcp_tables_rows_plan.cc links without the GPU runtime and without any other unit; a stand-alone program
    (tests/native/tables_rows_plan_san.cc), both built with -fsanitize=address,undefined, drives the builder over random entry
    sets and the refusals, and prints `0 failures` with no sanitizer report.  Nothing is loaded into python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "tables_rows_plan_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "native", "tables_rows_plan_san.cc"), os.path.join(CSRC, "fcp_tables_rows_plan.cc"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        pytest.skip("libasan / libubsan not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "20261020", "400"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-2:] == ["400 sets", "0 failures"], run.stdout[-2000:]


def test_the_shared_grouped_plan_header_alone_under_address_and_undefined_sanitizers(tmp_path):
    """recom_amd/csrc/fcp_grouped_plan.h — the class sort, the launch-list builder and the refusals that the grouped rows and the
    grouped digest entries share — needs no unit of the library; a stand-alone program (tests/native/grouped_plan_san.cc) built
    with -fsanitize=address,undefined drives the sort against std::stable_sort, the builder with and without a block cap,
    log2_of and the refusals' whole texts, and prints `0 failures` with no sanitizer report.  Nothing is loaded into python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "grouped_plan_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "native", "grouped_plan_san.cc"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        pytest.skip("libasan / libubsan not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "20261021", "600"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-2:] == ["600 sets", "0 failures"], run.stdout[-2000:]
