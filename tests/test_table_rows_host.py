"""fcp_table_update_rows / fcp_table_read_rows without a GPU: the C ABI's surface, the status order and the alignment rule, the
Python wrapper's refusals, and the code object of recom_amd/csrc/fcp_table_rows.hip.  (The kernels themselves:
tests/test_gpu_table_rows.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import table_convert_cases as TC
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
F32, BF16, F16, Q8 = (TC.KINDS[k] for k in ("f32", "bf16", "f16", "q8"))
A = 1 << 20                                                   # an address aligned for everything


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entries():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int fcp_table_update_rows(void *table, int32_t kind, int64_t table_rows, int32_t dim, const int64_t *row_ids, "
            "const float *rows, int64_t n, int64_t *skipped, int32_t device, void *stream);") in text
    assert ("int fcp_table_read_rows(float *rows, const void *table, int32_t kind, int64_t table_rows, int32_t dim, "
            "const int64_t *row_ids, int64_t n, int32_t device, void *stream);") in text
    assert "pairwise distinct" in text and "SKIPPED" in text
    assert {"fcp_table_update_rows", "fcp_table_read_rows"} <= set(_lib.EXPORTS)
    L = _lib.load()
    assert hasattr(L, "fcp_table_update_rows") and hasattr(L, "fcp_table_read_rows")
    assert re.search(r"#define FCP_ABI_VERSION 2\b", text) and _lib.FCP_ABI_VERSION == 2 and L.fcp_abi_version() == 2


def _update(table, kind, table_rows, dim, ids, rows, n, skipped=0, device=0):
    L = _lib.load()
    status = L.fcp_table_update_rows(C.c_void_p(table), kind, table_rows, dim, C.c_void_p(ids), C.c_void_p(rows), n,
                                     C.c_void_p(skipped), device, None)
    return status, L.fcp_last_error().decode()


def _read(table, kind, table_rows, dim, ids, rows, n, skipped=0, device=0):
    assert skipped == 0
    L = _lib.load()
    status = L.fcp_table_read_rows(C.c_void_p(rows), C.c_void_p(table), kind, table_rows, dim, C.c_void_p(ids), n, device, None)
    return status, L.fcp_last_error().decode()


ENTRIES = {"fcp_table_update_rows": _update, "fcp_table_read_rows": _read}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_status_codes_arrive_in_the_stated_order(entry):
    """No GPU here: valid arguments end in FCP_ERR_NO_DEVICE — after every argument check and after the FCP_OK of n == 0.
    (Pointers are never dereferenced on the host: plain numbers serve.)  The message names the entry and, between
    backquotes, the argument."""
    import torch
    no_gpu = not torch.cuda.is_available()      # (with a GPU valid arguments would run: only the device-free statuses are checked)
    INV, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK
    call = ENTRIES[entry]
    # 1. invalid arguments, each named: (table, kind, table_rows, dim, row_ids, rows, n)
    for args, word in (((A, Q8, 100, 64, A, A, -1), "n"), ((A, Q8, 100, 64, A, A, 2 ** 32 - 3), "n"),
                       ((A, Q8, 0, 64, A, A, 5), "table_rows"), ((A, Q8, -7, 64, A, A, 5), "table_rows"),
                       ((A, Q8, 2 ** 32 - 3, 64, A, A, 5), "table_rows"),
                       ((A, Q8, 100, 0, A, A, 5), "dim"), ((A, F32, 100, -3, A, A, 5), "dim"),
                       ((A, 4, 100, 64, A, A, 5), "kind"), ((A, -1, 100, 64, A, A, 5), "kind"),
                       ((0, Q8, 100, 64, A, A, 5), "table"), ((A, BF16, 100, 64, 0, A, 5), "row_ids"),
                       ((A, F16, 100, 64, A, 0, 5), "rows"),
                       ((A + 2, Q8, 100, 63, A, A, 5), "table"), ((A, Q8, 100, 64, A + 4, A, 5), "row_ids"),
                       ((A, Q8, 100, 64, A, A + 8, 5), "rows")):
        status, msg = call(*args)
        assert status == INV and f"`{word}`" in msg and msg.startswith(entry + ":"), (args, status, msg)
    if entry == "fcp_table_update_rows":
        status, msg = call(A, Q8, 100, 64, A, A, 5, skipped=A + 4)
        assert status == INV and "`skipped`" in msg, (status, msg)
    # the checks come in the stated order: n, table_rows, dim, kind, null pointers, alignment
    for args, word in (((0, 9, 0, 0, 0, 0, -1), "n"), ((0, 9, 0, 0, 0, 0, 5), "table_rows"), ((0, 9, 100, 0, 0, 0, 5), "dim"),
                       ((0, 9, 100, 64, 0, 0, 5), "kind"), ((0, Q8, 100, 64, 0, 0, 5), "table"),
                       ((A + 1, Q8, 100, 64, 0, 0, 5), "row_ids"), ((A + 1, Q8, 100, 64, A + 1, 0, 5), "rows"),
                       ((A + 1, Q8, 100, 64, A + 1, A + 1, 5), "table"), ((A, Q8, 100, 64, A + 1, A + 1, 5), "rows"),
                       ((A, Q8, 100, 64, A + 1, A, 5), "row_ids")):
        status, msg = call(*args)
        assert status == INV and f"`{word}`" in msg, (args, status, msg)
    # 2. an invalid argument wins over n == 0
    assert call(A, Q8, 0, 64, A, A, 0)[0] == INV
    assert call(A, 7, 100, 64, A, A, 0)[0] == INV
    assert call(A + 1, Q8, 100, 64, A, A, 0)[0] == INV
    assert call(A, Q8, 100, 0, 0, 0, 0)[0] == INV
    # 3. n == 0: FCP_OK with no launch and no device, null pointers included
    for kind in (F32, BF16, F16, Q8):
        assert call(A, kind, 100, 64, A, A, 0)[0] == OK
        assert call(0, kind, 1, 7, 0, 0, 0)[0] == OK
        assert call(0, kind, 2 ** 32 - 4, 7, 0, 0, 0, device=12345)[0] == OK
    # 4. everything valid: no device; there is no unsupported combination
    if no_gpu:
        for kind in (F32, BF16, F16, Q8):
            for dim in (64, 62, 61):
                assert call(A, kind, 100, dim, A, A, 5)[0] == NODEV
            assert call(A, kind, 2 ** 32 - 4, 64, A, A, 2 ** 32 - 4)[0] == NODEV          # the last values below both limits
        if entry == "fcp_table_update_rows":
            assert call(A, Q8, 100, 64, A, A, 5, skipped=A + 8)[0] == NODEV


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_alignment_rule_per_kind_and_vector_width(entry):
    """`table`: 4 * V bytes for float32, 2 * V for the 16-bit kinds, 4 for q8 whatever the dim; `rows`: 4 * V; V the largest
    of 4 | 2 | 1 that divides dim.  One step short of each edge is refused and names the argument; the edge itself passes
    (n == 0: past every argument check without a device)."""
    INV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_OK
    call = ENTRIES[entry]
    for dim, v in ((64, 4), (62, 2), (61, 1)):
        assert TC.vec_of(dim) == v
        for kind, need in ((F32, 4 * v), (BF16, 2 * v), (F16, 2 * v), (Q8, 4)):
            assert call(A + need, kind, 100, dim, A, A, 0)[0] == OK, (dim, kind)
            assert call(A + 3 * need, kind, 100, dim, A, A, 0)[0] == OK, (dim, kind)
            if need > 1:
                status, msg = call(A + need // 2, kind, 100, dim, A, A, 0)
                assert status == INV and "`table`" in msg and f"{need}-byte" in msg, (dim, kind, msg)
                assert call(A + need - 1, kind, 100, dim, A, A, 0)[0] == INV, (dim, kind)
        assert call(A, Q8, 100, dim, A, A + 4 * v, 0)[0] == OK
        status, msg = call(A, Q8, 100, dim, A, A + 2 * v, 0)
        assert status == INV and "`rows`" in msg and f"{4 * v}-byte" in msg, (dim, msg)
    assert call(A, Q8, 100, 64, A + 8, A, 0)[0] == OK
    assert call(A, Q8, 100, 64, A + 4, A, 0)[0] == INV
    if entry == "fcp_table_update_rows":
        assert call(A, Q8, 100, 64, A, A, 0, skipped=A + 8)[0] == OK
        assert call(A, Q8, 100, 64, A, A, 0, skipped=A + 4)[0] == INV


def test_python_wrapper_refuses_what_it_can_see():
    import torch
    from recom_amd import tables
    t = torch.zeros((10, 8))
    ids = torch.arange(4)
    rows = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="device to device"):                  # a host tensor
        tables.update_rows(t, ids, rows)
    with pytest.raises(ValueError, match="device to device"):
        tables.read_rows(t, ids)
    with pytest.raises(ValueError, match="no table format"):                   # a dtype that is no table format
        tables.update_rows(t.double(), ids, rows)
    with pytest.raises(ValueError, match="no table format"):
        tables.read_rows(t.to(torch.int32), ids)
    with pytest.raises(ValueError, match="unknown table dtype"):               # (and the unknown name stays unknown)
        tables.row_bytes("q4", 8)
    with pytest.raises(ValueError, match="float32"):
        tables.update_from_host(t, ids, rows.half())
    with pytest.raises(ValueError, match="int64"):
        tables.update_from_host(t, ids.to(torch.int32), rows)
    with pytest.raises(ValueError, match="chunk_rows"):
        tables.update_from_host(t, ids, rows, chunk_rows=0)
    with pytest.raises(ValueError, match="device to device"):
        tables.update_from_host(t, ids, rows)


def test_python_wrapper_refuses_mismatched_ids_and_rows(monkeypatch):
    """What lies behind the device check — the dtype of ids and rows, an ids / rows length mismatch, a dim mismatch — on
    host tensors, with the wrapper's one device test looked past (the library is never reached: every case is refused
    first)."""
    import torch
    from recom_amd import tables

    def kind_and_dim(t, what):
        names = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.uint8: "q8"}
        return names[t.dtype], int(t.shape[1]) - (8 if t.dtype == torch.uint8 else 0)
    monkeypatch.setattr(tables, "_kind_and_dim", kind_and_dim)
    monkeypatch.setattr(tables._lib, "load", lambda: pytest.fail("the library was reached"))
    ids = torch.arange(4)
    for t in (torch.zeros((10, 8)), torch.zeros((10, 16), dtype=torch.uint8), torch.zeros((10, 8), dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="int64"):
            tables.update_rows(t, ids.to(torch.int32), torch.zeros((4, 8)))
        with pytest.raises(ValueError, match="int64"):
            tables.read_rows(t, ids.reshape(2, 2))
        with pytest.raises(ValueError, match="float32"):
            tables.update_rows(t, ids, torch.zeros((4, 8), dtype=torch.float16))
        with pytest.raises(ValueError, match="row_ids names 4"):
            tables.update_rows(t, ids, torch.zeros((5, 8)))
        with pytest.raises(ValueError, match="row_ids names 4"):
            tables.read_rows(t, ids, out=torch.zeros((3, 8)))
        with pytest.raises(ValueError, match="of dim 7"):
            tables.update_rows(t, ids, torch.zeros((4, 7)))
        with pytest.raises(ValueError, match="of dim 16"):
            tables.read_rows(t, ids, out=torch.zeros((4, 16)))
        with pytest.raises(ValueError, match="skipped"):
            tables.update_rows(t, ids, torch.zeros((4, 8)), skipped=torch.zeros(1, dtype=torch.int32))
        with pytest.raises(ValueError, match="names 4"):
            tables.update_from_host(t, ids, torch.zeros((5, 8)))
        with pytest.raises(ValueError, match="of dim 9"):
            tables.update_from_host(t, ids, torch.zeros((4, 9)))


# ---- code object -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("asm") / "fcp_table_rows.s"
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                           os.path.join(ROOT, "recom_amd", "csrc", "fcp_table_rows.hip"), "-o", str(asm)],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
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


def test_code_object_of_the_row_kernels(rows_asm):
    """fcp_table_rows.hip compiles for gfx950: 21 q8 updaters (3 V x 7 G), three streaming updaters and three readers; no
    kernel has scratch or LDS; denormals are kept and IEEE mode is on.  The q8 updaters carry what
    tests/test_table_convert_host.py asserts of the quantisers: the two correctly rounded divisions, rint as the hardware's
    round-to-nearest-even, nothing contracted, the butterflies, loads of V floats and code stores of V bytes.  Every
    updater counts skipped rows with exactly one vector atomic add in its body (executed at most once per wave); the
    readers have none."""
    kernels = _kernels(rows_asm)
    quant = {k for k in kernels if "fcp_update_q8_kernel" in k}
    stream = {k for k in kernels if "fcp_update_rows_kernel" in k}
    read = {k for k in kernels if "fcp_read_rows_kernel" in k}
    assert len(quant) == 21 and len(stream) == 3 and len(read) == 3 and len(kernels) == 27, sorted(kernels)
    for name, desc in sorted(kernels.items()):
        assert _field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        assert _field(desc, "group_segment_fixed_size") == 0, f"{name}: uses LDS"
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc), f"{name}: fp32 subnormals are flushed"
        assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", desc), f"{name}: fp16 subnormals are flushed"
        assert re.search(r"\.amdhsa_ieee_mode 1\b", desc), f"{name}: not in IEEE mode"
        assert _field(desc, "next_free_vgpr") <= 64, name                     # 8 waves per SIMD: the kernels wait on memory
        body = _body(rows_asm, name)
        assert not re.search(r"\b(scratch_|ds_read|ds_write|ds_load|ds_store)", body), name
        assert len(re.findall(r"\bglobal_atomic_add_x2\b", body)) == (0 if name in read else 1), name
        assert not re.search(r"\bflat_", body), name                          # every access is a global one
    for v in (1, 2, 4):
        for g in (1, 2, 4, 8, 16, 32, 64):
            (name,) = [k for k in quant if f"fcp_update_q8_kernelILi{v}ELi{g}EE" in k]
            body = _body(rows_asm, name)
            assert len(re.findall(r"\bv_div_fixup_f32\b", body)) == 2 and len(re.findall(r"\bv_div_fmas_f32\b", body)) == 2, name
            n_rint = len(re.findall(r"\bv_rndne_f32", body))
            assert n_rint >= v, name
            assert not re.search(r"\bv_pk_fma_f32|\bv_mac_f32|\bv_mad_f32", body), name
            assert len(re.findall(r"\bv_fma_f32|\bv_fmac_f32", body)) == 5 * 2, name
            assert len(re.findall(r"\bv_mul_f32", body)) + 2 * len(re.findall(r"\bv_pk_mul_f32", body)) >= n_rint + 2, name
            assert len(re.findall(r"\bv_sub_f32", body)) + 2 * len(re.findall(r"\bv_pk_add_f32", body)) >= n_rint + 1, name
            steps = g.bit_length() - 1
            assert len(re.findall(r"\bds_bpermute_b32\b|_dpp\b|\bv_permlane", body)) >= (2 * steps if steps else 0), name
            if g == 1:
                assert not re.search(r"\bds_bpermute_b32\b", body), name
            load = {4: "global_load_dwordx4", 2: "global_load_dwordx2", 1: "global_load_dword"}[v]
            store = {4: "global_store_dword", 2: "global_store_short", 1: "global_store_byte"}[v]
            assert re.search(r"\b" + load + r"\b", body) and re.search(r"\b" + store + r"\b", body), name
            assert re.search(r"\bglobal_load_dwordx2\b", body), name                  # the row's id
    for v in (1, 2, 4):                     # the streaming kernels: a slot is one load and one store of V elements
        (up,) = [k for k in stream if f"fcp_update_rows_kernelILi{v}EE" in k]
        (rd,) = [k for k in read if f"fcp_read_rows_kernelILi{v}EE" in k]
        st32 = {4: "global_store_dwordx4", 2: "global_store_dwordx2", 1: "global_store_dword"}[v]
        st16 = {4: "global_store_dwordx2", 2: "global_store_dword", 1: "global_store_short"}[v]
        assert re.search(r"\b" + st32 + r"\b", _body(rows_asm, up)) and re.search(r"\b" + st16 + r"\b", _body(rows_asm, up)), up
        assert re.search(r"\bv_cvt_f16_f32", _body(rows_asm, up)), up
        body = _body(rows_asm, rd)
        assert len(re.findall(r"\bv_fma_f32\b", body)) == v and re.search(r"\bv_cvt_f32_f16", body), rd     # q8: one fma per element
        assert re.search(r"\b" + st32 + r"\b", body), rd
