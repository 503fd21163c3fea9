"""fcp_table_convert / fcp_table_row_bytes without a GPU: the quantiser's definition pinned against PyTorch's CPU op, the
error bound checked on that op's own output, the C ABI's surface and status order, and the code object of
recom_amd/csrc/fcp_convert.hip.  (The kernels themselves: tests/test_gpu_table_convert.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import table_convert_cases as TC
from recom_amd import lib as _lib
from recom_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
F32, BF16, F16, Q8 = (TC.KINDS[k] for k in ("f32", "bf16", "f16", "q8"))


def _prepack(x: np.ndarray) -> np.ndarray:
    import torch
    return torch.ops.quantized.embedding_bag_byte_prepack(torch.from_numpy(np.array(x, np.float32))).numpy()


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, what
    bad = np.argwhere((got != want).any(axis=1))[:, 0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} rows differ, first row {bad[0]}: {got[bad[0]]} want {want[bad[0]]}"


# ---- the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (1, 2, 3, 4, 7, 16, 33, 64, 127, 300))
def test_restatement_equals_torch_prepack_on_the_families(dim):
    """quantize_ref == quantized::embedding_bag_byte_prepack, byte for byte: Gaussian rows, rows near 5 with a 1e-3 spread,
    small integers, magnitudes of 1e30, constant rows."""
    x = TC.family_rows(dim, 2000, 3)
    _same_bytes(TC.quantize_ref(x), _prepack(x), ("families", dim))
    const = x[4::5]
    q = TC.quantize_ref(const)
    assert (q[:, :dim] == 0).all() and (q[:, dim:dim + 4] == 0).all()        # R = 0: codes 0, scale +0.0


@pytest.mark.parametrize("dim", (1, 2, 3, 5, 8, 64, 257, 300))
def test_restatement_equals_torch_prepack_on_the_edge_list(dim):
    """A tie at every half-integer code, min / max at the first and the last element, R subnormal, R near 1e-8, R near
    FLT_MAX / 2 (TC.edge_rows)."""
    x = TC.edge_rows(dim)
    ref = TC.quantize_ref(x)
    _same_bytes(ref, _prepack(x), ("edges", dim))
    if dim > 2:
        # the tie rows do what they are there for: scale 1, and every k + 0.5 went to the even neighbour
        n_tie = -(-255 // (dim - 2))
        ties, codes = x[:n_tie, 1:-1], ref[:n_tie, 1:dim - 1]
        assert (synth.q8_fields(ref[:n_tie])[1] == 1.0).all()
        assert (ties % 1 == 0.5).all() and (codes % 2 == 0).all() and (np.abs(codes - ties) == 0.5).all()
        assert set(np.unique(ties)) == set(np.arange(255) + 0.5)


def test_the_rows_of_the_gpu_test_follow_the_same_definition():
    """The GPU test's expectation is quantize_ref on TC.quant_rows: hold exactly those rows to torch too."""
    for dim in TC.QUANT_DIMS:
        _same_bytes(TC.quant_expectation(dim), _prepack(TC.quant_rows(dim)), ("quant_rows", dim))
    assert {TC.vec_of(d) for d in TC.QUANT_DIMS} == {1, 2, 4}
    assert {TC.group_of(d) for d in TC.QUANT_DIMS} == {1, 2, 4, 8, 16, 32, 64}
    for v, cap in TC.REGISTER_CAP.items():       # the register cap is crossed in each V
        dims = [d for d in TC.QUANT_DIMS if TC.vec_of(d) == v and TC.group_of(d) == 64]
        assert any(d <= cap for d in dims) and any(d > cap for d in dims), (v, dims)
    big = TC.big_rows_numpy(np.arange(0, 3000))
    assert np.isfinite(big).all() and len(np.unique(big)) == 1021


def test_error_bound_holds_for_torch_prepack():
    """For a row with R > 0:  |dequantised - x| <= 0.5 * scale + 1e-8 + 2^-22 * max(|mn|, |mx|), in float64.

    Derivation (u = 2^-24, the unit roundoff; M = max(|mn|, |mx|); Re = mx - mn exactly, Re <= 2 M; every d_i below is one
    rounding, |d_i| <= u):
      t = x - mn exactly, 0 <= t <= Re;  t' = fl(t) = t (1 + d1);  R = fl(Re);  inv = fl(255 / fl(R + 1e-8)) =
      255 / (R + 1e-8) * (1 + d2)(1 + d3);  p = fl(t' inv) = t' inv (1 + d4);  the code c = rint(p), |c - p| <= 0.5;
      scale = fl(R / 255) = R / 255 * (1 + d5);  the dequantised value d = fma(c, scale, mn) = (c scale + mn)(1 + d6).
      d - x = (c - p) scale  +  (p scale - t)  +  d6 (c scale + mn), and
        |(c - p) scale| <= 0.5 scale                                        the rounding of the code;
        p scale = t * R / (R + 1e-8) * (1 + th), |th| <= 5 u + O(u^2): since inv <= 255 / R (up to its roundings) the
          product never overshoots t by more than those roundings, and it falls short of t by t * 1e-8 / (R + 1e-8) <= 1e-8
          — the 1e-8 of the denominator, whole; what is left is |t th| <= 5 u Re <= 10 u M;
        |d6 (c scale + mn)| <= u (M + the terms above).
      Worst case, every rounding at its limit and aligned: 0.5 scale + 1e-8 + 11 u M.  The stated last term, 2^-22 M = 4 u M,
      is what five independent roundings reach in practice, not in the worst case: t' is exact whenever x and mn are within
      a factor of two (Sterbenz), the 5 u Re term needs Re near 2 M, and then 0.5 scale = Re / 510 is 10^4 times larger than
      u M and is itself never met with equality by all roundings at once.  So the bound is CHECKED here, element by element,
      on the reference's own output for every family and every edge row, before the GPU test relies on it.  It holds on
      all of them, and nothing had to be widened."""
    worst = 0.0
    for dim in (1, 2, 3, 7, 16, 64, 300):
        x = np.concatenate([TC.family_rows(dim, 1500, 9), TC.edge_rows(dim)])
        q = _prepack(x)
        deq = synth.dequantize_q8(q).astype(np.float64)
        live = (x.max(axis=1) - x.min(axis=1)) > 0
        assert live.sum() > 1000 or dim == 1
        err = np.abs(deq - x.astype(np.float64))[live]
        bound = TC.error_bound(x)[live]
        assert np.isfinite(err).all()
        ratio = (err / bound[:, None]).max() if err.size else 0.0
        worst = max(worst, float(ratio))
        assert (err <= bound[:, None]).all(), (dim, float(ratio))
    print(f"largest |error| / bound over torch's prepack output: {worst:.4f}")
    assert 0.5 < worst <= 1.0              # (the bound is not vacuous: some element comes within a factor of two)


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint64_t fcp_table_row_bytes\(int32_t kind, int32_t dim\);", text)
    assert re.search(r"\bint fcp_table_convert\(void \*dst, int32_t dst_kind, int64_t dst_row0, const void \*src, int32_t src_kind, "
                     r"int64_t rows,\s+int32_t dim, int32_t device, void \*stream\);", text)
    assert "must NOT overlap" in text and "Plans do not quantise" in text
    assert {"fcp_table_row_bytes", "fcp_table_convert"} <= set(_lib.EXPORTS)
    L = _lib.load()
    assert hasattr(L, "fcp_table_row_bytes") and hasattr(L, "fcp_table_convert")
    assert _lib.TABLE_KINDS == TC.KINDS
    assert re.search(r"enum \{ FCP_TAB_F32 = 0, FCP_TAB_BF16 = 1, FCP_TAB_F16 = 2 \}", text) and re.search(r"FCP_TAB_Q8 = 3\b", text)


def test_row_bytes():
    from recom_amd import tables
    L = _lib.load()
    for dim in (1, 3, 8, 64, 1000, 2 ** 31 - 1):
        assert [L.fcp_table_row_bytes(k, dim) for k in (F32, BF16, F16, Q8)] == [4 * dim, 2 * dim, 2 * dim, dim + 8]
        assert [tables.row_bytes(n, dim) for n in ("f32", "bf16", "f16", "q8")] == [4 * dim, 2 * dim, 2 * dim, dim + 8]
    for kind in (-1, 4, 99):
        assert L.fcp_table_row_bytes(kind, 8) == -1
    for kind in (F32, BF16, F16, Q8):
        assert L.fcp_table_row_bytes(kind, 0) == -1 and L.fcp_table_row_bytes(kind, -5) == -1
    with pytest.raises(ValueError):
        tables.row_bytes("q4", 8)
    with pytest.raises(ValueError):
        tables.row_bytes("q8", 0)


def _convert(dst, dst_kind, dst_row0, src, src_kind, rows, dim, device=0):
    L = _lib.load()
    status = L.fcp_table_convert(C.c_void_p(dst), dst_kind, dst_row0, C.c_void_p(src), src_kind, rows, dim, device, None)
    return status, L.fcp_last_error().decode()


def test_status_codes_arrive_in_the_stated_order():
    """No GPU here: valid arguments end in FCP_ERR_NO_DEVICE — after every argument check, after FCP_ERR_UNSUPPORTED and
    after the FCP_OK of rows == 0.  (Pointers are never dereferenced on the host: plain numbers serve.)"""
    import torch
    no_gpu = not torch.cuda.is_available()      # (with a GPU valid arguments would run: only the device-free statuses are checked)
    INV, UNS, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_UNSUPPORTED, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK
    A = 1 << 20                                                   # an address aligned for everything
    # 1. invalid arguments, each named
    for args, word in (((0, Q8, 0, A, F32, 5, 64), "dst"), ((A, Q8, 0, 0, F32, 5, 64), "src"),
                       ((A, 4, 0, A, F32, 5, 64), "dst_kind"), ((A, Q8, 0, A, -1, 5, 64), "src_kind"),
                       ((A, Q8, 0, A, F32, 5, 0), "dim"), ((A, Q8, 0, A, F32, 5, -3), "dim"),
                       ((A, Q8, 0, A, F32, -1, 64), "rows"), ((A, Q8, -1, A, F32, 5, 64), "dst_row0"),
                       ((A, Q8, 2 ** 32 - 10, A, F32, 7, 64), "dst_row0"),
                       ((A + 2, Q8, 0, A, F32, 5, 63), "dst"),            # a q8 base is 4-byte aligned whatever the dim
                       ((A, Q8, 0, A + 4, F32, 5, 64), "src"),            # float32, V 4: 16 bytes
                       ((A, Q8, 0, A + 4, F32, 5, 62), "src"),            # V 2: 8 bytes
                       ((A + 4, BF16, 0, A, F32, 5, 64), "dst"),          # 16-bit, V 4: 8 bytes
                       ((A + 2, F16, 0, A, F32, 5, 62), "dst"),           # V 2: 4 bytes
                       ((A + 1, F16, 0, A, F32, 5, 61), "dst"),           # V 1: 2 bytes
                       ((A, F32, 0, A + 2, Q8, 5, 64), "src"),
                       ((A, F32, 0, A, F32, 5, 64), "dst_kind"), ((A, Q8, 0, A, Q8, 5, 64), "dst_kind"),
                       ((A, BF16, 0, A, BF16, 5, 64), "dst_kind")):
        status, msg = _convert(*args)
        assert status == INV and word in msg, (args, status, msg)
    # alignments that ARE enough pass the argument checks
    for args in ((A + 4, Q8, 0, A + 4, F32, 5, 63), (A + 8, BF16, 0, A + 16, F32, 5, 64), (A + 4, F16, 0, A + 8, F32, 5, 62),
                 (A + 2, BF16, 0, A + 4, F32, 5, 61), (A + 4, F32, 0, A + 4, Q8, 5, 61), (A + 16, F32, 0, A + 8, F16, 5, 64)):
        assert _convert(*args[:5], 0, args[6])[0] == OK, args                   # (rows == 0: past every argument check)
        if no_gpu:
            assert _convert(*args)[0] == NODEV, args
    # an invalid argument wins over an unsupported pair, and over rows == 0
    assert _convert(A + 1, Q8, 0, A, BF16, 5, 64)[0] == INV
    assert _convert(A, Q8, 0, A, F32, 0, 0)[0] == INV
    assert _convert(A + 1, Q8, 0, A, F32, 0, 64)[0] == INV
    # 2. unsupported pairs: before rows == 0, before the device
    for d, s in ((BF16, F16), (F16, BF16), (Q8, BF16), (Q8, F16), (BF16, Q8), (F16, Q8)):
        for rows in (0, 5):
            status, msg = _convert(A, d, 0, A, s, rows, 64)
            assert status == UNS and "float32" in msg, (d, s, rows, status, msg)
    # 3. rows == 0: FCP_OK with no launch and no device, null pointers included
    for d, s in ((Q8, F32), (F32, Q8), (BF16, F32), (F32, F16)):
        assert _convert(A, d, 0, A, s, 0, 64)[0] == OK
        assert _convert(0, d, 3, 0, s, 0, 7)[0] == OK
    # 4. everything valid: no device
    for d, s in ((Q8, F32), (F32, Q8), (BF16, F32), (F16, F32), (F32, BF16), (F32, F16)):
        if no_gpu:
            assert _convert(A, d, 0, A, s, 5, 64)[0] == NODEV
            assert _convert(A, d, 2 ** 32 - 10, A, s, 6, 64)[0] == NODEV      # the last rows below the limit


def test_python_wrapper_refuses_what_it_can_see():
    import torch
    from recom_amd import tables
    x = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="device to device"):
        tables.convert(x, "q8")
    with pytest.raises(ValueError, match="unknown table dtype"):
        tables.convert(x, "q4")
    with pytest.raises(ValueError, match="no table format"):
        tables.convert(x.double(), "q8")
    with pytest.raises(ValueError, match="float32"):
        tables.convert_from_host(x.half(), "q8", "cpu")


# ---- code object -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def convert_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("asm") / "fcp_convert.s"
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                           os.path.join(ROOT, "recom_amd", "csrc", "fcp_convert.hip"), "-o", str(asm)],
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


def test_code_object_of_the_convert_kernels(convert_asm):
    """fcp_convert.hip compiles for gfx950; no kernel has scratch or LDS; denormals are kept and IEEE mode is on, as in the
    other units.  The quantisers: 3 V x 7 G, their group reduction without LDS instructions that touch memory, the divisions
    the correctly rounded sequence, rint the hardware's round-to-nearest-even, code stores of V bytes."""
    kernels = _kernels(convert_asm)
    quant = {k for k in kernels if "fcp_quantize_q8_kernel" in k}
    others = {frag: [k for k in kernels if frag in k] for frag in ("fcp_dequantize_q8_kernel", "fcp_narrow16_kernel", "fcp_widen16_kernel")}
    assert len(quant) == 21 and all(len(v) == 3 for v in others.values()) and len(kernels) == 30, sorted(kernels)
    for name, desc in sorted(kernels.items()):
        assert _field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        assert _field(desc, "group_segment_fixed_size") == 0, f"{name}: uses LDS"
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc), f"{name}: fp32 subnormals are flushed"
        assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", desc), f"{name}: fp16 subnormals are flushed"
        assert re.search(r"\.amdhsa_ieee_mode 1\b", desc), f"{name}: not in IEEE mode"
        assert _field(desc, "next_free_vgpr") <= 64, name                     # 8 waves per SIMD: the kernels wait on memory
        body = _body(convert_asm, name)
        assert not re.search(r"\b(scratch_|ds_read|ds_write|ds_load|ds_store)", body), name
    for v in (1, 2, 4):
        for g in (1, 2, 4, 8, 16, 32, 64):
            (name,) = [k for k in quant if f"fcp_quantize_q8_kernelILi{v}ELi{g}EE" in k]
            body = _body(convert_asm, name)
            # two correctly rounded divisions, the rounding of the codes, no approximate reciprocal on its own
            assert len(re.findall(r"\bv_div_fixup_f32\b", body)) == 2 and len(re.findall(r"\bv_div_fmas_f32\b", body)) == 2, name
            n_rint = len(re.findall(r"\bv_rndne_f32", body))
            assert n_rint >= v, name
            # nothing contracted: every fused multiply-add of the body belongs to a division's expansion (five each), and every
            # code has a multiplication and a subtraction of its own
            assert not re.search(r"\bv_pk_fma_f32|\bv_mac_f32|\bv_mad_f32", body), name
            assert len(re.findall(r"\bv_fma_f32|\bv_fmac_f32", body)) == 5 * 2, name
            assert len(re.findall(r"\bv_mul_f32", body)) + 2 * len(re.findall(r"\bv_pk_mul_f32", body)) >= n_rint + 2, name
            assert len(re.findall(r"\bv_sub_f32", body)) + 2 * len(re.findall(r"\bv_pk_add_f32", body)) >= n_rint + 1, name
            # the butterflies: log2(G) exchanges of min and of max
            steps = g.bit_length() - 1
            assert len(re.findall(r"\bds_bpermute_b32\b|_dpp\b|\bv_permlane", body)) >= (2 * steps if steps else 0), name
            if g == 1:
                assert not re.search(r"\bds_bpermute_b32\b", body), name
            load = {4: "global_load_dwordx4", 2: "global_load_dwordx2", 1: "global_load_dword"}[v]
            store = {4: "global_store_dword", 2: "global_store_short", 1: "global_store_byte"}[v]
            assert re.search(r"\b" + load + r"\b", body) and re.search(r"\b" + store + r"\b", body), name
