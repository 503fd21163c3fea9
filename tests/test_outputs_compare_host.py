"""fcp_outputs_compare / fcp_outputs_compare_workspace_bytes without a GPU: the two names and the 64-byte record in the header,
in lib.EXPORTS and in the loaded library; the workspace formula's properties; every FCP_ERR_INVALID_ARGUMENT in the documented
order (none needs a device, and no pointer is dereferenced); the ValueError of ops.compare_outputs; and the restatement of
outputs_compare_cases held to a plain Python loop.  (The kernels: tests/test_zzz_gpu_outputs_compare.py.)"""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import outputs_compare_cases as OC
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
INV, NODEV = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE
A = 1 << 20          # (pointers are never dereferenced on the host: plain numbers serve)


def test_header_declares_and_library_exports_the_two_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint64_t fcp_outputs_compare_workspace_bytes\(int32_t n_columns\);", text)
    assert re.search(r"\bint fcp_outputs_compare\(const void \*const \*ptrs_a, const int64_t \*row_strides_a, int32_t out_kind_a,\s+"
                     r"const void \*const \*ptrs_b,\s+const int64_t \*row_strides_b, int32_t out_kind_b,\s+const int32_t \*shapes.*?, "
                     r"int32_t n_columns,\s+fcp_output_error_t \*out[^,]*, void \*workspace,\s+int32_t device, void \*stream\);", text)
    names = {"fcp_outputs_compare_workspace_bytes", "fcp_outputs_compare"}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names)
    assert set(re.findall(r"\b(fcp_[a-z_0-9]+)\s*\(", text)) - {"fcp_alloc_fn"} == set(_lib.EXPORTS)
    # the record: 64 bytes, the header's field order in the ctypes mirror, in ops' NumPy dtype and in the tests' own
    body = re.search(r"typedef struct fcp_output_error \{(.*?)\} fcp_output_error_t; /\* 64 bytes \*/", text, re.S).group(1)
    fields = re.findall(r"^\s*(?:int64_t|double|float)\s+(\w+);", body, re.M)
    assert tuple(fields) == OC.FIELDS
    assert C.sizeof(_lib.OutputError) == 64 and tuple(f[0] for f in _lib.OutputError._fields_) == OC.FIELDS
    from recom_amd import ops
    assert ops.OUTPUT_ERROR_DTYPE == OC.RECORD and OC.RECORD.itemsize == 64 and OC.RECORD.names == OC.FIELDS
    for f in OC.FIELDS:
        assert getattr(_lib.OutputError, f).offset == OC.RECORD.fields[f][1], f


def test_workspace_bytes():
    """depends on n_columns alone; a multiple of 8; non-decreasing; holds the descriptors and n * T partial records; -1 for a
    negative argument"""
    L = _lib.load()
    ns = sorted(set(list(range(0, 200)) + [2 ** k + d for k in range(7, 31) for d in (-1, 0, 1)] + [1000, 1365, 1366, 4095, 4096, 4097,
                                                                                                 2 ** 31 - 1]))
    last = 0
    for n in ns:
        b = int(L.fcp_outputs_compare_workspace_bytes(n))
        assert b > 0 and b % 8 == 0 and b >= last, (n, b, last)
        t = OC.tiles_per_column(n)
        assert b >= 16 + 48 * n + 48 * n * t, (n, b, t)          # (48: the unit's descriptor and partial records)
        assert b <= 16 + 48 * n + 48 * (4096 + n), (n, b)
        last = b
    assert [OC.tiles_per_column(n) for n in (1, 64, 65, 1000, 4096, 4097, 5000)] == [64, 64, 64, 5, 1, 1, 1]
    for n in (-1, -2, -2 ** 31):
        assert int(L.fcp_outputs_compare_workspace_bytes(n)) == -1, n


def _compare(**kw):
    """two good columns ([3, 4] and [2, 5]), float32 against bf16, with the named arguments replaced"""
    good = dict(ptrs_a=[A, A + 64], strides_a=[4, 6], kind_a="f32", ptrs_b=[A + 2, A + 130], strides_b=[9, 5], kind_b="bf16",
                shapes=[3, 4, 2, 5], n=2, out=A, workspace=A)
    assert set(kw) <= set(good)
    good.update(kw)
    L = _lib.load()
    status = OC.call(L, good["ptrs_a"], good["strides_a"], good["kind_a"], good["ptrs_b"], good["strides_b"], good["kind_b"],
                     good["shapes"], good["n"], good["out"], good["workspace"])
    return status, L.fcp_last_error().decode()


def test_status_codes_arrive_in_the_stated_order():
    import torch
    cases = (
        (dict(ptrs_a=None), "`ptrs_a` is null"), (dict(strides_a=None), "`row_strides_a` is null"), (dict(ptrs_b=None), "`ptrs_b` is null"),
        (dict(strides_b=None), "`row_strides_b` is null"), (dict(shapes=None), "`shapes` is null"), (dict(shapes=None, n=-1), "`shapes` is null"),
        (dict(kind_a=3), "`out_kind_a`"), (dict(kind_a=-1), "`out_kind_a`"), (dict(kind_b=3), "`out_kind_b`"), (dict(kind_b=7, n=0), "`out_kind_b`"),
        (dict(n=-1), "`n_columns`"), (dict(n=-2 ** 31), "`n_columns`"),
        (dict(shapes=[3, 4, -1, 5]), "column 1: `shapes` holds negative rows"), (dict(shapes=[3, 0, 2, 5]), "column 0: `shapes` holds a dim"),
        (dict(shapes=[3, 4, 2, -5]), "column 1: `shapes` holds a dim"),
        (dict(strides_a=[3, 6]), "column 0: `row_strides_a`"), (dict(strides_b=[9, 4]), "column 1: `row_strides_b`"),
        (dict(strides_a=[4, -6]), "column 1: `row_strides_a`"),
        (dict(ptrs_a=[0, A]), "column 0: `ptrs_a` holds a null"), (dict(ptrs_b=[A, 0]), "column 1: `ptrs_b` holds a null"),
        (dict(ptrs_a=[A + 2, A]), "column 0: `ptrs_a` is not aligned to its 4-byte"), (dict(ptrs_a=[A, A + 1]), "column 1: `ptrs_a` is not aligned"),
        (dict(ptrs_b=[A + 1, A]), "column 0: `ptrs_b` is not aligned to its 2-byte"),
        (dict(ptrs_a=[A + 2, A], kind_a="f16", ptrs_b=[A + 2, A], kind_b="f32"), "column 0: `ptrs_b` is not aligned to its 4-byte"),
        (dict(out=0), "`out` is null"), (dict(out=0, n=0), "`out` is null"), (dict(workspace=0), "`workspace` is null"),
        (dict(workspace=0, n=0, ptrs_a=None, shapes=None), "`workspace` is null"),
        (dict(out=A + 4), "`out` is not 8-byte aligned"), (dict(workspace=A + 4), "`workspace` is not 8-byte aligned"),
    )
    for kw, word in cases:
        status, msg = _compare(**kw)
        assert status == INV and word in msg and msg.startswith("fcp_outputs_compare: "), (kw, status, msg)
    # the order: each call is wrong in everything that follows, too.  Per-column conditions go condition by condition, each over
    # the columns in ascending order (side a before side b within a column): column 1's short stride comes before column 0's
    # null pointer, column 1's null pointer before column 0's misaligned one
    bad = dict(ptrs_a=None, strides_a=None, ptrs_b=None, strides_b=None, shapes=None, kind_a=5, kind_b=9, n=-3, out=0, workspace=0)
    order = [("ptrs_a", [0, A + 1], "`ptrs_a` is null"), ("strides_a", [4, 2], "`row_strides_a` is null"),
             ("ptrs_b", [A + 1, 0], "`ptrs_b` is null"), ("strides_b", [1, 5], "`row_strides_b` is null"),
             ("shapes", [3, 0, -2, 5], "`shapes` is null"), ("kind_a", "f32", "`out_kind_a`"), ("kind_b", "bf16", "`out_kind_b`"),
             ("n", 2, "`n_columns`"),
             ("shapes", [3, 4, -2, 5], "column 0: `shapes` holds a dim"), ("shapes", [3, 4, 2, 5], "column 1: `shapes` holds negative rows"),
             ("strides_b", [4, 5], "column 0: `row_strides_b`"), ("strides_a", [4, 5], "column 1: `row_strides_a`"),
             ("ptrs_a", [A, A + 1], "column 0: `ptrs_a` holds a null"), ("ptrs_b", [A + 1, A], "column 1: `ptrs_b` holds a null"),
             ("ptrs_b", [A, A], "column 0: `ptrs_b` is not aligned"), ("ptrs_a", [A, A], "column 1: `ptrs_a` is not aligned"),
             ("out", A + 4, "`out` is null"), ("workspace", A + 4, "`workspace` is null"), ("out", A, "`out` is not 8"),
             ("workspace", A, "`workspace` is not 8")]
    for name, fixed, word in order:
        status, msg = _compare(**bad)
        assert status == INV and word in msg, (name, msg)
        bad[name] = fixed
    # the sentences around the shared staging routine (upload_image, fcp_host.h), whole: the workspace's two, and — no device
    # here, so from the unit's text with its adjacent string literals joined — the refusal of a capturing stream
    assert _compare(workspace=0) == (INV, "fcp_outputs_compare: `workspace` is null")
    assert _compare(workspace=A + 4) == (INV, "fcp_outputs_compare: `workspace` is not 8-byte aligned")
    with open(os.path.join(ROOT, "recom_amd", "csrc", "fcp_outputs_compare.hip")) as f:
        unit = re.sub(r'"\s*\n\s*"', "", f.read())
    assert ('fail(FCP_ERR_UNSUPPORTED, "fcp_outputs_compare: stream capture of a call with columns: their descriptors are installed from '
            'the host by every call, which a replay would not repeat")') in unit
    assert unit.index("stream_is_capturing(stream)") < unit.index("wait_for_inputs(ptrs_a")     # refused in front of the waits
    if not torch.cuda.is_available():
        assert _compare(**bad)[0] == NODEV
        # what IS valid gets as far as the device: rows 0 with null pointers, n_columns 0 with null arrays (the zero record is
        # written on the device), every pair of kinds, a 16-bit column at an odd element
        for kw in (dict(), dict(shapes=[0, 4, 0, 5], ptrs_a=[0, 0], ptrs_b=[0, 0]), dict(n=0),
                   dict(n=0, ptrs_a=None, strides_a=None, ptrs_b=None, strides_b=None, shapes=None), dict(ptrs_b=[A + 2, A + 6])):
            assert _compare(**kw)[0] == NODEV, kw
        for ka, kb in OC.KIND_PAIRS:
            assert _compare(kind_a=ka, kind_b=kb, ptrs_a=[A, A], ptrs_b=[A, A])[0] == NODEV, (ka, kb)


def test_compare_outputs_refuses_results_of_different_requests():
    from recom_amd import ops

    def outputs(shapes):
        n = len(shapes) // 2
        return ops.ProcessOutputs(np.zeros(n, np.int64), np.asarray(shapes, np.int32), np.ones(n, np.int64), None, [], np.zeros(0, np.int32))

    with pytest.raises(ValueError, match=r"column 1 is \[5, 8\] in a and \[5, 4\] in b"):
        ops.compare_outputs(outputs([5, 8, 5, 8, 7, 2]), outputs([5, 8, 5, 4, 6, 2]))
    with pytest.raises(ValueError, match=r"column 2 is \[7, 2\] in a and \[6, 2\] in b"):
        ops.compare_outputs_async(outputs([5, 8, 5, 8, 7, 2]), outputs([5, 8, 5, 8, 6, 2]))
    with pytest.raises(ValueError, match="3 columns against 2"):
        ops.compare_outputs(outputs([5, 8, 5, 8, 7, 2]), outputs([5, 8, 5, 8]))
    e = ops.OutputErrors(np.zeros(2, OC.RECORD).view(np.recarray), np.zeros(1, OC.RECORD).view(np.recarray)[0])
    assert e.identical and e.rel_rms() == 0.0 and e.rel_rms(1) == 0.0
    e.columns[1].sum_sq_err, e.columns[1].sum_sq_ref, e.total.differ = 4.0, 16.0, 3
    assert e.rel_rms(1) == 0.5 and not e.identical


def _bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _python_loop(a, b):
    """the value model with Python floats: a and b are lists of rows of float32 values given as Python floats"""
    r = dict(elems=0, differ=0, nonfinite=0, first_differ_row=-1, sum_sq_ref=0.0, sum_sq_err=0.0, max_abs_err=0.0, max_abs_ref=0.0, reserved=0)
    for i, (ra, rb) in enumerate(zip(a, b)):
        for x, y in zip(ra, rb):
            r["elems"] += 1
            if _bits(x) != _bits(y):
                r["differ"] += 1
                if r["first_differ_row"] < 0:
                    r["first_differ_row"] = i
            if math.isnan(x) or math.isinf(x) or math.isnan(y) or math.isinf(y):
                r["nonfinite"] += 1
                continue
            try:
                e = struct.unpack("<f", struct.pack("<f", y - x))[0]       # the float64 difference of two float32 values, rounded to float32
            except OverflowError:
                e = math.copysign(math.inf, y - x)
            r["sum_sq_ref"] += x * x
            r["sum_sq_err"] += e * e
            r["max_abs_err"] = max(r["max_abs_err"], abs(e))
            r["max_abs_ref"] = max(r["max_abs_ref"], abs(x))
    return r


def test_the_restatement_against_a_python_loop():
    """a handful of tiny columns whose sums are exact in float64 in any order (small dyadic values), so equality is asked"""
    nan, inf = float("nan"), float("inf")
    tiny = [
        ([[1.0, 2.0], [3.0, -4.0]], [[1.0, 2.0], [3.0, -4.0]]),                       # equal
        ([[1.0, 2.0], [3.0, -4.0]], [[1.0, 2.5], [3.0, -4.25]]),
        ([[0.0, -0.0, 1.5]], [[-0.0, -0.0, 1.5]]),                                      # +0 against -0 differs
        ([[nan, 1.0], [2.0, inf], [0.5, 0.25]], [[nan, 1.0], [nan, inf], [0.5, 0.75]]),   # equal NaNs, a NaN on one side, equal infs
        ([[inf], [1.0]], [[-inf], [1.0]]),
        ([[2.0 ** -149, 2.0 ** -130]], [[3 * 2.0 ** -149, 0.0]]),                      # denormals
        ([[0.0, 2.0 ** 127]], [[2.0 ** 127, 0.0]]),
        ([[-(2.0 ** 127)]], [[2.0 ** 127]]),                                            # e = 2^128 overflows float32: +inf
        ([], []),
    ]
    for a, b in tiny:
        dim = len(a[0]) if a else 3
        got = OC.restate_column(np.asarray(a, np.float32).reshape(len(a), dim), "f32", np.asarray(b, np.float32).reshape(len(b), dim), "f32")
        want = _python_loop(a, b)
        for f in OC.FIELDS:
            assert float(got[f]) == float(want[f]), (a, b, f, got[f], want[f])
    # a 16-bit side is widened first: bf16 0x3F80 is 1.0, fp16 0x3C01 is 1 + 2^-10
    got = OC.restate_column(np.asarray([[0x3F80, 0x7FC0]], np.uint16), "bf16", np.asarray([[0x3C01, 0x7E00]], np.uint16), "f16")
    assert (int(got["differ"]), int(got["nonfinite"]), float(got["sum_sq_err"]), float(got["max_abs_err"])) == (1, 1, 2.0 ** -20, 2.0 ** -10)
    total = OC.restate_total(np.array([OC.restate_column(np.asarray(a, np.float32).reshape(len(a), -1) if a else np.zeros((0, 3), np.float32), "f32",
                                                         np.asarray(b, np.float32).reshape(len(b), -1) if b else np.zeros((0, 3), np.float32), "f32")
                                       for a, b in tiny[:3]], OC.RECORD))
    assert (int(total["elems"]), int(total["differ"]), int(total["first_differ_row"]), float(total["max_abs_err"])) == (11, 3, 0, 0.5)
    assert int(OC.restate_total(np.zeros(0, OC.RECORD))["first_differ_row"]) == -1


def test_the_edge_matrix_holds_what_it_is_for():
    """every dim, row count and layout; every special at every corner; columns beyond T and 2 T row tiles; unaligned bases"""
    cols = OC.edge_columns()
    assert {(r, d) for r, d, _ in cols} >= {(r, d) for r in OC.ROWS for d in OC.DIMS}
    assert {lay for _, _, lay in cols} == set(OC.LAYOUTS)
    seen = set()
    for k, (r, d, _) in enumerate(cols):
        if r >= 2 and d >= 2 and not OC.is_equal_column(k):
            seen |= {(OC.corner_special(k, c), c) for c in range(4)}
    assert seen == {(s, c) for s in OC.INJECTED for c in range(4)}
    assert sum(OC.is_equal_column(k) for k in range(len(cols))) >= 20
    m = OC.edge_matrix("f32", "bf16")
    want = m["want"]
    assert want["differ"][-1] > 0 and want["nonfinite"][-1] > 0 and (want["differ"][:-1] == 0).sum() >= len(cols) // 9
    assert want["sum_sq_err"][:-1].max() > 2.0 ** 250 and np.isinf(want["max_abs_err"][:-1]).sum() == 0
    for side, eb in (("a", 4), ("b", 2)):
        offs = np.asarray([w[0] for w in m[side]["where"]])
        assert (offs % 2 == 1).any() and (offs % 4 == 0).any()
        assert {w[1] - d for w, (_, d) in zip(m[side]["where"], m["columns"])} >= {0, 1}
