"""fcp_table_count_ids / fcp_table_audit_weighted without a GPU: the two names in the header, in lib.EXPORTS and in the loaded
library; every FCP_ERR_INVALID_ARGUMENT of both entries in the documented order (no device is needed for any of them); n == 0;
what the Python wrappers refuse; and the restated references of table_traffic_cases on themselves.  (The kernels:
tests/test_gpu_table_traffic.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import table_audit_cases as TA
import table_traffic_cases as TT
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
INV, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK
A = 1 << 20          # (pointers are never dereferenced on the host: plain numbers serve)


def test_header_declares_and_library_exports_the_two_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint fcp_table_count_ids\(uint32_t \*counts, int64_t table_rows, const void \*ids, int32_t id_bytes, int64_t n,\s+"
                     r"int64_t \*skipped,\s+int32_t device, void \*stream\);", text)
    assert re.search(r"\bint fcp_table_audit_weighted\(const float \*src, int64_t rows, int32_t dim, const uint32_t \*row_counts,\s+"
                     r"fcp_table_audit_t \*out,\s+void \*workspace, int32_t device, void \*stream\);", text)
    names = {"fcp_table_count_ids", "fcp_table_audit_weighted"}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names)
    # the header's surface and the mirror agree (tests/test_host.py holds the same for every entry)
    assert set(re.findall(r"\b(fcp_[a-z_0-9]+)\s*\(", text)) - {"fcp_alloc_fn"} == set(_lib.EXPORTS)


def _count(counts, table_rows, ids, id_bytes, n, skipped, device=0):
    L = _lib.load()
    status = L.fcp_table_count_ids(C.c_void_p(counts), table_rows, C.c_void_p(ids), id_bytes, n, C.c_void_p(skipped), device, None)
    return status, L.fcp_last_error().decode()


def test_count_ids_status_codes_arrive_in_the_stated_order():
    import torch
    no_gpu = not torch.cuda.is_available()
    for args, word in (((A, 5, A, 8, -1, 0), "`n`"),
                       ((A, 0, A, 8, 3, 0), "`table_rows`"), ((A, -7, A, 8, 3, 0), "`table_rows`"), ((A, 2 ** 32 - 3, A, 8, 3, 0), "`table_rows`"),
                       ((A, 5, A, 0, 3, 0), "`id_bytes`"), ((A, 5, A, 2, 3, 0), "`id_bytes`"), ((A, 5, A, 16, 3, 0), "`id_bytes`"),
                       ((A, 5, A, -8, 3, 0), "`id_bytes`"),
                       ((0, 5, A, 8, 3, 0), "`counts`"), ((A, 5, 0, 8, 3, 0), "`ids`"), ((A, 5, 0, 4, 1, A), "`ids`"),
                       ((A + 2, 5, A, 8, 3, 0), "`counts`"), ((A + 1, 5, A, 4, 0, 0), "`counts`"),
                       ((A, 5, A + 4, 8, 3, 0), "`ids`"), ((A, 5, A + 2, 4, 3, 0), "`ids`"), ((A, 5, A + 12, 8, 0, 0), "`ids`"),
                       ((A, 5, A, 8, 3, A + 4), "`skipped`"), ((A, 5, A, 4, 0, A + 2), "`skipped`")):
        status, msg = _count(*args)
        assert status == INV and word in msg and msg.startswith("fcp_table_count_ids"), (args, status, msg)
    # the order of fcp_table_update_rows: n, table_rows, (the entry's own) id_bytes, null pointers, alignment
    assert "`n`" in _count(0, 0, 0, 3, -1, 4)[1]
    assert "`table_rows`" in _count(0, 0, 0, 3, 2, 4)[1]
    assert "`id_bytes`" in _count(0, 5, 0, 3, 2, 4)[1]
    assert "`counts`" in _count(0, 5, 0, 8, 2, 4)[1]
    assert "`ids`" in _count(A + 2, 5, 0, 8, 2, 4)[1]
    assert "`counts`" in _count(A + 2, 5, A + 4, 8, 2, 4)[1]
    assert "`ids`" in _count(A, 5, A + 4, 8, 2, 4)[1]
    assert "`skipped`" in _count(A, 5, A + 8, 8, 2, 4)[1]
    # n == 0 is FCP_OK without a device (a device index no machine has), null pointers included
    for args in ((0, 1, 0, 8, 0, 0), (A, 2 ** 32 - 4, A + 4, 4, 0, A + 8), (0, 5, 0, 4, 0, 0)):
        assert _count(*args, device=4097)[0] == OK, args
    if no_gpu:
        # alignments that ARE enough, skipped NULL, the two ends of table_rows
        for args in ((A + 4, 1, A + 8, 8, 3, 0), (A + 4, 2 ** 32 - 4, A + 4, 4, 3, A + 8), (A, 5, A, 8, 2 ** 40, 0)):
            assert _count(*args)[0] == NODEV, args


def _audit_w(src, rows, dim, row_counts, out, workspace, device=0):
    L = _lib.load()
    status = L.fcp_table_audit_weighted(C.c_void_p(src), rows, dim, C.c_void_p(row_counts), C.c_void_p(out), C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def test_weighted_audit_status_codes_arrive_in_the_audit_s_order():
    """fcp_table_audit's checks in fcp_table_audit's order (tests/test_table_audit_host.py), row_counts joining them: null with
    rows > 0 behind a null src, its alignment behind src's."""
    import torch
    no_gpu = not torch.cuda.is_available()
    for args, word in (((A, -1, 64, A, A, A), "rows"), ((A, 2 ** 32 - 3, 64, A, A, A), "rows"), ((A, 2 ** 40, 64, A, A, A), "rows"),
                       ((A, 5, 0, A, A, A), "dim"), ((A, 5, -3, A, A, A), "dim"),
                       ((A, 5, 64, A, 0, A), "out"), ((A, 5, 64, A, A, 0), "workspace"), ((A, 0, 64, 0, 0, A), "out"), ((0, 0, 64, 0, A, 0), "workspace"),
                       ((0, 5, 64, A, A, A), "src"),
                       ((A, 5, 64, 0, A, A), "row_counts"), ((A, 1, 1, 0, A, A), "row_counts"),
                       ((A + 4, 5, 64, A, A, A), "src"), ((A + 8, 5, 64, A, A, A), "src"), ((A + 4, 5, 62, A, A, A), "src"), ((A + 2, 5, 61, A, A, A), "src"),
                       ((A, 5, 64, A + 2, A, A), "row_counts"), ((A, 0, 64, A + 1, A, A), "row_counts"), ((A + 4, 5, 61, A + 3, A, A), "row_counts"),
                       ((A, 5, 64, A, A + 4, A), "out"), ((A, 5, 64, A, A, A + 4), "workspace")):
        status, msg = _audit_w(*args)
        assert status == INV and word in msg and msg.startswith("fcp_table_audit_weighted:"), (args, status, msg)
    assert "rows" in _audit_w(0, -1, 0, 0, 0, 0)[1]
    assert "dim" in _audit_w(0, 5, 0, 0, 0, 0)[1]
    assert "out" in _audit_w(0, 2 ** 32, 64, 0, 0, 0)[1]
    assert "workspace" in _audit_w(0, 2 ** 32, 64, 0, A, 0)[1]
    assert "src" in _audit_w(0, 2 ** 32, 64, 0, A, A)[1]
    assert "row_counts" in _audit_w(A + 4, 2 ** 32, 64, 0, A, A)[1]
    assert "rows must" in _audit_w(A + 4, 2 ** 32, 64, A + 2, A, A)[1]
    assert "src" in _audit_w(A + 4, 5, 64, A + 2, A + 4, A + 4)[1]
    assert "row_counts" in _audit_w(A, 5, 64, A + 2, A + 4, A + 4)[1]
    assert "out" in _audit_w(A, 5, 64, A + 4, A + 4, A + 4)[1]
    # the unweighted entry keeps its name in its messages
    L = _lib.load()
    assert L.fcp_table_audit(C.c_void_p(A), -1, 64, C.c_void_p(A), C.c_void_p(A), 0, None) == INV
    assert L.fcp_last_error().decode().startswith("fcp_table_audit:")
    if no_gpu:
        for args in ((A + 16, 5, 64, A + 4, A + 8, A + 8), (A + 4, 5, 61, A + 12, A, A), (0, 0, 64, 0, A, A), (A, 2 ** 32 - 4, 64, A, A, A)):
            assert _audit_w(*args)[0] == NODEV, args


def test_python_wrappers_refuse_what_they_can_see():
    import torch
    from recom_amd import tables
    import table_mixed_cases as TM
    t = torch.zeros((4, 8))
    for cells in (3, 5, 0):
        with pytest.raises(ValueError, match=f"row_counts has {cells} cells, the table 4 rows"):
            tables.audit(t, row_counts=torch.zeros((cells,), dtype=torch.int32))
    with pytest.raises(ValueError, match="uint32"):
        tables.audit(t, row_counts=torch.zeros((4,), dtype=torch.int64))
    with pytest.raises(ValueError, match="uint32"):
        tables.audit(t, row_counts=torch.zeros((4, 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="device to device"):          # (a matching pair on the host: the table's own refusal)
        tables.audit(t, row_counts=torch.zeros((4,), dtype=torch.int32))
    with pytest.raises(ValueError, match="row_counts names 1 inputs"):
        tables.audit_tables(TM.small_mixed_spec(), [t, t, t], row_counts=[None])
    with pytest.raises(ValueError, match="on the device"):
        tables.count_ids(torch.zeros((4,), dtype=torch.int32), torch.zeros((3,), dtype=torch.int64))
    with pytest.raises(ValueError, match="uint32"):
        tables.count_ids(torch.zeros((4,), dtype=torch.float32), torch.zeros((3,), dtype=torch.int64))
    c = tables.new_counts(5, "cpu")
    assert c.shape == (5,) and c.dtype in (getattr(torch, "uint32", torch.int32), torch.int32) and not c.numpy().any()


def test_the_restated_references():
    """count_ref: bincount, modulo 2^32, skipped ids, int32 widened with its sign.  weighted_aggregate: all-ones counts are the
    unweighted aggregate (a float64 sum of the same terms times 1.0), zero counts give zero sums, and a hand-made case."""
    got, skipped = TT.count_ref(4, np.asarray([0, 3, 3, -1, 4, 2 ** 32 + 1, TT.INT64_MIN, 3], np.int64))
    assert got.tolist() == [1, 0, 0, 3] and got.dtype == np.uint32 and skipped == 4
    got, skipped = TT.count_ref(2, np.asarray([[1, -5], [1, 1]], np.int32), start=np.asarray([7, 2 ** 32 - 2], np.uint32))
    assert got.tolist() == [7, 1] and skipped == 1
    got, skipped = TT.count_ref(3, TT.outside_ids(3))
    assert got.tolist() == [2, 0, 1] and skipped == 7
    for pattern in TT.PATTERNS:
        for rows in (1, 2, TT.BIG_VOCAB):
            ids = TT.draw_ids(pattern, 5000, rows)
            assert ids.dtype == np.int64 and ids.min() >= 0 and ids.max() < rows
            c, s = TT.count_ref(rows, ids)
            assert int(c.sum()) == 5000 and s == 0
    assert len(np.unique(TT.draw_ids("distinct", 3 * TT.SLOTS, TT.BIG_VOCAB))) == 3 * TT.SLOTS
    cong = np.unique(TT.draw_ids("congruent", 4000, TT.BIG_VOCAB))
    assert len(cong) == 3 * TT.PROBES and not (cong % TT.SLOTS).any()

    dim = 8
    stats = TA.source_stats(dim)
    idx = TA.table_index(dim, 300, "nan", "f16_bad")
    plain = TA.aggregate(stats, idx)
    ones = TT.weighted_aggregate(stats, idx, np.ones(300, np.uint32))
    zeros = TT.weighted_aggregate(stats, idx, np.zeros(300, np.uint32))
    assert ones["sum_sq"] == plain["sum_sq"] and zeros["sum_sq"] == 0.0
    for kind in TA.COMPACT:
        assert ones[kind] == plain[kind]
        assert zeros[kind]["sum_sq_err"] == 0.0
        assert {k: v for k, v in zeros[kind].items() if k != "sum_sq_err"} == {k: v for k, v in plain[kind].items() if k != "sum_sq_err"}
    c = TT.draw_counts(300, 1)
    assert c.dtype == np.uint32 and c[150] == 0xFFFFFFFF and c[100] == 0 and (c == 0).sum() > 50
    w = TT.weighted_aggregate(stats, idx, c)
    want = sum(float(c[r]) * float(stats["bf16"]["sse"][idx[r]]) for r in range(300))
    assert w["bf16"]["sum_sq_err"] == pytest.approx(want, rel=1e-12) and np.isfinite(w["sum_sq"])
    assert (w["rows"], w["rows_nonfinite"], w["first_nonfinite_row"]) == (plain["rows"], plain["rows_nonfinite"], plain["first_nonfinite_row"])
