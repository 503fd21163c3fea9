"""fcp_plan_table_rows / fcp_plan_traffic_bind / fcp_plan_traffic_count without a GPU: the three names in the header, in
lib.EXPORTS and in the loaded library; fcp_plan_table_rows on host-only plans; every refusal of bind and count that needs no
device, with its message; what the Python wrappers refuse; and the NumPy restatement of plan_traffic_cases on a hand-written
example.  (The kernel: tests/test_zz_gpu_plan_traffic.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plan_traffic_cases as PT
from recom_amd import lib as _lib
from recom_amd.ops import Plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
INV, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK
A = 1 << 20          # (pointers are never dereferenced on the host: plain numbers serve)


def _err():
    return _lib.load().fcp_last_error().decode()


def test_header_declares_and_library_exports_the_three_entries():
    text = open(HEADER).read()
    assert re.search(r"\bint fcp_plan_table_rows\(const fcp_plan_t \*plan, int64_t \*rows, int32_t capacity, int32_t \*n\);", text)
    assert re.search(r"\bint fcp_plan_traffic_bind\(fcp_plan_t \*plan, uint32_t \*const \*counts, int32_t n_counts, int64_t \*skipped\);", text)
    assert re.search(r"\bint fcp_plan_traffic_count\(fcp_plan_t \*plan, const fcp_process_args_t \*args\);", text)
    names = {"fcp_plan_table_rows", "fcp_plan_traffic_bind", "fcp_plan_traffic_count"}
    assert names <= set(_lib.EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in names)
    # the consequence the header states: the counts are fcp_table_count_ids' of the transformed ids
    assert "equal fcp_table_count_ids applied, per column, to the column's transformed ids" in " ".join(text.split()).replace("* ", "")


def test_table_rows_on_host_only_plans():
    L = _lib.load()
    spec, _inputs, _want, _skipped = PT.hand_example()
    plan = Plan(spec, host_only=True)
    assert plan.table_rows() == (6, 5)                          # table 1 is shared by vocab 5 and vocab 4: the largest
    assert list(plan.table_rows()) == PT.table_rows(spec)
    # an input no lookup column reads: -1 (three device inputs, the columns read 0 and 2)
    cols = [PT.gather_col(0, 11, 2), PT.gather_col(1, 7, 0, PT.IDS_I32), PT.gather_col(2, 13, 2)]
    spec3 = PT.gather_spec(cols, 3)
    plan3 = Plan(spec3, host_only=True)
    assert plan3.table_rows() == (7, -1, 13)
    # capacity smaller than n: only `capacity` values are written, *n is the number of device inputs all the same
    rows = (C.c_int64 * 3)(-7, -7, -7)
    n = C.c_int32(-1)
    assert L.fcp_plan_table_rows(plan3.handle, rows, 1, C.byref(n)) == OK
    assert list(rows) == [7, -7, -7] and n.value == 3
    assert L.fcp_plan_table_rows(plan3.handle, rows, 0, C.byref(n)) == OK and list(rows) == [7, -7, -7]
    # NULL pointers: either may be missing, or both
    assert L.fcp_plan_table_rows(plan3.handle, None, 3, C.byref(n)) == OK and n.value == 3
    assert L.fcp_plan_table_rows(plan3.handle, rows, 3, None) == OK and list(rows) == [7, -1, 13]
    assert L.fcp_plan_table_rows(plan3.handle, None, 0, None) == OK
    assert L.fcp_plan_table_rows(None, rows, 3, C.byref(n)) == INV and "null plan" in _err()
    # a plan without lookup columns or device inputs
    from recom_amd import synth
    m = synth.model_mixed(batch=5, vocab=97)
    full = Plan(m.spec, host_only=True)
    assert list(full.table_rows()) == PT.table_rows(m.spec) and len(full.table_rows()) == m.spec.n_device_inputs


def _bind(plan, counts, n_counts, skipped):
    L = _lib.load()
    arr = None if counts is None else (C.c_void_p * max(1, len(counts)))(*counts)
    status = L.fcp_plan_traffic_bind(plan.handle if plan is not None else None, arr, n_counts, C.c_void_p(skipped))
    return status, _err()


def test_bind_refusals_that_need_no_device():
    spec, _inputs, _want, _skipped = PT.hand_example()
    plan = Plan(spec, host_only=True)
    for args, word in (((None, -1, 0), "`n_counts`"), (([A, A], -2, 0), "`n_counts`"),
                       (([A], 1, 0), "`n_counts`"), (([A, A, A], 3, 0), "`n_counts`"),
                       ((None, 2, 0), "`counts`"),
                       (([A + 2, A], 2, 0), "`counts[0]`"), (([A, A + 1], 2, 0), "`counts[1]`"), (([0, A + 3], 2, A + 8), "`counts[1]`"),
                       (([A, A], 2, A + 4), "`skipped`"), (([0, 0], 2, A + 2), "`skipped`"), ((None, 0, A + 1), "`skipped`")):
        status, msg = _bind(plan, *args)
        assert status == INV and word in msg and msg.startswith("fcp_plan_traffic_bind:"), (args, status, msg)
    # the order: n_counts, null counts, alignment of counts, alignment of skipped
    assert "`n_counts`" in _bind(plan, None, 5, A + 1)[1]
    assert "`counts`" in _bind(plan, None, 2, A + 1)[1]
    assert "`counts[0]`" in _bind(plan, [A + 1, A + 1], 2, A + 1)[1]
    assert "device inputs (2)" in _bind(plan, [A], 1, 0)[1]
    status, msg = _bind(None, [A, A], 2, 0)
    assert status == INV and "null plan" in msg
    # an unbind is FCP_OK on any plan: n_counts == 0, or every entry NULL
    assert _bind(plan, None, 0, 0)[0] == OK
    assert _bind(plan, [0, 0], 2, 0)[0] == OK
    assert _bind(plan, [0, 0], 2, A + 8)[0] == OK
    # a real bind needs the device a host-only plan does not have
    for counts in ([A, A], [0, A + 4], [A + 8, 0]):
        status, msg = _bind(plan, counts, 2, A + 16)
        assert status == NODEV and "host-only" in msg, (counts, status, msg)


def _args(offsets=None, shapes=None, symbols=None, blob=0, nbytes=0):
    keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (offsets, shapes, symbols)]
    p = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep]
    return _lib.ProcessArgs(blob or None, nbytes, p[0], p[1], None, None, p[2], None), keep


def test_count_refusals_that_need_no_device():
    L = _lib.load()
    spec, inputs, _want, _skipped = PT.hand_example()
    plan = Plan(spec, host_only=True)
    a, _keep = _args([0, 40, 60], [5, 5, 5])
    assert L.fcp_plan_traffic_count(None, C.byref(a)) == INV and "null plan / args" in _err()
    assert L.fcp_plan_traffic_count(plan.handle, None) == INV and "null plan / args" in _err()
    for offs, shps in ((None, [5, 5, 5]), ([0, 40, 60], None), (None, None)):
        b, _k = _args(offs, shps)
        assert L.fcp_plan_traffic_count(plan.handle, C.byref(b)) == INV and "null offsets / shapes" in _err()
    # count without bind: FCP_ERR_INVALID_ARGUMENT, and the message names the entry that is missing
    assert L.fcp_plan_traffic_count(plan.handle, C.byref(a)) == INV
    assert _err().startswith("fcp_plan_traffic_count:") and "`fcp_plan_traffic_bind`" in _err()
    # after an unbind as well
    assert _bind(plan, [0, 0], 2, 0)[0] == OK
    assert L.fcp_plan_traffic_count(plan.handle, C.byref(a)) == INV and "`fcp_plan_traffic_bind`" in _err()
    # a plan with symbols wants them before anything else is looked at
    bags = Plan(PT.bag_spec(2, 50, [0, 0]), host_only=True)
    c, _k = _args([0, 8, 16, 24], [1, 2, 1, 2])
    assert L.fcp_plan_traffic_count(bags.handle, C.byref(c)) == INV and "plan needs symbols" in _err()


def test_python_wrappers_refuse_what_they_can_see():
    import torch
    from recom_amd import tables
    spec, _inputs, _want, _skipped = PT.hand_example()
    counts = tables.new_plan_counts(spec, "cpu")
    assert [None if c is None else tuple(c.shape) for c in counts] == [(6,), (5,)] and not any(c.numpy().any() for c in counts)
    cols = [PT.gather_col(0, 11, 2), PT.gather_col(1, 7, 0, PT.IDS_I32)]
    spec3 = PT.gather_spec(cols, 3)
    plan3 = Plan(spec3, host_only=True)
    for made in (tables.new_plan_counts(spec3, "cpu"), tables.new_plan_counts(plan3, "cpu")):      # a spec or a plan: the same
        assert [None if c is None else tuple(c.shape) for c in made] == [(7,), None, (11,)]
    plan = Plan(spec, host_only=True)
    with pytest.raises(ValueError, match="counts names 1 inputs, the plan has 2 device inputs"):
        plan.traffic_bind([counts[0]])
    with pytest.raises(ValueError, match=r"counts\[1\] has 6 cells, the plan's table 1 has 5 rows"):
        plan.traffic_bind([counts[0], counts[0]])
    with pytest.raises(ValueError, match="uint32"):
        plan.traffic_bind([torch.zeros((6,), dtype=torch.int64), None])
    with pytest.raises(ValueError, match=r"counts\[0\] is on cpu"):
        plan.traffic_bind(counts)
    with pytest.raises(ValueError, match="skipped is an int64 tensor of one element"):
        plan.traffic_bind([None, None], skipped=torch.zeros((2,), dtype=torch.int64))
    plan.traffic_bind(None)                                   # an unbind needs no device
    plan.traffic_bind([None, None])
    with pytest.raises(_lib.FcpError, match="fcp_plan_traffic_bind"):
        plan.traffic_count(None, [0, 40, 60], [5, 5, 5], stream=0)


def test_expected_counts_on_a_hand_written_example():
    """one filtered id, out-of-vocab ids (one of them inside the shared table but outside ITS column's vocab), one shared
    table; int32 ids widen with their sign; a start value is added to, modulo 2^32"""
    spec, inputs, want, skipped = PT.hand_example()
    got, got_skipped = PT.expected_counts(spec, inputs)
    assert got_skipped == skipped == 3 and PT.n_filtered(spec.columns[0], inputs) == 1
    assert all(g.dtype == np.uint32 and np.array_equal(g, w) for g, w in zip(got, want))
    start = [np.asarray([0xFFFFFFFF] * 6, np.uint32), None]
    again, _s = PT.expected_counts(spec, inputs, start=start)
    assert again[0].tolist() == [0xFFFFFFFF, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0] and np.array_equal(again[1], want[1])
    # the pieces: SELECT substitutes (inside and outside the vocab), hash in front, bucketize, the unsigned compare
    import dataclasses
    sel = dataclasses.replace(spec.columns[2], xform_mode=PT.XFORM_SELECT, xform_lo=(0,), xform_hi=(3,), xform_substitute=-5)
    assert PT.lookup_ids(sel, inputs).tolist() == [3, -5, 0, 3, 3]
    hashed = dataclasses.replace(spec.columns[2], hash_buckets=97)
    import fcp_oracle as O
    assert PT.lookup_ids(hashed, inputs).tolist() == [O.np_fingerprint64(str(v).encode()) % 97 for v in (3, 4, 0, 3, 3)]
    bkt = PT.gather_col(0, 4, 0, PT.IDS_F32_BUCKETIZE, boundaries=np.asarray([0.0, 1.0, 2.0], np.float32))
    assert PT.lookup_ids(bkt, [np.asarray([-1.0, 0.0, 0.5, 2.0, 9.0], np.float32)]).tolist() == [0, 1, 1, 3, 3]
    one = PT.gather_spec([PT.gather_col(0, 5, 0)], 1)
    got, s = PT.expected_counts(one, [np.asarray([-1, 5, 2 ** 32 + 1, PT.INT64_MIN, 4, 4], np.int64)])
    assert got[0].tolist() == [0, 0, 0, 0, 2] and s == 4
