"""Per-input table formats (FCP_FLAG_TABLES_PER_INPUT) without a GPU: the ABI's vocabulary, host-only plans (acceptance, the
invalid arguments, the four refusals, canonicalisation of uniform kinds, fcp_plan_table_kinds, table bytes, the placement
gate), plan files of version 8, the code object of fcp_tables_mixed.hip, and the conditions the GPU cells rely on (the layout
of the plans; that no kernel which picks a neighbour's loader can pass them).  Cases: tests/table_mixed_cases.py."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import table_mixed_cases as M
from recom_amd import lib as _lib
from recom_amd import placement, plan_io, synth
from recom_amd.ops import Plan
from recom_amd.plan import (FLAG_OUT_BF16, FLAG_TABLES_BF16, FLAG_TABLES_F16, FLAG_TABLES_PER_INPUT, FLAG_TABLES_Q8, PlanSpec,
                            Tables16Unsupported, TablesMixedUnsupported, TablesQ8Unsupported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {"f32": 0, "bf16": 1, "f16": 2, "q8": 3}


# ---- vocabulary -----------------------------------------------------------------------------------------------------------
def test_constants_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    assert re.search(r"FCP_FLAG_TABLES_PER_INPUT = 1u << 6\b", text)
    assert re.search(r"^enum \{ FCP_TAB_MIXED = 255 \};$", text, re.M)
    assert re.search(r"FCP_LAUNCH_DENSE_TABMIX = 14, FCP_LAUNCH_RAGGED_TABMIX = 15, FCP_LAUNCH_HYBRID_TABMIX = 16", text)
    assert re.search(r"#define FCP_ABI_VERSION 2\b", text)
    assert FLAG_TABLES_PER_INPUT == _lib.FLAG_TABLES_PER_INPUT == 64 and _lib.TAB_MIXED == 255
    assert [_lib.LAUNCH_KERNELS[k] for k in (14, 15, 16)] == ["dense_tabmix", "ragged_tabmix", "hybrid_tabmix"]
    assert _lib.PLAN_TABLE_DTYPES[255] == "mixed"


def test_mixed_is_no_row_format():
    """fcp_table_row_bytes and fcp_table_convert refuse FCP_TAB_MIXED like any other unknown kind."""
    L = _lib.load()
    assert L.fcp_table_row_bytes(_lib.TAB_MIXED, 8) == -1
    assert _lib.TAB_MIXED not in _lib.ALL_TABLE_DTYPES and "mixed" not in _lib.TABLE_KINDS


def test_the_extension_record_keeps_its_size_and_earlier_offsets():
    E = _lib.ColumnExt
    assert C.sizeof(E) == 72
    want = {"seg_map_n": 0, "seg_map_sym": 4, "seg_map_sym_slot": 8, "weights_input1": 12, "seg_map_mul": 16, "seg_map_div": 48,
            "table_kind1": 56, "reserved0": 60, "reserved1": 64}
    assert {n: getattr(E, n).offset for n, _ in E._fields_} == want
    assert E.reserved1.size == 8 and E.table_kind1.size == 4
    text = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    body = re.search(r"typedef struct fcp_column_ext \{(.*?)\} fcp_column_ext_t;", text, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|int64_t) (\w+)(?:\[(\w+)\])?;", body, re.M)
    assert [f[1] for f in fields] == ["seg_map_n", "seg_map_sym", "seg_map_sym_slot", "weights_input1", "seg_map_mul", "seg_map_div",
                                      "table_kind1", "reserved0", "reserved1"]
    assert fields[-1] == ("int64_t", "reserved1", "1") and fields[-3][0] == fields[-2][0] == "int32_t"


# ---- host-only plans ------------------------------------------------------------------------------------------------------
def _create_raw(spec: PlanSpec, kinds1=None, flags=FLAG_TABLES_PER_INPUT, with_ext=True):
    """fcp_plan_create_ex with these flag bits and these table_kind1 values per column, past the Python mirror: (status,
    message, table dtype, table kinds, table bytes)."""
    L = _lib.load()
    base = Plan.__new__(Plan)                        # descriptor arrays as Plan builds them, created by hand below
    cols = (_lib.ColumnDesc * spec.n_columns)()
    for k, c in enumerate(spec.columns):
        cols[k] = _lib.ColumnDesc(c.form, c.combiner, c.dim, c.id_source, c.vocab, c.table_input, c.ids_input, c.seg_input, c.seg_kind,
                                  c.seg_stride, c.rows_source, c.rows_arg, 0, None, c.concat_group, c.concat_slot, c.xform_mode, 0, None,
                                  None, 0, 0)
    ranks = np.asarray(spec.host_input_ranks, np.int32)
    esz = np.asarray(spec.host_input_elem_sizes, np.int32)
    desc = _lib.PlanDesc(_lib.FCP_ABI_VERSION, spec.n_columns, cols, len(ranks), ranks.ctypes.data_as(C.POINTER(C.c_int32)),
                         esz.ctypes.data_as(C.POINTER(C.c_int32)), spec.n_device_inputs, spec.n_groups, spec.n_symbols, spec.layout, 0,
                         spec.shard_rank, spec.shard_world, spec.flags | flags | _lib.FLAG_HOST_ONLY)
    ext = None
    if with_ext:
        ext = (_lib.ColumnExt * spec.n_columns)()
        for k, c in enumerate(spec.columns):
            ext[k].weights_input1 = int(c.weights_input) + 1
            ext[k].table_kind1 = 0 if kinds1 is None else int(kinds1[k])
    h = C.c_void_p()
    rc = L.fcp_plan_create_ex(C.byref(desc), ext, C.byref(h))
    if rc != _lib.FCP_OK:
        return rc, L.fcp_last_error().decode(), None, None, None
    base._L, base.handle, base._keep = L, h, []
    out = (rc, "", base.table_dtype(), base.table_dtypes(), base.table_bytes())
    base.close()
    return out


def _kinds1(spec, names):
    """table_kind1 per column from one name per device input"""
    return [1 + KIND[names[c.table_input]] if c.form in M.LOOKUP else 0 for c in spec.columns]


def test_a_mixed_plan_is_accepted_and_names_its_kinds():
    spec = M.small_mixed_spec()
    rc, _, dtype, kinds, nbytes = _create_raw(spec, _kinds1(spec, M.SMALL_KINDS))
    assert rc == _lib.FCP_OK and dtype == "mixed" and kinds == M.SMALL_KINDS
    want = [M.VOCAB * 4 * 4, M.VOCAB * 8 * 2, M.VOCAB * (4 + 8)]
    assert nbytes == (sum(want), max(want))
    # through PlanSpec / Plan
    s = spec.with_table_dtypes(M.SMALL_KINDS)
    assert s.table_dtypes == M.SMALL_KINDS and s.table_dtype == "f32" and s.plan_flags() & FLAG_TABLES_PER_INPUT and s.mixed_tables()
    p = Plan(s, host_only=True)
    assert p.table_dtype() == "mixed" and p.table_dtypes() == M.SMALL_KINDS and p.table_bytes() == (sum(want), max(want))
    assert int(placement.table_bytes(s).sum()) == sum(want)
    assert s.to_dict()["table_dtypes"] == M.SMALL_KINDS and "table_dtypes" not in spec.to_dict()
    # the output side is the float32 twin's
    p32 = Plan(spec, host_only=True)
    assert p32.table_dtypes() == ("f32", "f32", "f32")
    shapes, sym = [5, 5, 9, 6, 9], [5]
    assert p.arena_bytes(shapes, sym) == p32.arena_bytes(shapes, sym) and p.group_width(0) == p32.group_width(0)


def test_an_input_no_lookup_column_reads_has_no_kind():
    spec = M.small_mixed_spec()
    spec = dataclasses.replace(spec, n_device_inputs=5)
    rc, _, dtype, kinds, _ = _create_raw(spec, _kinds1(spec, M.SMALL_KINDS))
    assert rc == _lib.FCP_OK and kinds == M.SMALL_KINDS + ("-", "-")
    s = spec.with_table_dtypes(M.SMALL_KINDS + ("q8", "f16"))          # names of unread inputs are dropped
    assert s.table_dtypes == M.SMALL_KINDS + ("-", "-")
    assert Plan(s, host_only=True).table_dtypes() == s.table_dtypes


def test_invalid_arguments():
    spec = M.small_mixed_spec()
    mixed = _kinds1(spec, M.SMALL_KINDS)
    # together with a plan-wide table bit
    for bit in (FLAG_TABLES_BF16, FLAG_TABLES_F16, FLAG_TABLES_Q8):
        rc, msg, *_ = _create_raw(spec, mixed, flags=FLAG_TABLES_PER_INPUT | bit)
        assert rc == _lib.FCP_ERR_INVALID_ARGUMENT and "exclude" in msg, msg
        with pytest.raises(ValueError, match="exclude"):
            dataclasses.replace(spec.with_table_dtypes(M.SMALL_KINDS), flags=bit).validate()
    with pytest.raises(ValueError, match="exclude"):
        dataclasses.replace(spec.with_table_dtypes(M.SMALL_KINDS), table_dtype="bf16").validate()
    # columns that share a table_input name different kinds: both columns are named
    shared = dataclasses.replace(spec, columns=[spec.columns[0], dataclasses.replace(spec.columns[1], table_input=0, dim=4), spec.columns[2]])
    rc, msg, *_ = _create_raw(shared, [1, 2, 4])
    assert rc == _lib.FCP_ERR_INVALID_ARGUMENT and "columns 0 and 1" in msg and "table input 0" in msg, msg
    assert _create_raw(shared, [2, 2, 4])[0] == _lib.FCP_OK
    assert _create_raw(shared, [0, 1, 4])[0] == _lib.FCP_OK               # 0 means float32, as 1 + FCP_TAB_F32 does
    # a column without a table carries 0
    plan = M.build_plan(4, "ragged")
    for form in (4, 5):
        k = [i for i, c in enumerate(plan.spec32.columns) if c.form == form][0]
        kinds1 = _kinds1(plan.spec32, plan.kinds)
        assert _create_raw(plan.spec32, kinds1)[0] == _lib.FCP_OK
        kinds1[k] = 2
        rc, msg, *_ = _create_raw(plan.spec32, kinds1)
        assert rc == _lib.FCP_ERR_INVALID_ARGUMENT and f"column {k}" in msg and "without a table" in msg, msg
    # a value that is no 1 + FCP_TAB_*
    for bad in (5, -1, 256):
        rc, msg, *_ = _create_raw(spec, [bad, 1, 1])
        assert rc == _lib.FCP_ERR_INVALID_ARGUMENT and "table_kind1" in msg
    # the Python mirror
    with pytest.raises(ValueError, match="names 2 inputs"):
        spec.with_table_dtypes(("f32", "q8"))
    with pytest.raises(ValueError, match="q4"):
        spec.with_table_dtypes(("f32", "q4", "q8"))
    with pytest.raises(ValueError, match="table_dtypes"):
        dataclasses.replace(spec, table_dtypes=("f32", "-", "q8")).validate()


def test_without_the_flag_the_field_is_not_read_and_null_ext_means_float32():
    spec = M.small_mixed_spec()
    f32 = Plan(spec, host_only=True).table_bytes()
    rc, _, dtype, kinds, nbytes = _create_raw(spec, [4, 4, 4], flags=0)
    assert (rc, dtype, kinds, nbytes) == (_lib.FCP_OK, "f32", ("f32",) * 3, f32)
    rc, _, dtype, kinds, nbytes = _create_raw(spec, [77, -3, 9], flags=FLAG_TABLES_Q8)        # garbage in the field: never looked at
    assert (rc, dtype, kinds) == (_lib.FCP_OK, "q8", ("q8",) * 3)
    rc, _, dtype, kinds, nbytes = _create_raw(spec, with_ext=False)
    assert (rc, dtype, kinds, nbytes) == (_lib.FCP_OK, "f32", ("f32",) * 3, f32)


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16", "q8"])
def test_uniform_kinds_are_the_plan_wide_plan(kind, tmp_path):
    """All tables of one kind under the flag: fcp_plan_table_dtype, the bytes and the plan file are the plan-wide plan's."""
    spec = M.small_mixed_spec()
    wide = Plan(spec.with_table_dtype(kind), host_only=True)
    rc, _, dtype, kinds, nbytes = _create_raw(spec, _kinds1(spec, (kind,) * 3))
    assert (rc, dtype, kinds, nbytes) == (_lib.FCP_OK, kind, (kind,) * 3, wide.table_bytes())
    # PlanSpec: a uniform tuple IS table_dtype
    s = spec.with_table_dtypes((kind,) * 3)
    assert s.table_dtypes is None and s.table_dtype == kind and not s.plan_flags() & FLAG_TABLES_PER_INPUT
    # a spec that keeps the uniform tuple (set directly) goes through the library's flag, and still writes the old file
    raw = dataclasses.replace(spec, table_dtypes=(kind,) * 3)
    raw.validate()
    assert raw.plan_flags() & FLAG_TABLES_PER_INPUT and not raw.mixed_tables()
    p = Plan(raw, host_only=True)
    assert p.table_dtype() == kind and p.table_bytes() == wide.table_bytes()
    a, b = tmp_path / "a.plan", tmp_path / "b.plan"
    plan_io.save_plan(raw, str(a))
    plan_io.save_plan(spec.with_table_dtype(kind), str(b))
    assert a.read_bytes() == b.read_bytes() and a.read_text().startswith("fcp_plan 7\n" if kind != "f32" else "fcp_plan 2\n")
    # the plan-wide refusals, by THEIR names
    if kind != "f32":
        cls = TablesQ8Unsupported if kind == "q8" else Tables16Unsupported
        with pytest.raises(cls, match="narrow output"):
            dataclasses.replace(raw, out_dtype="bf16").validate()
        rc, msg, *_ = _create_raw(spec, _kinds1(spec, (kind,) * 3), flags=FLAG_TABLES_PER_INPUT | FLAG_OUT_BF16)
        assert rc == _lib.FCP_ERR_UNSUPPORTED and ("8-bit tables" if kind == "q8" else "16-bit tables") in msg


@pytest.mark.parametrize("why", sorted(M.refused_specs()))
def test_unsupported_plan_kinds_are_refused_by_name(why):
    spec, extra, word = M.refused_specs()[why]
    Plan(spec, host_only=True)                                          # the float32-table plan is fine
    rc, msg, *_ = _create_raw(spec, _kinds1(spec, M.SMALL_KINDS), flags=FLAG_TABLES_PER_INPUT | extra)
    assert rc == _lib.FCP_ERR_UNSUPPORTED and word in msg and "per-input table formats" in msg, (rc, msg)
    with pytest.raises(TablesMixedUnsupported, match=re.escape(word)) as e:
        dataclasses.replace(spec, flags=spec.flags | extra).with_table_dtypes(M.SMALL_KINDS).validate()
    # the same words
    assert str(e.value) in msg


def test_table_bytes_are_the_per_kind_sum_and_the_placement_gate_sees_them():
    """BASELINE's SHARD (4000 columns x 1 M rows, dims 8 / 16 / 32 / 64) with kinds by dim: 1000 x 1 M x (32 + 32 + 64 + 72)
    = 200 GB fits one 288 GB device where 480 GB of float32 tables do not.  And the narrow column the issue is about: a
    dim-1 table costs 4 bytes per row as float32 beside q8 tables, not 9."""
    f32 = synth.model_s2(columns=4000, vocab=1_000_000, batch=4).spec
    mixed = synth.model_s2(columns=4000, vocab=1_000_000, batch=4, table_dtypes=M.S2_KINDS).spec
    assert mixed.mixed_tables() and mixed.table_dtypes[:4] == ("f32", "bf16", "f16", "q8")
    want = 1000 * 10 ** 6 * (8 * 4 + 16 * 2 + 32 * 2 + 64 + 8)
    assert int(placement.table_bytes(mixed).sum()) == want == 200 * 10 ** 9
    p = Plan(mixed, host_only=True)
    assert p.table_bytes() == (want, 10 ** 6 * 72) and p.table_dtype() == "mixed"
    assert placement.decide_placement(f32, 8, hbm_bytes=288 * 10 ** 9).mode != placement.REPLICATE
    assert placement.decide_placement(mixed, 8, hbm_bytes=288 * 10 ** 9).mode == placement.REPLICATE
    L = _lib.load()
    tb = np.ascontiguousarray(placement.table_bytes(mixed), np.int64)
    out = _lib.Placement()
    _lib.check(L.fcp_placement_decide(tb.ctypes.data, len(tb), 288 * 10 ** 9, placement.DEFAULT_RESERVE_BYTES, 8, placement.ROW_SHARD,
                                      C.byref(out)), "fcp_placement_decide")
    assert out.mode == placement.REPLICATE
    wide = synth.model_s2(columns=8, vocab=1000, batch=4, dims=(1, 64), table_dtypes={64: "q8"})
    assert wide.spec.table_dtypes == ("f32", "q8") * 4
    assert Plan(wide.spec, host_only=True).table_bytes()[0] == 4 * 1000 * (4 + 72) == wide.table_bytes()
    assert Plan(wide.spec.with_table_dtypes(None).with_table_dtype("q8"), host_only=True).table_bytes()[0] == 4 * 1000 * (9 + 72)


def test_synth_produces_each_table_in_its_kind():
    m = synth.model_s2(columns=8, vocab=50, batch=4, table_dtypes=M.S2_KINDS)
    tabs = m.numpy_tables()
    assert [(t.dtype, t.shape) for t in tabs[:4]] == [(np.dtype(np.float32), (50, 8)), (np.dtype(np.uint16), (50, 16)),
                                                      (np.dtype(np.uint16), (50, 32)), (np.dtype(np.uint8), (50, 72))]
    assert m.table_bytes() == 2 * 50 * (32 + 32 + 64 + 72)
    uniform = synth.model_s2(columns=8, vocab=50, batch=4, table_dtypes={d: "bf16" for d in (8, 16, 32, 64)})
    assert uniform.spec.table_dtypes is None and uniform.spec.table_dtype == "bf16"


# ---- plan files -----------------------------------------------------------------------------------------------------------
def _lib_from_file(path, flags=0):
    L = _lib.load()
    h = C.c_void_p()
    rc = L.fcp_plan_create_from_file(str(path).encode(), 0, flags | _lib.FLAG_HOST_ONLY, C.byref(h))
    dt = None
    if rc == _lib.FCP_OK:
        v = C.c_int32(-1)
        assert L.fcp_plan_table_dtype(h, C.byref(v)) == _lib.FCP_OK
        dt = _lib.PLAN_TABLE_DTYPES[v.value]
        L.fcp_plan_destroy(h)
    return rc, dt


def test_version_8_round_trips_through_both_parsers(tmp_path):
    for spec32, kinds in ((M.small_mixed_spec(), M.SMALL_KINDS), (M.build_plan(2, "ragged").spec32, M.build_plan(2, "ragged").kinds),
                          (dataclasses.replace(M.small_mixed_spec(), n_device_inputs=4), M.SMALL_KINDS + ("-",))):
        s = spec32.with_table_dtypes(kinds)
        path = tmp_path / "mixed.plan"
        plan_io.save_plan(s, str(path))
        lines = path.read_text().split("\n")
        assert lines[0] == "fcp_plan 8" and lines[1] == f"table_dtypes {len(kinds)} " + " ".join(kinds) and lines[2].startswith("layout ")
        back = plan_io.load_plan(str(path))
        assert back.table_dtypes == tuple(kinds) and back.table_dtype == "f32" and back.out_dtype == "f32"
        again = tmp_path / "again.plan"
        plan_io.save_plan(back, str(again))
        assert again.read_bytes() == path.read_bytes()
        assert _lib_from_file(path) == (_lib.FCP_OK, "mixed")
        p = Plan.from_file(str(path), host_only=True)
        assert p.table_dtype() == "mixed" and p.table_dtypes() == tuple(kinds) == p.spec.table_dtypes
        assert p.table_bytes() == Plan(s, host_only=True).table_bytes()
        # plan-wide table bits on a version-8 file; narrow output on top of it is the refused combination
        for bit in (FLAG_TABLES_BF16, FLAG_TABLES_F16, FLAG_TABLES_Q8):
            assert _lib_from_file(path, bit)[0] == _lib.FCP_ERR_INVALID_ARGUMENT
        assert _lib_from_file(path, FLAG_TABLES_PER_INPUT) == (_lib.FCP_OK, "mixed")
        assert _lib_from_file(path, FLAG_OUT_BF16)[0] == _lib.FCP_ERR_UNSUPPORTED
        # files of version <= 7 are what they were
        plan_io.save_plan(spec32, str(path))
        assert "table_dtype" not in path.read_text() and _lib_from_file(path) == (_lib.FCP_OK, "f32")


def test_malformed_table_dtypes_lines_are_refused_by_both_parsers(tmp_path):
    spec = M.small_mixed_spec()
    good = tmp_path / "good.plan"
    plan_io.save_plan(spec.with_table_dtypes(M.SMALL_KINDS), str(good))
    lines = good.read_text().split("\n")
    assert lines[1] == "table_dtypes 3 f32 bf16 q8"
    old = tmp_path / "old.plan"
    plan_io.save_plan(spec, str(old))
    old_lines = old.read_text().split("\n")
    v7 = tmp_path / "v7.plan"
    plan_io.save_plan(spec.with_table_dtype("q8"), str(v7))
    v7_lines = v7.read_text().split("\n")
    variants = {
        "a name too few": [lines[0], "table_dtypes 3 f32 bf16"] + lines[2:],
        "a name too many": [lines[0], "table_dtypes 3 f32 bf16 q8 q8"] + lines[2:],
        "a count that is not the plan's": [lines[0], "table_dtypes 2 f32 bf16"] + lines[2:],
        "a count larger than the plan's": [lines[0], "table_dtypes 4 f32 bf16 q8 f16"] + lines[2:],
        "no count": [lines[0], "table_dtypes f32 bf16 q8"] + lines[2:],
        "unknown name": [lines[0], "table_dtypes 3 f32 q4 q8"] + lines[2:],
        "no name for a table a column reads": [lines[0], "table_dtypes 3 f32 - q8"] + lines[2:],
        "version 8 without the line": [lines[0]] + lines[2:],
        "version 8 with the version 7 line": [lines[0], "table_dtype q8"] + lines[2:],
        "line after layout": [lines[0], lines[2], lines[1]] + lines[3:],
        "repeated line": lines[:2] + [lines[1]] + lines[2:],
        "repeated at the end": lines[:-1] + [lines[1], ""],
        "table_dtype behind it": lines[:2] + ["table_dtype q8"] + lines[2:],
        "line in a version <= 5 file": [old_lines[0], lines[1]] + old_lines[1:],
        "line at the end of a version <= 5 file": old_lines[:-1] + [lines[1], ""],
        "line in a version 7 file, in table_dtype's place": [v7_lines[0], lines[1]] + v7_lines[2:],
        "line in a version 7 file, behind table_dtype": v7_lines[:2] + [lines[1]] + v7_lines[2:],
        "one kind in a version 8 file": [lines[0], "table_dtypes 3 q8 q8 q8"] + lines[2:],
        "version 9": ["fcp_plan 9"] + lines[1:],
    }
    for what, text in variants.items():
        path = tmp_path / "bad.plan"
        path.write_text("\n".join(text))
        assert _lib_from_file(path)[0] == _lib.FCP_ERR_INVALID_ARGUMENT, what
        with pytest.raises((ValueError, AssertionError)):
            plan_io.load_plan(str(path))
    assert _lib_from_file(good) == (_lib.FCP_OK, "mixed")


# ---- the plans of the GPU cells ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", M.FLAVOURS)
@pytest.mark.parametrize("vec", M.VECS)
def test_layout_of_the_gpu_plans(vec, flavour):
    """What the GPU cells rely on: V is the plan's vec, 24..32 lookup columns on as many device inputs (one shared), kinds
    cycling in concat order, at least two spans, every span with all four kinds, a column across the span boundary, odd q8
    dims at V = 1, and the flavour's forms."""
    plan = M.build_plan(vec, flavour)
    spec = plan.spec32
    lookups = [c for c in spec.columns if c.form in M.LOOKUP]
    assert 24 <= len(lookups) <= 32 and len(plan.kinds) == len(lookups) - 1 == spec.n_device_inputs
    assert [plan.kinds[c.table_input] for c in lookups] == [M.KINDS[i % 4] for i in range(len(lookups))]
    assert all(c.dim % vec == 0 and c.vocab == M.VOCAB for c in lookups) and any(c.dim % (2 * vec) for c in spec.columns)
    spans = M.span_kinds(plan)
    assert len(spans) >= 2 and all(s == set(M.KINDS) for s in spans), spans
    assert M.straddlers(plan)
    a, b = plan.shared
    assert spec.columns[a].table_input == spec.columns[b].table_input and plan.kinds[spec.columns[a].table_input] == "q8"
    if vec == 1:
        q8_dims = {c.dim for c in lookups if plan.kinds[c.table_input] == "q8"}
        assert {1, 5, 7, 9} <= q8_dims              # rows of 9, 13, 15 and 17 bytes: scale and bias at any byte
    forms = {c.form for c in spec.columns}
    assert forms == {"dense": {1, 4}, "ragged": {1, 2, 3, 4, 5}, "hybrid": {1, 2, 3, 4, 5}}[flavour]
    if flavour != "dense":
        assert any(c.xform_mode for c in spec.columns) and {c.combiner for c in spec.columns if c.form == 2} == {1, 2}
    p = Plan(plan.spec, host_only=True)
    assert p.table_dtype() == "mixed" and p.table_dtypes() == plan.kinds
    tabs, dec = M.plan_tables(vec, flavour)
    dims = {c.table_input: c.dim for c in lookups}
    assert p.table_bytes()[0] == sum(t.nbytes for t in tabs) == sum(M.VOCAB * M.row_bytes(k, dims[t]) for t, k in enumerate(plan.kinds))
    # the special values are in the decoded tables: -0.0, subnormals, both infinities, NaN
    flat = np.concatenate([d.ravel() for d in dec])
    assert (flat.view(np.uint32) == 0x80000000).any() and ((flat != 0) & (np.abs(flat) < 2.0 ** -126)).any()
    assert (flat == np.inf).any() and (flat == -np.inf).any() and np.isnan(flat).any()


def test_the_cells_reach_all_21_instantiations():
    reached = {(f, v, r if f != "ragged" else 0) for v, f, _b, r, _w in M.cells()}
    assert reached == set(M.kernel_names().values()) and len(reached) == 21
    for v, f, b, r, _w in M.cells():
        if f != "ragged":
            assert r == (4 if b >= 64 else 2 if b >= 32 else 1)           # how the library picks rows per wave
    # ids 0, vocab - 1, -1 and vocab in every plan's requests; a bag beyond a wave's tile in every ragged one
    for v, f, b in M.requests_of_cells():
        plan = M.build_plan(v, f)
        inputs, _ = M.request(v, f, b)
        ids = np.concatenate([np.asarray(inputs[c.ids_input]).ravel() for c in plan.spec32.columns if c.form in M.LOOKUP])
        if b >= 5:
            assert {0, M.VOCAB - 1, -1, M.VOCAB} <= set(ids.tolist()), (v, f, b)
        if f != "dense":
            lens = [np.diff(inputs[c.seg_input]).max() for c in plan.spec32.columns if c.form == 2]
            assert max(lens) == M.LONG_BAG > 384 and sorted(lens)[-2] <= 10


def _differs(a, b):
    nan = np.isnan(a) | np.isnan(b)
    return np.where(nan, np.isnan(a) != np.isnan(b), a.view(np.uint32) != b.view(np.uint32))


@pytest.mark.parametrize("vec,flavour,batch", M.requests_of_cells(), ids=[f"{f}-V{v}-B{b}" for v, f, b in M.requests_of_cells()])
def test_a_neighbours_loader_cannot_pass(oracle, vec, flavour, batch):
    """For every lookup column: the expectation under the column's true kind differs from the expectation under each other
    kind — the same table bytes read by that kind's loader, where that stays inside the table — on at least half of the
    output elements a table element reaches (found with tables of ones: an element no table element reaches is 0)."""
    plan = M.build_plan(vec, flavour)
    spec = plan.spec32
    tabs, dec = M.plan_tables(vec, flavour)
    want, _ = M.expectation(vec, flavour, batch)
    reach, _ = M.run_oracle(vec, flavour, batch, [np.ones_like(d) for d in dec])
    offs = spec.column_offsets()
    dims = {c.table_input: c.dim for c in spec.columns if c.form in M.LOOKUP}
    checked = 0
    for shift in (1, 2, 3):
        others = [M.KINDS[(M.KINDS.index(k) + shift) % 4] for k in plan.kinds]
        alt = [M.reinterpret(t, k, o, dims[i]) for i, (t, k, o) in enumerate(zip(tabs, plan.kinds, others))]
        got, _ = M.run_oracle(vec, flavour, batch, [d if a is None else a for d, a in zip(dec, alt)])
        for k, c in enumerate(spec.columns):
            if c.form not in M.LOOKUP or alt[c.table_input] is None:
                continue
            sl = slice(offs[k], offs[k] + c.dim)
            reached = reach[:, sl] != 0
            if not reached.any():                    # (batch 1: a column whose only id is out of the vocabulary)
                continue
            frac = float(_differs(want[:, sl], got[:, sl])[reached].mean())
            assert frac >= 0.5, (vec, flavour, batch, "column", k, plan.kinds[c.table_input], "read as", others[c.table_input], frac)
            checked += 1
    assert checked >= 24        # (most columns have at least one other kind whose rows fit inside their bytes)


# ---- code object ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tabmix_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    out, procs = {}, {}
    for src in ("fcp_tables_mixed", "fcp_kernels"):
        asm = tmp_path_factory.mktemp("asm") / f"{src}.s"
        procs[src] = (asm, subprocess.Popen([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                                             os.path.join(ROOT, "recom_amd", "csrc", f"{src}.hip"), "-o", str(asm)],
                                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for src, (asm, proc) in procs.items():
        _, err = proc.communicate()
        assert proc.returncode == 0, err[-2000:]
        out[src] = asm.read_text()
    return out


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}


def _field(desc, name):
    return int(re.search(r"\.amdhsa_" + name + r" (\d+)", desc).group(1))


def test_code_object_of_the_tabmix_kernels(tabmix_asm):
    """The 21 kernels exist by name, use no scratch and exactly their float32 twins' LDS; VGPR counts are printed, not
    asserted (DESIGN.md §3 quotes them)."""
    text = tabmix_asm["fcp_tables_mixed"]
    kernels = _kernels(text)
    names = M.kernel_names()
    assert len(names) == 21
    unmatched = [k for k in kernels if sum(frag in k for frag in names) != 1]
    assert not unmatched and len(kernels) == len(names), (unmatched, len(kernels))
    f32 = _kernels(tabmix_asm["fcp_kernels"])
    for name, desc in sorted(kernels.items()):
        (kernel, v, r), = [kv for frag, kv in names.items() if frag in name]
        twin = f"fcp_{kernel}_kernelILi{v}E" + (f"Li{r}E" if kernel != "ragged" else "") + "Lb0EE"
        (twin_desc,) = [d for k, d in f32.items() if twin in k]
        vgpr, twin_vgpr = _field(desc, "next_free_vgpr"), _field(twin_desc, "next_free_vgpr")
        lds, twin_lds = _field(desc, "group_segment_fixed_size"), _field(twin_desc, "group_segment_fixed_size")
        print(f"{kernel} V{v} R{r}: {vgpr} VGPRs (float32 twin {twin_vgpr}), {lds} B LDS (twin {twin_lds})")
        assert _field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        assert lds == twin_lds, name
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc), f"{name}: fp32 subnormals are flushed"
        assert re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", desc), f"{name}: fp16 subnormals are flushed"
