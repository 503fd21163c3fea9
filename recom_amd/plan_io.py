"""Column-plan files: what the `dlpath` attr of ``Addons>FeatureColumnProcess``
points at in this build (the reference points it at a JIT-compiled ``.so``,
``feature_column_process_op_gpu.cu.cc:49-55``).  Plain text, parsed by
``tf_shim/fcp_tf_ops.cc::LoadPlanFile`` and by :func:`load_plan`.
"""
from __future__ import annotations

import numpy as np

from .plan import COMBINER_SQRTN, OUT_FORMATS, TABLE_FORMATS, ColumnSpec, PlanSpec, StageInfo


def save_plan(spec: PlanSpec, path: str, stage: "StageInfo | None" = None) -> None:
    """``stage``: the stage section (version 3 files) — how ``Addons>ConcatInputs`` packs each of its inputs for this
    (staged) plan; one entry per host input of ``spec``."""
    spec.validate()
    if stage is not None and len(stage.modes) != spec.n_host_inputs:
        raise ValueError("the stage section lists one entry per host input of the plan")
    with open(path, "w") as f:
        maps = [(k, c) for k, c in enumerate(spec.columns) if len(c.seg_mul)]
        weights = [(k, c) for k, c in enumerate(spec.columns) if c.weights_input >= 0]
        v5 = bool(weights) or any(c.combiner == COMBINER_SQRTN for c in spec.columns)
        if spec.table_dtypes is not None and not spec.mixed_tables():   # one kind under per-input formats: the plan-wide plan's file
            read = spec.read_inputs()
            spec = spec.with_table_dtypes(None).with_table_dtype(spec.table_dtypes[read[0]] if read else "f32")
        if spec.table_dtypes is not None:   # version 8, plans whose tables have more than one format only: one name per device input
            f.write(f"fcp_plan 8\ntable_dtypes {spec.n_device_inputs} {' '.join(spec.table_dtypes)}\n")
        elif spec.table_dtype != "f32":   # version 7, plans with 16-bit or 8-bit tables only (never narrow output as well): likewise
            f.write(f"fcp_plan 7\ntable_dtype {spec.table_dtype}\n")
        elif spec.out_dtype != "f32":   # version 6, narrow-output plans only: the dtype is the file's second line
            f.write(f"fcp_plan 6\nout_dtype {spec.out_dtype}\n")
        else:
            f.write(f"fcp_plan {5 if v5 else 4 if maps else 3 if stage is not None else 2}\n")
        f.write(f"layout {spec.layout}\n")
        f.write(f"groups {spec.n_groups} symbols {spec.n_symbols} device_inputs {spec.n_device_inputs}\n")
        f.write(f"host_inputs {spec.n_host_inputs}\n")
        for r, e in zip(spec.host_input_ranks, spec.host_input_elem_sizes):
            f.write(f"{r} {e}\n")
        f.write(f"columns {spec.n_columns}\n")
        for c in spec.columns:
            b = [] if c.boundaries is None else [repr(float(np.float32(x))) for x in c.boundaries]
            f.write(" ".join(str(x) for x in (
                c.form, c.combiner, c.dim, c.id_source, c.vocab, c.table_input, c.ids_input, c.seg_input,
                c.seg_kind, c.seg_stride, c.rows_source, c.rows_arg, c.concat_group, c.concat_slot, len(b))))
            f.write(" " + " ".join(b) if b else "")
            # version 2: the id transform — mode, number of intervals, substitute, hash buckets, (lo, hi) pairs
            x = [c.xform_mode, len(c.xform_lo), c.xform_substitute, c.hash_buckets] + \
                [v for p in zip(c.xform_lo, c.xform_hi) for v in p]
            f.write(" " + " ".join(str(int(v)) for v in x) + "\n")
        if v5:       # version 5: per-id weights — column, host input (a plan that only uses the sqrtn combiner: "weights 0")
            f.write(f"weights {len(weights)}\n")
            for k, c in weights:
                f.write(f"{k} {int(c.weights_input)}\n")
        if maps:     # version 4: segment-id maps — column, coordinates, symbol, symbol slot, mul0..mul3, div
            f.write(f"segmaps {len(maps)}\n")
            for k, c in maps:
                mul = [int(v) for v in c.seg_mul] + [0] * (4 - len(c.seg_mul))
                f.write(" ".join(str(int(v)) for v in [k, len(c.seg_mul), c.seg_sym, c.seg_sym_slot] + mul + [c.seg_div]) + "\n")
        if stage is not None:
            f.write(f"stage {len(stage.modes)} symbols_input {stage.symbols_input}\n")
            for m, k in zip(stage.modes, stage.rows_symbol):
                f.write(f"{int(m)} {int(k)}\n")


def load_plan(path: str) -> PlanSpec:
    tok = open(path).read().split()
    it = iter(tok)

    def nxt():
        try:
            return next(it)
        except StopIteration:
            raise ValueError(f"truncated column plan {path}") from None

    if nxt() != "fcp_plan":
        raise ValueError("bad plan header")
    version = int(nxt())
    if version not in (1, 2, 3, 4, 5, 6, 7, 8):
        raise ValueError("bad plan header")
    out_dtype = table_dtype = "f32"
    table_dtypes = None
    if version >= 8:              # "table_dtypes D k0 ... k(D-1)": the same place and rules, in version 8 files and no others
        if nxt() != "table_dtypes":
            raise ValueError(f"expected 'table_dtypes D k0 ... k(D-1)' in {path}")
        try:
            n_kinds = int(nxt())
        except ValueError:
            raise ValueError(f"expected 'table_dtypes D k0 ... k(D-1)' in {path}") from None
        if n_kinds < 0:
            raise ValueError(f"expected 'table_dtypes D k0 ... k(D-1)' in {path}")
        table_dtypes = tuple(nxt() for _ in range(n_kinds))
        for n in table_dtypes:
            if n != "-" and n not in TABLE_FORMATS:
                raise ValueError(f"unknown table dtype {n!r} in the table_dtypes line of {path}")
    elif version >= 7:              # "table_dtype bf16|f16|q8": the same place and rules, in version 7 files and no others
        if nxt() != "table_dtype":
            raise ValueError(f"expected 'table_dtype bf16', 'table_dtype f16' or 'table_dtype q8' in {path}")
        table_dtype = nxt()
        if table_dtype == "f32" or table_dtype not in TABLE_FORMATS:
            raise ValueError(f"unknown table_dtype {table_dtype!r} in {path}")
    elif version >= 6:            # "out_dtype bf16|f16": here and nowhere else, in version 6 files and no others
        if nxt() != "out_dtype":
            raise ValueError(f"expected 'out_dtype bf16' or 'out_dtype f16' in {path}")
        out_dtype = nxt()
        if out_dtype == "f32" or out_dtype not in OUT_FORMATS:
            raise ValueError(f"unknown out_dtype {out_dtype!r} in {path}")
    if nxt() != "layout":
        raise ValueError(f"expected 'layout' in {path}")
    layout = int(nxt())
    assert nxt() == "groups"
    n_groups = int(nxt())
    assert nxt() == "symbols"
    n_symbols = int(nxt())
    assert nxt() == "device_inputs"
    n_dev = int(nxt())
    assert nxt() == "host_inputs"
    n_host = int(nxt())
    ranks, esz = [], []
    for _ in range(n_host):
        ranks.append(int(nxt()))
        esz.append(int(nxt()))
    assert nxt() == "columns"
    cols = []
    for _ in range(int(nxt())):
        v = [int(nxt()) for _ in range(15)]
        b = np.asarray([float(nxt()) for _ in range(v[14])], np.float32) if v[14] else None
        mode, lo, hi, sub, hb = 0, [], [], 0, 0
        if version >= 2:
            mode, n, sub, hb = int(nxt()), int(nxt()), int(nxt()), int(nxt())
            for _ in range(n):
                lo.append(int(nxt()))
                hi.append(int(nxt()))
        cols.append(ColumnSpec(form=v[0], combiner=v[1], dim=v[2], id_source=v[3], vocab=v[4], table_input=v[5],
                               ids_input=v[6], seg_input=v[7], seg_kind=v[8], seg_stride=v[9], rows_source=v[10],
                               rows_arg=v[11], concat_group=v[12], concat_slot=v[13], boundaries=b,
                               xform_mode=mode, xform_lo=tuple(lo), xform_hi=tuple(hi), xform_substitute=sub,
                               hash_buckets=hb))
    import dataclasses
    rest = list(it)
    if rest[:1] == ["weights"]:
        if version < 5:
            raise ValueError(f"a weights section needs a version-5 plan file: {path}")
        m = int(rest[1])
        if m < 0 or len(rest) < 2 + 2 * m:
            raise ValueError(f"truncated weights section in {path}")
        for j in range(m):
            k, i = int(rest[2 + 2 * j]), int(rest[3 + 2 * j])
            if not 0 <= k < len(cols) or cols[k].weights_input >= 0 or not 0 <= i < n_host:
                raise ValueError(f"malformed weights entry {j} in {path}")
            cols[k] = dataclasses.replace(cols[k], weights_input=i)
        rest = rest[2 + 2 * m:]
    if version >= 4 and rest[:1] == ["segmaps"]:
        for j in range(int(rest[1])):
            v = [int(x) for x in rest[2 + 9 * j: 11 + 9 * j]]
            cols[v[0]] = dataclasses.replace(cols[v[0]], seg_mul=tuple(v[4:4 + v[1]]), seg_div=v[8], seg_sym=v[2],
                                             seg_sym_slot=v[3])
    if tok.count("table_dtypes") != (1 if version >= 8 else 0):
        raise ValueError(f"misplaced or repeated table_dtypes line in {path}")
    if tok.count("table_dtype") != (1 if version == 7 else 0):
        raise ValueError(f"misplaced or repeated table_dtype line in {path}")
    if tok.count("out_dtype") != (1 if version == 6 else 0):   # anywhere but the second line, twice, or in an older file
        raise ValueError(f"misplaced or repeated out_dtype line in {path}")
    spec = PlanSpec(cols, ranks, esz, n_dev, n_groups=n_groups, n_symbols=n_symbols, layout=layout, out_dtype=out_dtype,
                    table_dtype=table_dtype)
    if table_dtypes is not None:
        if len(table_dtypes) != n_dev:
            raise ValueError(f"the table_dtypes line names {len(table_dtypes)} inputs, the plan has {n_dev} device inputs: {path}")
        read = set(spec.read_inputs())
        for t, n in enumerate(table_dtypes):
            if (n == "-") != (t not in read):
                raise ValueError(f"the table_dtypes line of {path} must name exactly the device inputs lookup columns read (input {t})")
        spec = dataclasses.replace(spec, table_dtypes=table_dtypes)
        if not spec.mixed_tables():
            raise ValueError(f"version 8 is for plans whose tables have more than one dtype: {path}")
    spec.validate()
    return spec


def load_stage(path: str) -> "StageInfo | None":
    """The stage section of a plan file as the LIBRARY parses it (``fcp_plan_file_stage_info`` — what the shim's
    ConcatInputsOp calls with the node's ``_fcp_plan`` attr), or None: a plain plan."""
    import ctypes as C
    from . import lib as _lib
    L = _lib.load()
    n, sym_in = C.c_int32(0), C.c_int32(-1)
    _lib.check(L.fcp_plan_file_stage_info(path.encode(), C.byref(n), None, None, 0, C.byref(sym_in)), "fcp_plan_file_stage_info")
    if n.value == 0:
        return None
    modes = np.zeros(n.value, np.uint8)
    rows = np.zeros(n.value, np.int32)
    _lib.check(L.fcp_plan_file_stage_info(path.encode(), C.byref(n), modes.ctypes.data, rows.ctypes.data, n.value,
                                          C.byref(sym_in)), "fcp_plan_file_stage_info")
    return StageInfo([int(m) for m in modes], [int(r) for r in rows], int(sym_in.value))
