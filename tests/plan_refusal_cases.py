"""The refusal matrix of plan descriptors: every storage-format family against every condition the library refuses (or
accepts) by name, as raw descriptors for ``fcp_plan_create_ex``.  ``tests/golden/plan_refusals.json`` holds what the library
answered for each of them — (status, message) — BEFORE the descriptor code was folded into one rule list, and what the
Python mirror (``PlanSpec.validate``) raised where that differs from the library's answer:

    python tests/plan_refusal_cases.py --record        (with the library and the package of the commit to record)

The plan has three columns, one of them pooled — the smallest that can express every case: a condition on column k turns
that column into what the condition needs (a pooled column for weights / sqrtn, an EXTERNAL slot, a payload column).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_refusals.json")

# == include/fcp_hip.h
OUT_BF16, OUT_F16, TAB_BF16, TAB_F16, TAB_Q8, PER_INPUT, HOST_ONLY = 1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5, 1 << 6, 1 << 31
GATHER, POOLED, PASSTHROUGH, EXTERNAL = 1, 2, 4, 6
SUM, SQRTN = 1, 3
KINDS = ("f32", "bf16", "f16", "q8")            # FCP_TAB_* order
# host inputs: ids of columns 0..2 (int64), the pooled column's CSR offsets (int32), two float32 tensors (weights / payload)
RANKS, ELEM_SIZES = [1, 1, 1, 1, 1, 2], [8, 8, 8, 4, 4, 4]
CSR_INPUT, F32_INPUTS = 3, (4, 5)

# family -> (flag bits, table_kind1 per column or None)
FAMILIES = {
    "out_bf16": (OUT_BF16, None), "out_f16": (OUT_F16, None),
    "tab_bf16": (TAB_BF16, None), "tab_f16": (TAB_F16, None), "tab_q8": (TAB_Q8, None),
    "per_input_mixed": (PER_INPUT, (1, 2, 4)),
    **{f"per_input_all_{n}": (PER_INPUT, (1 + k,) * 3) for k, n in enumerate(KINDS)},
}
PLAN_CONDITIONS = ("sharded", "narrow", "per_column")
COLUMN_CONDITIONS = ("external", "weights", "sqrtn")
SINGLES = ("none", "sharded", "per_column", "external@0", "weights@1", "sqrtn@1", "narrow", "both_out_bits", "second_table_bit",
           "q8_table_bit", "other_table_flag", "shared_table_other_kind", "kind1_out_of_range", "kind1_without_table")
PAIRS = tuple(f"{p}+{c}@1" for p in PLAN_CONDITIONS for c in COLUMN_CONDITIONS) + ("weights@0+sqrtn@1",) + \
    tuple(f"{c}@0+{c}@2" for c in COLUMN_CONDITIONS)


def _base(family):
    flags, kinds1 = FAMILIES[family]
    cols = [dict(form=GATHER, combiner=0, table=k, weights=-1, kind1=kinds1[k] if kinds1 else 0) for k in range(3)]
    cols[1].update(form=POOLED, combiner=SUM)
    return dict(flags=flags, layout=0, shard_world=1, columns=cols)


def _apply(d, cond):
    what, _, k = cond.partition("@")
    k = int(k) if k else 0
    c = d["columns"][k] if what in COLUMN_CONDITIONS + ("kind1_out_of_range", "kind1_without_table") else None
    if what == "sharded":
        d["shard_world"] = 2
    elif what == "per_column":
        d["layout"] = 1
    elif what == "narrow":                          # an output bit added
        d["flags"] |= OUT_BF16
    elif what == "both_out_bits":
        d["flags"] |= OUT_BF16 | OUT_F16
    elif what == "second_table_bit":
        d["flags"] |= TAB_BF16 if d["flags"] & TAB_F16 else TAB_F16
    elif what == "q8_table_bit":
        d["flags"] |= TAB_Q8
    elif what == "other_table_flag":                # a plan-wide table bit together with the per-input flag
        d["flags"] |= TAB_BF16 if d["flags"] & PER_INPUT else PER_INPUT
    elif what == "shared_table_other_kind":         # columns 0 and 2 read table 0 and name different kinds
        d["columns"][2].update(table=0, kind1=1 + d["columns"][0]["kind1"] % 4)
    elif what == "kind1_out_of_range":
        c["kind1"] = 6
    elif what == "kind1_without_table":
        c.update(form=PASSTHROUGH, combiner=0, kind1=2)
    elif what == "external":
        c.update(form=EXTERNAL, combiner=0, kind1=0)
    elif what == "weights":
        c.update(form=POOLED, combiner=c["combiner"] or SUM, weights=F32_INPUTS[0])
    elif what == "sqrtn":
        c.update(form=POOLED, combiner=SQRTN)
    elif what != "none":
        raise ValueError(cond)


def cases():
    """[(name, descriptor dict)] in a fixed order: the golden file is keyed by name."""
    out = []
    for family in FAMILIES:
        for conds in SINGLES + PAIRS:
            d = _base(family)
            for cond in conds.split("+"):
                _apply(d, cond)
            out.append((f"{family}/{conds}", d))
    return out


# ---- the library's answer ---------------------------------------------------------------------------------------------------
def column_fields(k, c):
    """fcp_column_desc_t of column k of a case, in plan-file order: form, combiner, dim, id_source, vocab, table_input, ids_input,
    seg_input, seg_kind, seg_stride, rows_source, rows_arg, concat_group, concat_slot."""
    form = c["form"]
    lookup, pooled = form in (GATHER, POOLED), form == POOLED
    return (form, c["combiner"], 4, 1, 100 if lookup else 0, c["table"] if lookup else -1,
            -1 if form == EXTERNAL else F32_INPUTS[1] if form == PASSTHROUGH else k, CSR_INPUT if pooled else -1, 3 if pooled else 0, 1,
            3 if form == EXTERNAL else 1 if pooled else 2 if form == PASSTHROUGH else 0, F32_INPUTS[1] if form == PASSTHROUGH else 0, 0, k)


def create_raw(L, lib, d):
    """fcp_plan_create_ex of a host-only plan, past the Python mirror: (status, message)."""
    n = len(d["columns"])
    cols, ext = (lib.ColumnDesc * n)(), (lib.ColumnExt * n)()
    for k, c in enumerate(d["columns"]):
        v = column_fields(k, c)
        cols[k] = lib.ColumnDesc(*v[:12], 0, None, v[12], v[13], 0, 0, None, None, 0, 0)
        ext[k].weights_input1 = c["weights"] + 1
        ext[k].table_kind1 = c["kind1"]
    ranks, esz = (C.c_int32 * len(RANKS))(*RANKS), (C.c_int32 * len(RANKS))(*ELEM_SIZES)
    desc = lib.PlanDesc(lib.FCP_ABI_VERSION, n, cols, len(RANKS), ranks, esz, 3, 1, 1, d["layout"], 0, 0, d["shard_world"],
                        d["flags"] | HOST_ONLY)
    h = C.c_void_p()
    rc = L.fcp_plan_create_ex(C.byref(desc), ext, C.byref(h))
    if rc == lib.FCP_OK:
        L.fcp_plan_destroy(h)
        return rc, ""
    return rc, L.fcp_last_error().decode()


def write_cases(path, golden):
    """The matrix and its recorded answers as text, for tests/native/plan_desc_san.cc: a header "cases host_inputs (rank
    elem_size)...", then per case one line of numbers — name, flags, layout, shard_world, device inputs, symbols, columns, status,
    and per column its fields, weights_input1 and table_kind1 — and one line with the message."""
    with open(path, "w") as f:
        all_cases = cases()
        f.write(f"{len(all_cases)} {len(RANKS)} " + " ".join(f"{r} {e}" for r, e in zip(RANKS, ELEM_SIZES)) + "\n")
        for name, d in all_cases:
            v = [name, d["flags"] | HOST_ONLY, d["layout"], d["shard_world"], 3, 1, len(d["columns"]), golden[name]["status"]]
            for k, c in enumerate(d["columns"]):
                v += list(column_fields(k, c)) + [c["weights"] + 1, c["kind1"]]
            f.write(" ".join(str(x) for x in v) + "\n" + golden[name]["message"] + "\n")


# ---- the Python mirror ------------------------------------------------------------------------------------------------------
def plan_spec(d):
    """The PlanSpec of a case, or None where PlanSpec cannot express it (table_kind1 values that are no per-input format)."""
    from recom_amd.plan import ColumnSpec, PlanSpec
    flags = d["flags"]
    table_dtypes = None
    if flags & PER_INPUT:
        by_input = {}
        for c in d["columns"]:
            if c["form"] not in (GATHER, POOLED):
                if c["kind1"]:
                    return None
                continue
            if not 0 <= c["kind1"] <= 4 or by_input.setdefault(c["table"], c["kind1"]) != c["kind1"]:
                return None
        table_dtypes = tuple(KINDS[max(by_input[t], 1) - 1] if t in by_input else "-" for t in range(3))
    out = {OUT_BF16: "bf16", OUT_F16: "f16"}.get(flags & (OUT_BF16 | OUT_F16), "f32")
    tab = {TAB_BF16: "bf16", TAB_F16: "f16", TAB_Q8: "q8"}.get(flags & (TAB_BF16 | TAB_F16 | TAB_Q8), "f32")
    cols = []
    for k, c in enumerate(d["columns"]):
        v = column_fields(k, c)
        cols.append(ColumnSpec(form=v[0], combiner=v[1], dim=v[2], id_source=v[3], vocab=v[4], table_input=v[5], ids_input=v[6], seg_input=v[7],
                               seg_kind=v[8], seg_stride=v[9], rows_source=v[10], rows_arg=v[11], concat_group=v[12], concat_slot=v[13],
                               weights_input=c["weights"]))
    # bits that out_dtype / table_dtype do not stand for (two bits of one family at once) travel in PlanSpec.flags
    return PlanSpec(columns=cols, host_input_ranks=list(RANKS), host_input_elem_sizes=list(ELEM_SIZES), n_device_inputs=3, n_symbols=1,
                    layout=d["layout"], shard_world=d["shard_world"], flags=flags & ~PER_INPUT, out_dtype=out, table_dtype=tab,
                    table_dtypes=table_dtypes)


def python_answer(d):
    """What ``PlanSpec.validate`` does with a case: None (inexpressible), or (exception class name or "", message)."""
    spec = plan_spec(d)
    if spec is None:
        return None
    try:
        spec.validate()
    except ValueError as e:
        return type(e).__name__, str(e)
    return "", ""


def expected_python(status, message):
    """The Python answer that mirrors the library's (status, message)."""
    if status == 0:
        return "", ""
    if status == 1:
        return "ValueError", message
    for subject, cls in (("narrow output", "NarrowOutputUnsupported"), ("per-input table formats", "TablesMixedUnsupported"),
                         ("8-bit tables", "TablesQ8Unsupported"), ("16-bit tables", "Tables16Unsupported")):
        if message.split(": ", 1)[-1].startswith(subject) or message.startswith(subject):
            return cls, message
    return "?", message


def record():
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (behind PYTHONPATH: the commit to record)
    from recom_amd import lib
    L = lib.load()
    golden = {}
    for name, d in cases():
        status, message = create_raw(L, lib, d)
        entry = {"status": status, "message": message}
        py = python_answer(d)
        if py is not None and py != expected_python(status, message):
            entry["python"] = list(py)             # the mirror disagrees with the library here, and did before the fold
        golden[name] = entry
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(golden)} cases, {sum('python' in e for e in golden.values())} where the Python mirror differs, "
          f"{os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    else:
        sys.exit(__doc__)
