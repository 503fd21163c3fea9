"""Random plans through the fused-kernel variants beside float32 — narrow output (bf16 / fp16), plan-wide bf16 / fp16 / q8
tables, per-input table formats: the plans, twins, requests, expectations and the coverage census of
tests/test_variant_fuzz_host.py (CPU) and tests/test_gpu_variant_fuzz.py (GPU).  Test data only: no GPU, no torch.

The draw is tests/test_gpu_fuzz.py::random_model, imported, not copied: none of what it draws (five forms, three id sources
with every bucketize tier, hashing, SELECT / FILTER, ids outside the vocabulary, three segment encodings with folded
reshapes, 1 to 3 groups with their own batches, V of 4 / 2 / 1, 1 to 400 columns, bags of up to 500 ids) is on the variants'
refusal list, so every plan has a narrow, a bf16, an fp16, a q8 and a per-table twin.

The yardstick is the one the variants promise, bit for bit: the float32 plan on the widened / dequantised tables — the C
oracle's result on the decoded tables — rounded once at the store for narrow output (narrow_output_cases.narrow).

`SEEDS` is the smallest set out of range(64) whose plans and requests together hold every combination the census names
(`facts`, `FACTS`); running this module prints it.  The census is asserted in tests/test_variant_fuzz_host.py."""
import dataclasses
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle")):      # as tests/conftest.py does: this module also runs as a script
    if _p not in sys.path:
        sys.path.insert(0, _p)

import narrow_output_cases as N
import table_mixed_cases as M
from recom_amd import synth
from recom_amd.plan import (FLAG_COUNT_BAD_IDS, FORM_BATCH_COL_REDUCTION, FORM_GATHER, FORM_GATHER_SCATTER, FORM_PASSTHROUGH,
                            FORM_SEGMENT_REDUCE, IDS_F32_BUCKETIZE, IDS_I32, IDS_I64, SEG_CSR_I32, SEG_IDS_I32, SEG_IDS_I64,
                            XFORM_NONE)
from test_gpu_fuzz import random_model

BASE = 7000
TARGETS = ("narrow_bf16", "narrow_f16", "tab_bf16", "tab_f16", "tab_q8", "tabmix")
NARROW = {"narrow_bf16": "bf16", "narrow_f16": "f16"}              # target -> out_dtype
PLAN_WIDE = {"tab_bf16": "bf16", "tab_f16": "f16", "tab_q8": "q8"}   # target -> table_dtype
SUFFIX = {"narrow_bf16": "_narrow", "narrow_f16": "_narrow", "tab_bf16": "_tab16", "tab_f16": "_tab16", "tab_q8": "_tabq8",
          "tabmix": "_tabmix"}                                     # what a fused kernel's name ends in
KINDS = M.KINDS                                                    # ("f32", "bf16", "f16", "q8")
BATCHES = (1, 2, 5, 33, 64, 130, 257)
N_REQUESTS = 3
LOOKUP = M.LOOKUP
FORMS = (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER, FORM_PASSTHROUGH, FORM_BATCH_COL_REDUCTION)
WAVE = M.WAVE                                                      # slots (of V elements) per span
LONG_BAG = 384                                                     # more ids than this: the ragged body's further rounds

# the smallest set out of range(64) for which the census holds (`python tests/variant_fuzz_cases.py` prints it)
SEEDS = (1, 11, 22)


# ---- plans and requests -----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Request:
    batches: tuple
    inputs: list
    symbols: np.ndarray
    blob: np.ndarray
    offsets: np.ndarray
    shapes: np.ndarray


def _pack(inputs):
    from recom_amd.ops import concat_inputs
    return concat_inputs(inputs)


@functools.lru_cache(maxsize=4)
def _drawn(seed: int):
    """(spec32, tables32, make, requests): the plan and, from the same generator continued, its three requests — drawn in
    one go, so that they depend on nothing but the seed."""
    rng = np.random.default_rng(BASE + seed)
    spec, tables, make = random_model(rng)
    spec = dataclasses.replace(spec, flags=FLAG_COUNT_BAD_IDS)
    for t in tables:
        t.setflags(write=False)
    reqs = []
    for _ in range(N_REQUESTS):
        batches = tuple(int(rng.choice(BATCHES)) for _ in range(spec.n_groups))
        inputs, symbols = make(rng, batches)
        reqs.append(Request(batches, inputs, symbols, *_pack(inputs)))
    return spec, tables, make, reqs


def plan(seed: int):
    """(spec32, tables32, make) of np.random.default_rng(BASE + seed)."""
    return _drawn(seed)[:3]


def requests(seed: int):
    """The three requests of a seed: the same for every target."""
    return _drawn(seed)[3]


def vec_of(spec) -> int:
    """V as the library derives it: the largest of 4, 2, 1 that divides every column's dim."""
    return 4 if all(c.dim % 4 == 0 for c in spec.columns) else 2 if all(c.dim % 2 == 0 for c in spec.columns) else 1


def mixed_kinds(seed: int) -> tuple:
    """One kind per table for the `tabmix` target, from a generator of their own: the plan a seed draws does not depend on
    them."""
    n = plan(seed)[0].n_device_inputs
    return tuple(str(k) for k in np.random.default_rng([BASE, seed]).choice(KINDS, n))


def _encode(table: np.ndarray, kind: str) -> np.ndarray:
    if kind == "f32":
        return table
    return synth.quantize_q8(table) if kind == "q8" else synth.table_patterns(table, kind)


def _decode(table: np.ndarray, kind: str) -> np.ndarray:
    if kind == "f32":
        return table
    return synth.dequantize_q8(table) if kind == "q8" else synth.table_values(table, kind)


@functools.lru_cache(maxsize=8)
def twin(seed: int, target: str):
    """(spec, tables as the plan reads them, decoded float32 tables) of a target."""
    spec32, tables, _ = plan(seed)
    if target in NARROW:
        return spec32.with_out_dtype(NARROW[target]), tables, tables
    if target in PLAN_WIDE:
        kinds = (PLAN_WIDE[target],) * len(tables)
        spec = spec32.with_table_dtype(PLAN_WIDE[target])
    else:
        assert target == "tabmix", target
        kinds = mixed_kinds(seed)
        spec = spec32.with_table_dtypes(kinds)
    spec.validate()
    enc = [_encode(t, k) for t, k in zip(tables, kinds)]
    dec = [_decode(t, k) for t, k in zip(enc, kinds)]
    for t in enc + dec:
        t.setflags(write=False)
    return spec, enc, dec


def oracle_on(seed: int, tables, t: int):
    """(groups, bad ids) of the float32 plan on float32 `tables`, request t (not cached)."""
    import fcp_oracle
    spec32 = plan(seed)[0]
    r = requests(seed)[t]
    want, bad = fcp_oracle.COracle().process_feature_columns(spec32.to_dict(), r.blob, r.offsets, r.shapes, list(tables), r.symbols)
    for w in want:
        w.setflags(write=False)
    return want, bad


@functools.lru_cache(maxsize=4 * N_REQUESTS)
def _oracle(seed: int, key: str, t: int):
    """Cached per (seed, decoded-tables key, request): "f32" is the key of both narrow targets."""
    return oracle_on(seed, plan(seed)[1] if key == "f32" else twin(seed, key)[2], t)


def expectation32(seed: int, target: str, t: int):
    """(float32 groups, bad ids) of the oracle behind `expectation`: for a narrow target the float32 plan's own result."""
    return _oracle(seed, "f32" if target in NARROW else target, t)


def expectation(seed: int, target: str, t: int):
    """(groups, bad ids) the target must give for request t: float32 matrices for the table targets, uint16 patterns for the
    narrow ones."""
    groups, bad = expectation32(seed, target, t)
    if target in NARROW:
        return [N.narrow(g, NARROW[target]) for g in groups], bad
    return groups, bad


def column_at(spec, group: int, element_offset: int):
    """(column index, form, id source, seg kind, table kind or None) of the column that holds element `element_offset` of a row
    of concat group `group` — for failure messages.  `spec`: the float32 plan or any twin (the columns are the same; the
    table kind is the twin's, None for a column without a table)."""
    for k, (c, off) in enumerate(zip(spec.columns, spec.column_offsets())):
        if c.concat_group == group and off <= element_offset < off + c.dim:
            kind = spec.input_table_dtype(c.table_input) if c.form in LOOKUP else None
            return k, c.form, c.id_source, c.seg_kind, kind
    raise IndexError(f"group {group} has no element {element_offset}")


# ---- what a kernel that picks a neighbour's loader would read -------------------------------------------------------------------
def neighbour_kinds(seed: int) -> list:
    """Per table of the `tabmix` twin: the kind of the nearest lookup column (in concat order) that shares a 64-slot span with
    the table's column and has another kind, or None."""
    spec = plan(seed)[0]
    kinds = mixed_kinds(seed)
    w = WAVE * vec_of(spec)
    offs = spec.column_offsets()
    out = [None] * spec.n_device_inputs
    cols = [(k, c, offs[k]) for k, c in enumerate(spec.columns) if c.form in LOOKUP]
    for k, c, off in cols:
        spans = set(range(off // w, (off + c.dim - 1) // w + 1))
        near = [(abs(o - off), kinds[d.table_input]) for j, d, o in cols
                if d.concat_group == c.concat_group and kinds[d.table_input] != kinds[c.table_input]
                and spans & set(range(o // w, (o + d.dim - 1) // w + 1))]
        if near:
            out[c.table_input] = min(near)[1]
    return out


def misread(table: np.ndarray, kind: str, other: str, dim: int):
    """float32 [vocab, dim]: what the plan would read if it took the bytes of `table` (of `kind`) for a table of `other` —
    table_mixed_cases.reinterpret, 37 rows at a time (row r of the other format begins at byte r x its row size, wherever
    the table begins); rows it cannot form (beyond the table's bytes) keep their true values.  None if it forms no row."""
    vocab = table.shape[0]
    raw = np.ascontiguousarray(table).view(np.uint8).reshape(-1)
    step = M.row_bytes(other, dim)
    out = np.array(_decode(table, kind), np.float32, copy=True)
    formed = 0
    for r0 in range(0, vocab, M.VOCAB):
        got = M.reinterpret(raw[r0 * step:], kind, other, dim)
        if got is None:
            break
        n = min(M.VOCAB, vocab - r0)
        out[r0:r0 + n] = got[:n]
        formed += n
    return out if formed else None


def misread_tables(seed: int):
    """(decoded tables of the `tabmix` twin with every table that has a span neighbour of another kind read by that
    neighbour's loader, the number of tables so changed)"""
    spec, enc, dec = twin(seed, "tabmix")
    kinds = mixed_kinds(seed)
    dims = {c.table_input: c.dim for c in spec.columns if c.form in LOOKUP}
    out, n = [], 0
    for t, other in enumerate(neighbour_kinds(seed)):
        wrong = None if other is None else misread(enc[t], kinds[t], other, dims[t])
        out.append(dec[t] if wrong is None else wrong)
        n += wrong is not None
    return out, n


# ---- the census -------------------------------------------------------------------------------------------------------------
def span_kinds(spec32, kinds, group: int):
    """per 64-slot span of the group: the kinds of the lookup columns with a slot in it"""
    w = WAVE * vec_of(spec32)
    out = [set() for _ in range(-(-spec32.group_width(group) // w))]
    for c, off in zip(spec32.columns, spec32.column_offsets()):
        if c.concat_group == group and c.form in LOOKUP:
            for sp in range(off // w, (off + c.dim - 1) // w + 1):
                out[sp].add(kinds[c.table_input])
    return out


def segment_rows(c, r: Request) -> np.ndarray:
    """The output row of every id of a pooled / scatter column with segment ids in request `r`, rows outside the output
    included: idx[0], or — a folded reshape — (sum_k idx[k] * mul[k]) // div with one factor times a symbol."""
    seg = r.inputs[c.seg_input]
    if c.seg_kind == SEG_IDS_I32:
        return seg.astype(np.int64)
    idx = seg.reshape(-1, c.seg_stride)
    if not len(c.seg_mul):
        return idx[:, 0]
    mul, div = [int(v) for v in c.seg_mul], int(c.seg_div)
    if c.seg_sym >= 0:
        s = int(r.symbols[c.seg_sym])
        if c.seg_sym_slot == 4:
            div *= s
        else:
            mul[c.seg_sym_slot] *= s
    return sum(idx[:, k] * m for k, m in enumerate(mul)) // div


def bag_lengths(c, r: Request) -> np.ndarray:
    """ids per output row of a pooled / scatter column in request `r` (ids of rows outside the output not counted)."""
    if c.seg_kind == SEG_CSR_I32:
        return np.diff(r.inputs[c.seg_input].astype(np.int64))
    rows = int(r.symbols[c.rows_arg])
    at = segment_rows(c, r)
    return np.bincount(at[(at >= 0) & (at < rows)], minlength=rows)


FACTS = tuple(
    [("form", f, k) for f in LOOKUP for k in KINDS] +                       # tabmix: every lookup form with every kind
    [("ids", s, k) for s in (IDS_I32, IDS_I64, IDS_F32_BUCKETIZE) for k in KINDS] +
    [("seg", s, k) for s in (SEG_CSR_I32, SEG_IDS_I32, SEG_IDS_I64) for k in KINDS] +      # on a pooled column
    [("xform", k) for k in KINDS] + [("hash", k) for k in KINDS] +
    [("span_three_kinds",), ("span_one_kind",)] +                            # the ballot's two branches
    [("form_vec", f, v) for f in FORMS for v in (4, 2, 1)] +
    [("columns_100",), ("groups_3",), ("vocab_1",), ("reshape", "div"), ("reshape", "mul")] +
    [("long_bag", k) for k in KINDS] +                                       # over the requests
    [("scatter_twice",), ("scatter_outside",), ("batch", 1), ("batch", 257)])


@functools.lru_cache(maxsize=None)
def facts(seed: int) -> frozenset:
    """Which of FACTS the plan of `seed`, its drawn kinds and its three requests hold."""
    spec, _, _, reqs = _drawn(seed)
    kinds = mixed_kinds(seed)
    v = vec_of(spec)
    out = set()
    for c in spec.columns:
        out.add(("form_vec", c.form, v))
        if c.form not in LOOKUP:
            continue
        k = kinds[c.table_input]
        out |= {("form", c.form, k), ("ids", c.id_source, k)}
        if c.form == FORM_SEGMENT_REDUCE:
            out.add(("seg", c.seg_kind, k))
            if len(c.seg_mul):
                out.add(("reshape", "div" if len(c.seg_mul) == 1 else "mul"))
        if c.xform_mode != XFORM_NONE:
            out.add(("xform", k))
        if c.hash_buckets:
            out.add(("hash", k))
        if c.vocab == 1:
            out.add(("vocab_1",))
        for r in reqs:
            if c.form == FORM_SEGMENT_REDUCE and bag_lengths(c, r).max(initial=0) > LONG_BAG:
                out.add(("long_bag", k))
            if c.form == FORM_GATHER_SCATTER:
                if bag_lengths(c, r).max(initial=0) >= 2:
                    out.add(("scatter_twice",))
                if c.seg_kind != SEG_CSR_I32:
                    at = segment_rows(c, r)
                    if ((at < 0) | (at >= int(r.symbols[c.rows_arg]))).any():
                        out.add(("scatter_outside",))
    if len(set(kinds[t] for t in spec.read_inputs())) > 1:
        for g in range(spec.n_groups):
            for held in span_kinds(spec, kinds, g):
                if len(held) >= 3:
                    out.add(("span_three_kinds",))
                if len(held) == 1:
                    out.add(("span_one_kind",))
    if spec.n_columns >= 100:
        out.add(("columns_100",))
    if spec.n_groups == 3:
        out.add(("groups_3",))
    for r in reqs:
        out |= {("batch", b) for b in r.batches if b in (1, 257)}
    return frozenset(out & set(FACTS))


def eligible(seed: int) -> bool:
    """A seed may be chosen if its plan has a lookup column and its drawn kinds are not all one kind (that is the plan-wide
    plan by design)."""
    spec = plan(seed)[0]
    read = spec.read_inputs()
    return bool(read) and len({mixed_kinds(seed)[t] for t in read}) > 1


def missing(seeds) -> list:
    """The facts of FACTS that no seed of `seeds` holds."""
    held = set().union(*[facts(s) for s in seeds]) if seeds else set()
    return [f for f in FACTS if f not in held]


def search(candidates=range(0, 64)) -> tuple:
    """The smallest set of eligible seeds out of `candidates` that holds every fact; of several, the first in order."""
    pool = [s for s in candidates if eligible(s)]
    have = {s: facts(s) for s in pool}
    lacking = [f for f in FACTS if not any(f in have[s] for s in pool)]
    assert not lacking, f"no seed of the candidates holds {lacking}"
    for size in range(1, 11):
        found = []

        def cover(chosen, open_facts):
            if not open_facts:
                found.append(tuple(sorted(chosen)))
                return
            if len(chosen) == size:
                return
            rarest = min(open_facts, key=lambda f: sum(f in have[s] for s in pool))      # every cover holds one of its seeds
            for s in pool:
                if rarest in have[s] and s not in chosen:
                    cover(chosen | {s}, open_facts - have[s])

        cover(frozenset(), frozenset(FACTS))
        if found:
            return min(found)
    raise AssertionError("the census needs more than 10 seeds")


if __name__ == "__main__":
    print(search())
