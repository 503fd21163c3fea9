"""The random plans of tests/test_gpu_variant_fuzz.py without a GPU (cases: tests/variant_fuzz_cases.py): that the library
accepts every twin, that the fixed seed list reaches the code the GPU test is meant for (the coverage census), that the
expectation tells the wrong readings apart, and that `column_at` names the right column.  This file is what keeps the GPU
test from passing on a draw that does not reach the variants' cross-feature paths."""
import numpy as np
import pytest

import narrow_output_cases as N
import table_q8_cases as Q
import variant_fuzz_cases as F
from recom_amd.ops import Plan
from recom_amd.plan import (FORM_BATCH_COL_REDUCTION, FORM_GATHER, FORM_GATHER_SCATTER, FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE,
                            IDS_F32_BUCKETIZE, IDS_I32, IDS_I64, SEG_CSR_I32, SEG_IDS_I32, SEG_IDS_I64)


# ---- 1. the library accepts the twins -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", F.SEEDS)
def test_the_library_accepts_every_twin(seed):
    spec32 = F.plan(seed)[0]
    assert spec32.read_inputs(), "a seed without a lookup column tests no table format"
    for target in F.TARGETS:
        spec = F.twin(seed, target)[0]
        p = Plan(spec, host_only=True)
        what = (seed, target)
        assert p.out_dtype() == spec.out_dtype == F.NARROW.get(target, "f32"), what
        if target == "tabmix":
            kinds = F.mixed_kinds(seed)
            assert len({kinds[t] for t in spec32.read_inputs()}) > 1, (what, "one kind for all tables is the plan-wide plan")
            assert spec.mixed_tables() and p.table_dtype() == "mixed", what
            assert p.table_dtypes() == tuple(k if t in spec32.read_inputs() else "-" for t, k in enumerate(kinds)), what
        else:
            assert p.table_dtype() == spec.table_dtype == F.PLAN_WIDE.get(target, "f32"), what
            assert set(p.table_dtypes()) <= {spec.table_dtype, "-"}, what
        assert p.counts()["columns"] == spec32.n_columns and p.counts()["groups"] == spec32.n_groups, what
        p.close()


# ---- 2. the coverage census -------------------------------------------------------------------------------------------------
def test_the_seed_list_is_short_and_every_seed_is_eligible():
    assert 1 <= len(F.SEEDS) <= 10 and len(set(F.SEEDS)) == len(F.SEEDS)
    assert all(0 <= s < 64 and F.eligible(s) for s in F.SEEDS)


def test_the_census_names_what_the_issue_names():
    """FACTS, spelled out once more: a fact dropped from the list would otherwise drop out of the census unnoticed."""
    lookup = (FORM_GATHER, FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER)
    forms = lookup + (FORM_PASSTHROUGH, FORM_BATCH_COL_REDUCTION)
    want = {("form", f, k) for f in lookup for k in F.KINDS}
    want |= {("ids", s, k) for s in (IDS_I32, IDS_I64, IDS_F32_BUCKETIZE) for k in F.KINDS}
    want |= {("seg", s, k) for s in (SEG_CSR_I32, SEG_IDS_I32, SEG_IDS_I64) for k in F.KINDS}
    want |= {(w, k) for w in ("xform", "hash", "long_bag") for k in F.KINDS}
    want |= {("form_vec", f, v) for f in forms for v in (4, 2, 1)}
    want |= {("span_three_kinds",), ("span_one_kind",), ("columns_100",), ("groups_3",), ("vocab_1",), ("reshape", "div"),
             ("reshape", "mul"), ("scatter_twice",), ("scatter_outside",), ("batch", 1), ("batch", 257)}
    assert set(F.FACTS) == want and len(F.FACTS) == len(want) == 74
    assert F.KINDS == ("f32", "bf16", "f16", "q8") and F.LONG_BAG == 384 and F.WAVE == 64


@pytest.mark.parametrize("fact", F.FACTS, ids=["-".join(str(x) for x in f) for f in F.FACTS])
def test_census(fact):
    """Over SEEDS — the plans, the kinds drawn for `tabmix`, the three requests of each: every lookup form, id source, segment
    encoding (on a pooled column), SELECT / FILTER column and hashed column with each of the four table kinds; a 64-slot span
    with three kinds or more and one with a single kind in a mixed plan (the two branches of the ballot); each of the five
    forms at V 4, 2 and 1; a plan of 100 columns or more, one of three concat groups, a table of vocabulary 1, a folded
    reshape of each kind; a bag of more than 384 ids on a pooled column of each kind, a GATHER_SCATTER row hit twice and one
    outside the output, a batch of 1 and one of 257."""
    assert any(fact in F.facts(s) for s in F.SEEDS), fact


def test_the_facts_are_what_the_plans_hold():
    """`facts` against the plan it describes, for the facts that can be seen directly."""
    for seed in F.SEEDS:
        spec = F.plan(seed)[0]
        held = F.facts(seed)
        assert (("columns_100",) in held) == (spec.n_columns >= 100) and (("groups_3",) in held) == (spec.n_groups == 3)
        assert (("vocab_1",) in held) == any(c.vocab == 1 and c.form in F.LOOKUP for c in spec.columns)
        p = Plan(spec, host_only=True)
        assert {f[2] for f in held if f[0] == "form_vec"} == {F.vec_of(spec)}
        assert all(c.dim % F.vec_of(spec) == 0 for c in spec.columns)
        assert sum(p.group_width(g) for g in range(spec.n_groups)) == sum(c.dim for c in spec.columns)
        p.close()
        for r in F.requests(seed):
            assert len(r.batches) == spec.n_groups and set(r.batches) <= set(F.BATCHES)
            assert (("batch", 257) in held) or 257 not in r.batches


def test_seeds_is_what_the_search_finds():
    """`python tests/variant_fuzz_cases.py` prints the tuple the file holds: the smallest set out of range(64)."""
    assert F.search() == F.SEEDS
    assert not F.missing(F.SEEDS) and all(F.missing(F.SEEDS[:i] + F.SEEDS[i + 1:]) for i in range(len(F.SEEDS)))


# ---- 3. the expectation can tell the wrong readings apart -------------------------------------------------------------------
def _differ(a, b) -> int:
    """elements with different bit patterns"""
    return sum(int((np.ascontiguousarray(x).view(np.uint32) != np.ascontiguousarray(y).view(np.uint32)).sum()) for x, y in zip(a, b))


def _size(groups) -> int:
    return sum(g.size for g in groups)


def _read_kinds(seed, target, t) -> set:
    """the table kinds of the lookup columns that read at least one valid id in request t: what the float32 plan gives on
    tables of ones is non-zero exactly in those columns"""
    spec = F.twin(seed, target)[0]
    ones, _ = F.oracle_on(seed, [np.ones_like(x) for x in F.plan(seed)[1]], t)
    out = set()
    for c, off in zip(spec.columns, spec.column_offsets()):
        if c.form in F.LOOKUP and ones[c.concat_group][:, off:off + c.dim].any():
            out.add(spec.input_table_dtype(c.table_input))
    return out


@pytest.mark.parametrize("seed", F.SEEDS)
def test_the_expectation_tells_the_wrong_readings_apart(seed):
    """Properties of the inputs and of the reference alone.  The oracle's groups hold no NaN, so every comparison is one of
    bit patterns.  Shares of differing elements over the three requests, seeds 1 / 11 / 22 (all elements of all groups,
    PASSTHROUGH and BATCH_COL_REDUCTION columns and rows without ids included):

      each table target against the float32 plan on the unrounded tables (asserted per request that reads a table of a
        non-f32 kind through a valid id)             tab_bf16 50.5 / 52.4 / 45.7 %, tab_f16 50.5 / 52.3 / 45.6 %,
                                                     tab_q8 45.0 / 49.2 / 45.0 %, tabmix 37.1 / 37.4 / 35.0 %
      tab_q8 against the oracle on two_roundings of the same bytes                  26.9 / 29.8 / 29.0 %
      narrow_bf16 against truncate_bf16 of the float32 result                       39.7 / 39.9 / 40.1 %
      tabmix against every table read by its span neighbour's loader               40.2 / 31.6 / 30.7 %  (24 / 18 / 190 tables)

    Only "greater than zero" is asserted."""
    f32 = [F.expectation32(seed, "narrow_bf16", t) for t in range(F.N_REQUESTS)]       # the float32 plan on the unrounded tables
    total = sum(_size(g) for g, _ in f32)
    shares = {}
    for target in ("tab_bf16", "tab_f16", "tab_q8", "tabmix"):
        n = 0
        for t in range(F.N_REQUESTS):
            want, bad = F.expectation(seed, target, t)
            assert not any(np.isnan(w).any() for w in want), (seed, target, t)
            assert bad == f32[t][1], (seed, target, t)                     # the id path does not depend on the tables
            d = _differ(want, f32[t][0])
            if _read_kinds(seed, target, t) - {"f32"}:
                assert d > 0, (seed, target, t, "the expectation is the float32 plan's: the table format cannot be seen")
            n += d
        shares[target] = n / total
    assert not any(np.isnan(w).any() for g, _ in f32 for w in g), seed

    enc = F.twin(seed, "tab_q8")[1]
    other = [Q.two_roundings(q) for q in enc]
    shares["two_roundings"] = sum(_differ(F.expectation(seed, "tab_q8", t)[0], F.oracle_on(seed, other, t)[0])
                                  for t in range(F.N_REQUESTS)) / total
    assert shares["two_roundings"] > 0, seed

    n = 0
    for t in range(F.N_REQUESTS):
        got = F.expectation(seed, "narrow_bf16", t)[0]
        n += sum(int((g != N.truncate_bf16(w)).sum()) for g, w in zip(got, f32[t][0]))
    shares["truncate_bf16"] = n / total
    assert n > 0, seed

    wrong, n_tables = F.misread_tables(seed)
    assert n_tables > 0, (seed, "no table has a span neighbour of another kind")
    shares["neighbour"] = sum(_differ(F.expectation(seed, "tabmix", t)[0], F.oracle_on(seed, wrong, t)[0])
                              for t in range(F.N_REQUESTS)) / total
    assert shares["neighbour"] > 0, seed
    print(seed, n_tables, {k: round(100 * v, 1) for k, v in shares.items()})


def test_some_request_counts_bad_ids():
    """ids outside the vocabulary are drawn, and the running total the GPU test compares is not 0 throughout"""
    bad = {seed: sum(F.expectation(seed, "narrow_bf16", t)[1] for t in range(F.N_REQUESTS)) for seed in F.SEEDS}
    assert any(v > 0 for v in bad.values()), bad


def test_the_narrow_targets_share_one_oracle_run():
    seed = F.SEEDS[0]
    a, b = F.expectation(seed, "narrow_bf16", 0), F.expectation(seed, "narrow_f16", 0)
    assert F.expectation32(seed, "narrow_bf16", 0)[0][0] is F.expectation32(seed, "narrow_f16", 0)[0][0]
    assert all(x.dtype == np.uint16 and y.dtype == np.uint16 and x.shape == y.shape for x, y in zip(a[0], b[0])) and a[1] == b[1]
    assert all(np.array_equal(x, N.narrow(w, "bf16")) for x, w in zip(a[0], F.expectation32(seed, "narrow_bf16", 0)[0]))


def test_the_requests_of_a_seed_do_not_depend_on_the_target_or_the_order_of_calls():
    seed = F.SEEDS[0]
    first = [(r.batches, r.blob.tobytes()) for r in F.requests(seed)]
    F._drawn.cache_clear()
    F.twin.cache_clear()
    F.twin(seed, "tabmix")
    assert [(r.batches, r.blob.tobytes()) for r in F.requests(seed)] == first
    rng = np.random.default_rng(F.BASE + seed)                     # the plan is test_gpu_fuzz.random_model's, unchanged
    from test_gpu_fuzz import random_model
    spec, tables, _ = random_model(rng)
    import dataclasses
    for a, b in zip(spec.columns, F.plan(seed)[0].columns):
        assert dataclasses.replace(a, boundaries=None) == dataclasses.replace(b, boundaries=None)
        assert (a.boundaries is None) == (b.boundaries is None) and (a.boundaries is None or np.array_equal(a.boundaries, b.boundaries))
    assert len(spec.columns) == F.plan(seed)[0].n_columns
    assert all(np.array_equal(a, b) for a, b in zip(tables, F.plan(seed)[1]))


# ---- 4. column_at -----------------------------------------------------------------------------------------------------------
def test_column_at_names_the_column_of_the_first_and_last_element_of_every_column():
    seed = next(s for s in F.SEEDS if F.plan(s)[0].n_groups > 1)
    spec = F.twin(seed, "tabmix")[0]
    kinds = F.mixed_kinds(seed)
    offs = spec.column_offsets()
    assert spec.n_groups > 1 and len({c.concat_group for c in spec.columns}) == spec.n_groups
    for k, c in enumerate(spec.columns):
        kind = kinds[c.table_input] if c.form in F.LOOKUP else None
        want = (k, c.form, c.id_source, c.seg_kind, kind)
        assert F.column_at(spec, c.concat_group, offs[k]) == want
        assert F.column_at(spec, c.concat_group, offs[k] + c.dim - 1) == want
    spec32 = F.plan(seed)[0]
    k = next(k for k, c in enumerate(spec32.columns) if c.form in F.LOOKUP)
    assert F.column_at(spec32, spec32.columns[k].concat_group, offs[k])[4] == "f32"
    for g in range(spec.n_groups):
        with pytest.raises(IndexError):
            F.column_at(spec, g, spec.group_width(g))
