"""Per-id weights and the sqrtn combiner of pooled columns, without a GPU: the plan vocabulary (descriptor, extension record,
version-5 plan files, both parsers), the places that enumerate a column's host inputs, the restatement of
tests/weighted_bag_cases.py held to float64, PyTorch-CPU and the TF-graph evaluator, how well the cells' inputs tell a fused
multiply-add from the specified arithmetic, and the code-object facts of the weighted kernels."""
import dataclasses
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import weighted_bag_cases as W
from recom_amd import plan as PL
from recom_amd.plan import ColumnSpec, PlanSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spec(combiner=PL.COMBINER_MEAN, weighted=True, form=PL.FORM_SEGMENT_REDUCE, w_esz=4):
    """ids (int64), CSR offsets, weights -> one pooled column; a gather column beside it."""
    c = ColumnSpec(form, 8, 100, combiner, PL.IDS_I64, 0, 0, 1, PL.SEG_CSR_I32, 1, PL.ROWS_FROM_SYMBOL, 0, None, 0, 0,
                   weights_input=2 if weighted else -1)
    g = ColumnSpec(PL.FORM_GATHER, 4, 50, PL.COMBINER_NONE, PL.IDS_I32, 1, 3, -1, PL.SEG_NONE, 1, PL.ROWS_FROM_IDS, 0, None, 0, 1)
    return PlanSpec([c, g], [1, 1, 1, 1], [8, 4, w_esz, 4], n_device_inputs=2, n_symbols=1)


def _unchecked(spec):
    """Past the Python checks: what the library itself says."""
    spec = dataclasses.replace(spec, columns=[dataclasses.replace(c) for c in spec.columns])
    spec.validate = lambda: None
    for c in spec.columns:
        c.validate = lambda: None
    return spec


def test_plans_with_weights_and_sqrtn_are_accepted_and_malformed_ones_refused():
    from recom_amd.lib import FcpError
    from recom_amd.ops import Plan
    for combiner in (PL.COMBINER_SUM, PL.COMBINER_MEAN, PL.COMBINER_SQRTN):
        p = Plan(_spec(combiner, True), host_only=True)
        assert p.counts()["columns"] == 2
        p.close()
    Plan(_spec(PL.COMBINER_SQRTN, False), host_only=True).close()
    good = _spec()
    refusals = {
        "weights on a gather column": dataclasses.replace(good, columns=[good.columns[0], dataclasses.replace(good.columns[1], weights_input=2)]),
        "weights on a scatter column": _spec(PL.COMBINER_NONE, True, PL.FORM_GATHER_SCATTER),
        "weights input out of range": dataclasses.replace(good, columns=[dataclasses.replace(good.columns[0], weights_input=4), good.columns[1]]),
        "weights input negative": dataclasses.replace(good, columns=[dataclasses.replace(good.columns[0], weights_input=-3), good.columns[1]]),
        "weights of 8-byte elements": _spec(w_esz=8),
        "sqrtn on a gather column": dataclasses.replace(good, columns=[good.columns[0], dataclasses.replace(good.columns[1], combiner=PL.COMBINER_SQRTN)]),
        "sqrtn on a scatter column": _spec(PL.COMBINER_SQRTN, False, PL.FORM_GATHER_SCATTER),
        "combiner 4": _spec(4, False),
    }
    for what, spec in refusals.items():
        with pytest.raises(ValueError):
            spec.validate()
        with pytest.raises(FcpError) as e:
            Plan(_unchecked(spec), host_only=True)
        assert e.value.status == 1, (what, e.value)                   # FCP_ERR_INVALID_ARGUMENT
    # positional constructions keep their meaning: the new field comes last and defaults to "no weights"
    assert [f.name for f in dataclasses.fields(ColumnSpec)][-1] == "weights_input" and good.columns[1].weights_input == -1


def test_version_5_plan_files_round_trip_through_both_parsers(tmp_path):
    from recom_amd.lib import FcpError
    from recom_amd.ops import Plan
    from recom_amd.plan_io import load_plan, save_plan
    path = str(tmp_path / "w.fcp")
    for cell in (W.FormCell(4, "wmean", "csr"), W.FormCell(2, "wsqrtn", "idx64"), W.FormCell(1, "sqrtn", "ids32")):
        spec = W.form_case(cell).spec
        save_plan(spec, path)
        text = open(path).read()
        n_w = sum(c.weights_input >= 0 for c in spec.columns)
        assert text.startswith("fcp_plan 5\n") and f"\nweights {n_w}\n" in text, cell
        assert load_plan(path).to_dict().keys() == spec.to_dict().keys()
        assert _same_dict(load_plan(path).to_dict(), spec.to_dict()), cell
        p = Plan.from_file(path, host_only=True)
        assert p.counts()["columns"] == spec.n_columns
        p.close()
    # with a segment-id map and a stage section: one extension record carries map and weights
    from segmap_cases import build
    mapped, plain, *_ = build(1)
    cols = list(mapped.columns)
    cols[0] = dataclasses.replace(cols[0], weights_input=mapped.n_host_inputs)
    both = dataclasses.replace(mapped, columns=cols, host_input_ranks=list(mapped.host_input_ranks) + [1],
                               host_input_elem_sizes=list(mapped.host_input_elem_sizes) + [4])
    staged, stage = both.staged_for_concat_inputs()
    assert stage.modes[both.columns[0].weights_input] == PL.STAGE_COPY and staged.columns[0].weights_input == both.columns[0].weights_input
    save_plan(staged, path, stage)
    text = open(path).read()
    assert text.startswith("fcp_plan 5\n") and text.index("\nweights 1\n") < text.index("\nsegmaps ") < text.index("\nstage ")
    assert _same_dict(load_plan(path).to_dict(), staged.to_dict())
    Plan.from_file(path, host_only=True).close()
    # plans without the feature keep their version line and have no weights section
    for spec, stage_, version in ((plain, None, 2), (mapped, None, 4)):
        save_plan(spec, path, stage_)
        text = open(path).read()
        assert text.startswith(f"fcp_plan {version}\n") and "weights" not in text
    spec = W.form_case(W.FormCell(4, "wmean", "csr")).spec
    save_plan(spec, path)
    good = open(path).read()
    first = next(k for k, c in enumerate(spec.columns) if c.weights_input >= 0)
    n_w = sum(c.weights_input >= 0 for c in spec.columns)
    malformed = {
        "a column named twice": good.replace(f"weights {n_w}\n", f"weights {n_w + 1}\n{first} {spec.columns[first].weights_input}\n", 1),
        "an input out of range": good.replace(f"weights {n_w}\n{first} {spec.columns[first].weights_input}\n",
                                              f"weights {n_w}\n{first} {spec.n_host_inputs}\n", 1),
        "a column out of range": good.replace(f"weights {n_w}\n{first} ", f"weights {n_w}\n{spec.n_columns} ", 1),
        "a weights section in a version-4 file": good.replace("fcp_plan 5\n", "fcp_plan 4\n", 1),
    }
    for what, text in malformed.items():
        assert text != good, what
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises((ValueError, AssertionError)):
            load_plan(path)
        with pytest.raises(FcpError):
            Plan.from_file(path, host_only=True)


def _same_dict(a, b) -> bool:
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_dict(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_dict(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def test_weights_inputs_are_renumbered_staged_and_counted():
    case = W.form_case(W.FormCell(4, "wmean", "ids32"))
    spec = case.spec
    inputs, symbols = case.requests[0]
    # column_subset: the weights input is renumbered with the others
    keep = [k for k, c in enumerate(spec.columns) if c.weights_input >= 0][1:] + [1]
    sub = spec.column_subset(keep)
    sub.spec.validate()
    for c_sub, k in zip(sub.spec.columns, keep):
        c = spec.columns[k]
        assert (c_sub.weights_input >= 0) == (c.weights_input >= 0)
        if c.weights_input >= 0:
            assert sub.host_inputs[c_sub.weights_input] == c.weights_input
            assert sub.spec.host_input_elem_sizes[c_sub.weights_input] == 4
        assert sub.host_inputs[c_sub.ids_input] == c.ids_input
    from recom_amd.ops import Plan
    Plan(sub.spec, host_only=True).close()
    # staged(): weights travel as plain copies; the segment ids next to them still become row offsets
    staged, modes, _ = spec.staged()
    for c0, c1 in zip(spec.columns, staged.columns):
        if c0.weights_input >= 0:
            assert modes[c0.weights_input] == PL.STAGE_COPY and c1.weights_input == c0.weights_input
            assert modes[c0.seg_input] == PL.STAGE_SEG_TO_CSR and c1.seg_kind == PL.SEG_CSR_I32
    # a tensor that one column reads as weights is never converted to row offsets for another
    cols = list(spec.columns)
    w0 = next(k for k, c in enumerate(cols) if c.weights_input >= 0)
    other = next(k for k, c in enumerate(cols) if c.form == PL.FORM_SEGMENT_REDUCE and k != w0)
    cols[w0] = dataclasses.replace(cols[w0], weights_input=cols[other].seg_input)
    _, modes2, _ = dataclasses.replace(spec, columns=cols).staged()
    assert modes2[cols[other].seg_input] == PL.STAGE_COPY
    # algorithmic bytes: + 4 B per id of every weighted column, nothing else
    from recom_amd.ops import concat_inputs
    shapes = concat_inputs(inputs)[2]
    plain = dataclasses.replace(spec, columns=[dataclasses.replace(c, weights_input=-1) for c in spec.columns])
    a, b = spec.algorithmic_bytes(shapes, symbols), plain.algorithmic_bytes(shapes, symbols)
    nnz = sum(np.asarray(inputs[c.ids_input]).size for c in spec.columns if c.weights_input >= 0)
    assert nnz > 0 and a["total"] - b["total"] == 4 * nnz == a["weights"] and a["read"] - b["read"] == 4 * nnz
    assert "weights" not in b and {k: v for k, v in a.items() if k not in ("weights", "read", "total")} == \
        {k: v for k, v in b.items() if k not in ("read", "total")}


FINITE = list(W.all_weighted_cases())


@pytest.mark.parametrize("cid,case,weighted", FINITE, ids=[c[0] for c in FINITE])
def test_restatement_against_float64_and_the_fused_variant(cid, case, weighted):
    """Every cell of the form and id-path matrices (finite inputs): the float32 restatement lies within the derived
    rounding bound of the float64 restatement, no element is NaN (nothing is compared as "is NaN" in these cells), and —
    weighted cells — at least 10 % of the elements of bags with two or more ids differ in bits from the contracted variant
    fl32(acc + w * x): a kernel that fuses the multiply into the add cannot pass them."""
    for t in (0, 1):
        inputs, symbols = case.requests[t]
        got = W.restate(case.spec, case.tables, inputs, symbols)
        truth = W.restate(case.spec, case.tables, inputs, symbols, f64=True)
        bound = W.float64_bound(case.spec, case.tables, inputs, symbols)
        assert got.bad == truth.bad
        for g in range(case.spec.n_groups):
            m = got.pooled[g]
            err = np.abs(got.groups[g][:, m].astype(np.float64) - truth.groups[g][:, m])
            assert (err <= bound[g][:, m]).all(), (cid, t, float((err - bound[g][:, m]).max()))
            assert np.array_equal(E_bits(got.groups[g][:, ~m]), E_bits(truth.groups[g][:, ~m].astype(np.float32)))
        assert W.nan_share(case.spec, got) == 0.0
        if weighted:
            share = W.fused_share(case.spec, case.tables, inputs, symbols)
            print(f"{cid} request {t}: {share:.3f} of the elements tell the fused variant apart")
            assert share >= 0.10, (cid, t, share)


def E_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_form_cells_cover_the_edge_lengths_and_the_long_bags():
    from kernel_variant_cases import CAPW, EDGE_LENS
    for cell in W.form_cells():
        case = W.form_case(cell)
        assert set(EDGE_LENS) <= case.lens_seen and {CAPW + 1, 1000} <= case.lens_seen, (cell.id, sorted(case.lens_seen))
        inputs, symbols = case.requests[0]
        span0 = [c for k, c in enumerate(case.spec.columns) if k <= 6]
        for r, total in ((2, CAPW), (3, CAPW + 1)):                  # the ids a wave of span 0 stages for this row
            n = sum(1 if c.form == PL.FORM_GATHER else
                    int(np.diff(W.row_offsets(c, inputs[c.seg_input], int(symbols[0])))[r]) if c.form == PL.FORM_SEGMENT_REDUCE else 0
                    for c in span0)
            assert n == total, (cell.id, r, n)
        assert all(int(np.diff(W.row_offsets(c, inputs[c.seg_input], int(symbols[0])))[1]) == 0
                   for c in case.spec.columns if c.form == PL.FORM_SEGMENT_REDUCE)


def test_weighted_sum_against_pytorch_embedding_bag():
    """PyTorch-CPU embedding_bag(mode="sum", per_sample_weights) — the one weighted form it has — within the float64 bound
    of the restatement."""
    import torch
    import torch.nn.functional as F
    for enc in W.ENCODINGS:
        case = W.form_case(W.FormCell(4, "wsum", enc))
        inputs, symbols = case.requests[0]
        got = W.restate(case.spec, case.tables, inputs, symbols).groups[0]
        bound = W.float64_bound(case.spec, case.tables, inputs, symbols)[0]
        offs = case.spec.column_offsets()
        checked = 0
        for k, c in enumerate(case.spec.columns):
            if c.weights_input < 0:
                continue
            o = W.row_offsets(c, inputs[c.seg_input], int(symbols[0]))
            ref = F.embedding_bag(torch.from_numpy(np.asarray(inputs[c.ids_input], np.int64)), torch.from_numpy(case.tables[c.table_input]),
                                  torch.from_numpy(np.asarray(o[:-1], np.int64)), mode="sum",
                                  per_sample_weights=torch.from_numpy(np.asarray(inputs[c.weights_input], np.float32))).numpy()
            sl = slice(offs[k], offs[k] + c.dim)
            err = np.abs(got[:, sl].astype(np.float64) - ref.astype(np.float64))
            assert (err <= bound[:, sl]).all(), (enc, k, float((err - bound[:, sl]).max()))
            checked += 1
        assert checked == 4


def test_unweighted_sqrtn_equals_the_tf_graph_evaluator_bit_for_bit():
    """oracle/tf_graph_eval.py evaluates SparseSegmentSqrtN as a sum in id order divided by the float32 square root of the
    float32 count: the restatement must produce the same bits."""
    import tf_graph_eval
    ev = tf_graph_eval.GraphEvaluator(types.SimpleNamespace(node=[]))
    checked = 0
    for vec in W.VECS:
        case = W.form_case(W.FormCell(vec, "sqrtn", "ids32"))
        inputs, symbols = case.requests[0]
        got = W.restate(case.spec, case.tables, inputs, symbols).groups[0]
        offs = case.spec.column_offsets()
        for k, c in enumerate(case.spec.columns):
            if c.combiner != PL.COMBINER_SQRTN:
                continue
            node = types.SimpleNamespace(op="SparseSegmentSqrtN", attr={}, name=f"col{k}")
            ref = ev._eval(node, [case.tables[c.table_input], inputs[c.ids_input], inputs[c.seg_input]])[0]
            want = np.zeros((int(symbols[0]), c.dim), np.float32)
            want[:ref.shape[0]] = ref                                  # (trailing rows without ids: zeros)
            assert np.array_equal(E_bits(got[:, offs[k]:offs[k] + c.dim]), E_bits(want)), (vec, k)
            checked += 1
    assert checked == 12


def test_weight_value_cells_keep_nan_rows_a_small_share():
    """The special-value cells: elements whose expectation is NaN (compared as "is NaN") are at most a quarter; the row whose
    weights cancel is +0.0 under MEAN with a non-zero numerator; all-zero weights give +0.0 rows."""
    for vec in W.VECS:
        case = W.value_case(vec)
        for t in (0, 1):
            res = W.restate(case.spec, case.tables, *case.requests[t])
            share = W.nan_share(case.spec, res)
            assert 0 < share <= 0.25, (vec, t, share)
        res = W.restate(case.spec, case.tables, *case.requests[0])
        out = res.groups[0]
        r_cancel, r_zero = W.SCENARIOS.index("cancel"), W.SCENARIOS.index("all_zero")
        wsum, wmean, wsqrtn = slice(0, 3 * vec), slice(3 * vec, 8 * vec), slice(8 * vec, 15 * vec)
        assert (out[r_cancel, wsum] != 0).all() and (E_bits(out[r_cancel, wmean]) == 0).all() and (out[r_cancel, wsqrtn] != 0).all()
        assert (E_bits(out[r_zero]) == 0).all()
        assert np.isposinf(out[W.SCENARIOS.index("overflow_order")]).all()


def test_weighted_kernels_fit_the_occupancy_budget(tmp_path):
    """The code object of fcp_weighted.hip (gfx950, no GPU needed): six instantiations — V in {1, 2, 4} x SHARDED, what
    fcp_launch_weighted can reach — each at most 64 VGPRs (8 waves per SIMD) for EVERY V, no scratch, at most 20 480 B of
    LDS (8 blocks per CU), fp32 subnormals kept, IEEE mode, and — the unsharded ones, which divide — the IEEE division
    sequence and the correctly rounded square root.  (Held by their own name: the tests of the other fused kernels match `fcp_ragged_kernel` and friends.)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    asm = tmp_path / "w.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                        os.path.join(ROOT, "recom_amd", "csrc", "fcp_weighted.hip"), "-o", str(asm)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    seen = set()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        name, desc = m.group(1), m.group(2)
        k = re.search(r"fcp_weighted_bag_kernelILi(\d)ELb([01])E", name)
        assert k, f"unexpected kernel {name} in fcp_weighted.hip"
        seen.add((int(k.group(1)), bool(int(k.group(2)))))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        assert vgpr <= 64, f"{name}: {vgpr} VGPRs"
        assert scratch == 0, f"{name}: uses scratch"
        assert lds <= 20480, f"{name}: {lds} bytes of LDS"
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", desc), f"{name}: fp32 subnormals are flushed"
        assert re.search(r"\.amdhsa_ieee_mode 1\b", desc), f"{name}: not in IEEE mode"
        label = re.search(r"^" + re.escape(name) + r":", text, re.M)
        body = text[label.end():m.start()]
        if not int(k.group(2)):
            assert "v_div_scale_f32" in body and "v_div_fixup_f32" in body, f"{name}: not an IEEE division"
            # the correctly rounded square root: v_sqrt_f32 (1 ulp) and its correction by two fused residuals — the bare
            # instruction (what __fsqrt_rn compiles to) fails here
            sq = body.find("v_sqrt_f32")
            assert sq >= 0 and body[sq:sq + 600].count("v_fma_f32") >= 2, f"{name}: the square root is not correctly rounded"
        assert "v_mul_f32" in body or "v_pk_mul_f32" in body, f"{name}: no separate product"
    assert seen == {(v, s) for v in (1, 2, 4) for s in (False, True)}, seen
