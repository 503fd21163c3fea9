"""float32 tables converted on the device (fcp_table_convert), then served: the plan kernels this file runs are the existing
ones (fcp_tables_q8.hip, fcp_tables16.hip, fcp_kernels.hip); what is new is where their tables come from.

For one dense, one ragged and one hybrid plan of the variant cells (narrow_output_cases.DISCRIMINATION_KEYS) and each of q8 /
bf16 / fp16: the converted tables are the bytes the CPU restatement gives; the plan on them equals, bit for bit, the float32
plan on the tables fcp_table_convert widens back; and for q8 every sum-pooled column stays within the sum over the bag of the
per-element bound 0.5 * scale + 1e-8 + 2^-22 * max(|mn|, |mx|) (tests/test_table_convert_host.py) of the float32 plan on the
ORIGINAL tables.  (That bound is the issue's: it leaves out the float32 rounding of the two sums themselves, at most
2 (n - 1) 2^-24 sum|x| for a bag of n — five orders of magnitude below the 0.5 * scale term of these Gaussian tables.)"""
import numpy as np
import pytest

import kernel_variant_cases as K
import narrow_output_cases as N
import table16_cases as T16
import table_convert_cases as TC
from recom_amd import synth
from recom_amd.plan import COMBINER_SUM, FORM_SEGMENT_REDUCE, SEG_CSR_I32

pytestmark = pytest.mark.gpu

KEYS = N.DISCRIMINATION_KEYS
assert [k[0] for k in KEYS] == ["dense", "ragged", "hybrid"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _bag_bound(col, inputs, symbols, table: np.ndarray) -> np.ndarray:
    """float64 [rows]: the sum over each bag of the per-element bound of the rows its ids name (ids outside the vocabulary
    read zeros in both plans: no term)."""
    ids = np.asarray(inputs[col.ids_input]).astype(np.int64).reshape(-1)
    rows = int(symbols[col.rows_arg])
    if col.seg_kind == SEG_CSR_I32:
        off = np.asarray(inputs[col.seg_input]).astype(np.int64)
        seg = np.repeat(np.arange(rows), np.diff(off[:rows + 1]))
        ids = ids[off[0]:off[rows]]
    else:
        seg = np.asarray(inputs[col.seg_input]).astype(np.int64).reshape(-1)[::col.seg_stride][:len(ids)]
    ok = (ids >= 0) & (ids < col.vocab) & (seg >= 0) & (seg < rows)
    per_row = TC.error_bound(table)
    out = np.zeros(rows, np.float64)
    np.add.at(out, seg[ok], per_row[ids[ok]])
    return out


@pytest.mark.parametrize("dtype", ("q8", "bf16", "f16"))
@pytest.mark.parametrize("key", KEYS, ids=[k[0] for k in KEYS])
def test_plans_on_tables_converted_on_the_device(torch_cuda, key, dtype):
    torch = torch_cuda
    from recom_amd import tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    case = K.build_case(*key)
    spec32 = case.spec
    dev = torch.device("cuda", 0)
    tabs32 = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in case.tables]
    conv = tables.convert_tables(spec32, tabs32, dtype)
    wide = [tables.convert(t, "f32") for t in conv]
    # the converted tables are what the CPU says they are
    for i, (t32, c, w) in enumerate(zip(case.tables, conv, wide)):
        if dtype == "q8":
            want = TC.quantize_ref(t32)
            assert (c.cpu().numpy() == want).all(), (key, i)
            T16.assert_same_bits(w.cpu().numpy(), synth.dequantize_q8(want), (key, dtype, "widened", i))
        else:
            bits = c.cpu().view(torch.int16).numpy().view(np.uint16)
            assert (bits == N.narrow(t32, dtype)).all(), (key, dtype, i)
            T16.assert_same_bits(w.cpu().numpy(), T16.widen(bits, dtype), (key, dtype, "widened", i))
    op = FeatureColumnProcess(spec32.with_table_dtype(dtype), 0)
    op32 = FeatureColumnProcess(spec32, 0)
    assert op.plan.table_dtype() == dtype and op32.plan.table_dtype() == "f32"
    pooled = [k for k, c in enumerate(spec32.columns)
              if c.form == FORM_SEGMENT_REDUCE and c.combiner == COMBINER_SUM and not c.xform_mode]
    assert pooled or key[0] == "dense"
    for t, (inputs, symbols) in enumerate(case.requests):
        blob, offsets, shapes = concat_inputs(inputs)
        d_blob = torch.from_numpy(blob).to(dev)
        out = op(d_blob, offsets, shapes, conv, symbols)
        ref = op32(d_blob, offsets, shapes, wide, symbols)
        torch.cuda.synchronize()
        assert op.plan.last_launch()["kernel"] == key[0] + ("_tabq8" if dtype == "q8" else "_tab16")
        for g in range(spec32.n_groups):
            got, want = out.groups[g].cpu().numpy(), ref.groups[g].cpu().numpy()
            assert not np.isnan(want).any()
            assert T16.assert_same_bits(got, want, (key, dtype, t, "group", g)) == 0
        if dtype != "q8" or not pooled:
            continue
        orig = op32(d_blob, offsets, shapes, tabs32, symbols)
        torch.cuda.synchronize()
        for k in pooled:
            c = spec32.columns[k]
            bound = _bag_bound(c, inputs, symbols, case.tables[c.table_input])
            err = np.abs(out.column(k).cpu().numpy().astype(np.float64) - orig.column(k).cpu().numpy().astype(np.float64))
            assert err.shape == (len(bound), c.dim)
            worst = float((err / np.maximum(bound, 1e-300)[:, None]).max()) if err.size else 0.0
            print(f"{key[0]} request {t} column {k}: largest |q8 sum - float32 sum| / bound = {worst:.3f}")
            assert (err <= bound[:, None]).all(), (key, t, k, worst)
