"""fcp_table_update_rows / fcp_table_read_rows on a non-default stream, and the loader that streams a host delta through a
pinned buffer (kernels: recom_amd/csrc/fcp_table_rows.hip).

A file of its own that sorts behind tests/test_z_gpu_private_streams.py, for the reason tests/test_zzz_gpu_table_convert_stream.py gives: a stream taken
from torch's pool and asynchronous copies out of pinned memory shift which hardware queue later streams are mapped to, the
one thing the private-stream tests depend on and cannot see.  Behind them it disturbs nothing."""
import numpy as np
import pytest

import table_convert_cases as TC
import table_rows_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def test_stream_order(torch_cuda):
    """On a non-default stream, with no synchronisation in between: update_rows, then read_rows, then the plan of the small
    model on the updated q8 tables.  Stream order is all there is, and the results are those of the synchronised run
    (tests/test_gpu_table_rows.py::test_plan_on_an_updated_table): the restatement's tables, their dequantised rows, the
    float32 plan on them."""
    torch = torch_cuda
    from recom_amd import synth, tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    dev = torch.device("cuda", 0)
    spec, masters, deltas, (inputs, symbols) = R.small_model()
    want_q8, want_deq = R.small_model_expected_tables(masters, deltas)
    op, op32 = FeatureColumnProcess(spec.with_table_dtype("q8"), 0), FeatureColumnProcess(spec, 0)
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    q8 = [tables.convert(torch.from_numpy(m).to(dev), "q8") for m in masters]
    d_deltas = [(torch.from_numpy(i).to(dev), torch.from_numpy(r).to(dev)) for i, r in deltas]
    ref = op32(d_blob, offsets, shapes, [torch.from_numpy(w).to(dev) for w in want_deq], symbols)
    torch.cuda.synchronize()
    want = ref.groups[0].cpu().numpy()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    with torch.cuda.stream(stream):
        for t, (i, r) in zip(q8, d_deltas):
            tables.update_rows(t, i, r, stream=stream.cuda_stream)
        back = [tables.read_rows(t, i) for t, (i, _r) in zip(q8, d_deltas)]      # the wrapper's default: torch's current stream
        out = op(d_blob, offsets, shapes, q8, symbols, stream=stream.cuda_stream)
    stream.synchronize()
    for t, w, b, (ids, _rows) in zip(q8, want_q8, back, deltas):
        assert (t.cpu().numpy() == w).all()
        assert (b.cpu().numpy().view(np.uint32) == synth.dequantize_q8(w[ids]).view(np.uint32)).all()
    got = out.groups[0].cpu().numpy()
    assert np.abs(want).max() > 0 and (got.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("kind", ("q8", "bf16"))
def test_update_from_host_streams_chunks(torch_cuda, kind):
    """A host delta through one pinned bounce buffer, in chunks that do not divide n: the table equals the one-call update
    and the restatement.  dim 7: q8 rows start at every byte alignment."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    dim, n, table_rows = 7, 1000, 1500
    x = TC.quant_rows(dim)
    ids = R.distinct_ids(n, table_rows, 12)
    assert n % 301 and len(set(ids.tolist())) == n
    _buf1, one = R.poisoned(torch, kind, dim, table_rows, dev)
    buf2, chunked = R.poisoned(torch, kind, dim, table_rows, dev)
    tables.update_rows(one, torch.from_numpy(ids).to(dev), torch.from_numpy(x.copy()).to(dev))
    assert tables.update_from_host(chunked, torch.from_numpy(ids), torch.from_numpy(x.copy()), chunk_rows=301) is chunked
    torch.cuda.synchronize()
    assert bool((_buf1 == buf2).all())
    R.check_poisoned(buf2, kind, dim, table_rows, ids, R.expect_bytes(x, kind), (kind, "update_from_host"))
