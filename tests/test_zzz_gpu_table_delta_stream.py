"""fcp_table_delta_distinct and tables.apply_delta on a non-default stream (kernels: recom_amd/csrc/fcp_table_delta.hip).

A file of its own that sorts behind tests/test_z_gpu_private_streams.py, for the reason tests/test_zzz_gpu_table_convert_stream.py
gives: a stream taken from torch's pool shifts which hardware queue later streams are mapped to, the one thing the
private-stream tests depend on and cannot see.  Behind them it disturbs nothing."""
import numpy as np
import pytest

import table_convert_cases as TC
import table_delta_cases as D
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
    """On a non-default stream, with no synchronisation in between: delta_distinct_async, update_rows and digest_rows of its
    padded outputs, then apply_delta of a second repeating delta with the digest kept.  Stream order is all there is; the q8
    table and the digests are those of the restatements."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    dim, table_rows, n = 12, 900, D.MIN_CHUNK + D.TILE + 1
    master = TC.family_rows(dim, table_rows, 8)
    deltas = []
    for seed in (1, 2):
        ids = D.draw_ids("hot_head", n, table_rows, seed=seed)
        ids[3::29] = -1
        deltas.append((ids, TC.family_rows(dim, n, 9 + seed)))
    pos, report, ids_out, _p = D.distinct_ref(deltas[0][0], table_rows)
    assert report["duplicates"] > 0 and report["skipped"] > 0
    after_one = D.apply_ref(master, *deltas[0])
    after_two = D.apply_ref(after_one, *deltas[1])
    digest_one = tables.digest_host(R.expect_bytes(after_one, "q8"), "q8", dim=dim)      # of the table between the two deltas
    table = tables.convert(torch.from_numpy(master).to(dev), "q8")
    d = [(torch.from_numpy(i).to(dev), torch.from_numpy(r).to(dev)) for i, r in deltas]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    with torch.cuda.stream(stream):
        ids_d, rows_d, report_d = tables.delta_distinct_async(*d[0], table_rows=table_rows, stream=stream.cuda_stream)
        tables.update_rows(table, ids_d, rows_d)                     # the wrapper's default: torch's current stream
        mid = table.clone()
        got_report, digest_two = tables.apply_delta(table, *d[1], digest=digest_one, stream=stream.cuda_stream)
    stream.synchronize()
    assert report_d.cpu().tolist() == [n, report["distinct"], report["duplicates"], report["skipped"]]
    assert (ids_d.cpu().numpy() == ids_out).all()
    assert (rows_d.cpu().numpy()[:len(pos)].view(np.uint32) == deltas[0][1][pos].view(np.uint32)).all()
    assert (mid.cpu().numpy() == R.expect_bytes(after_one, "q8")).all()
    want = R.expect_bytes(after_two, "q8")
    assert (table.cpu().numpy() == want).all()
    assert got_report == tables.DeltaReport(**D.distinct_ref(deltas[1][0], table_rows)[1])
    assert digest_two == tables.digest_host(want, "q8", dim=dim) == tables.digest(table)
