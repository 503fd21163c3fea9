"""fcp_table_diff chained into fcp_table_digest_rows and fcp_table_update_rows on a non-default stream, and the host-streaming
wrappers tables.diff_from_host / tables.sync_from_host (kernels: recom_amd/csrc/fcp_table_diff.hip).

A file of its own that sorts behind tests/test_z_gpu_private_streams.py, for the reason tests/test_zzz_gpu_table_convert_stream.py
gives: a stream taken from torch's pool shifts which hardware queue later streams are mapped to, the one thing the
private-stream tests depend on and cannot see.  Behind them it disturbs nothing."""
import numpy as np
import pytest

import table_diff_cases as D

pytestmark = pytest.mark.gpu

KINDS = tuple(D.KINDS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _masters(table_rows: int, dim: int, seed: int):
    """(served master, new master, the rows meant to change): every third row and the tiles' edges loud, the rest as served"""
    old = D.base_rows(table_rows, dim, seed=seed)
    mask = D.mask_of("every3", table_rows) | D.mask_of("tile_edges", table_rows) | D.mask_of("last", table_rows)
    return old, np.where(mask[:, None], D.loud(old), old), mask


def _bytes_of(torch, t):
    return t.cpu().contiguous().view(torch.uint8).numpy().reshape(t.shape[0], -1)


@pytest.mark.parametrize("kind", KINDS)
def test_diff_digest_update_digest_in_stream_order(torch_cuda, kind):
    """On a non-default stream, with no host read in between: diff -> digest_rows -> update_rows -> digest_rows of the padded
    outputs.  The table then equals tables.convert(new master) byte for byte, the carried digest is tables.digest of the
    result, and a second diff reports nothing."""
    torch = torch_cuda
    import ctypes as C
    from recom_amd import lib, tables
    L = lib.load()
    dev = torch.device("cuda", 0)
    dim, table_rows = 12, 2 * D.MIN_CHUNK + D.TILE + 1
    old, new, mask = _masters(table_rows, dim, seed=4)
    want_ids, want_report, want_ids_out = D.diff_ref(D.ref_bytes(new, kind), D.ref_bytes(old, kind))
    assert want_ids.tolist() == np.flatnonzero(mask).tolist()
    d_old, d_new = torch.from_numpy(old).to(dev), torch.from_numpy(new).to(dev)
    table = d_old.clone() if kind == "f32" else tables.convert(d_old, kind)
    want_table = d_new.clone() if kind == "f32" else tables.convert(d_new, kind)
    digest_before = tables.digest(table)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        outs, workspace = tables._digest_buffers(torch, L, dev, s, n_out=2)
        size = C.sizeof(lib.TableDigest)
        ids_d, rows_d, report_d = tables.diff_async(table, d_new, stream=s)
        tables._enqueue_digest_rows(L, table, kind, dim, ids_d, table_rows, 0, 1, outs.data_ptr(), workspace, s)
        tables.update_rows(table, ids_d, rows_d)                     # the wrapper's default: torch's current stream
        tables._enqueue_digest_rows(L, table, kind, dim, ids_d, table_rows, 0, 1, outs.data_ptr() + size, workspace, s)
        _ids2, _rows2, report2_d = tables.diff_async(table, d_new, stream=s)
    stream.synchronize()
    assert report_d.cpu().tolist() == [table_rows, want_report["changed"], want_report["first_changed"], want_report["last_changed"]]
    assert (ids_d.cpu().numpy() == want_ids_out).all()
    assert (rows_d.cpu().numpy()[:len(want_ids)].view(np.uint32) == new.view(np.uint32)[want_ids]).all()
    assert (_bytes_of(torch, table) == _bytes_of(torch, want_table)).all() and (_bytes_of(torch, table) == D.ref_bytes(new, kind)).all()
    before, after = tables._digests_of(outs)
    assert before.rows == after.rows == len(want_ids) and before.skipped == after.skipped == table_rows - len(want_ids)
    carried = (digest_before - int(before.sum) + int(after.sum)) % (1 << 64)
    assert carried == tables.digest(table) == tables.digest_host(D.ref_bytes(new, kind), kind, dim=dim) and carried != digest_before
    assert report2_d.cpu().tolist() == [table_rows, 0, -1, -1]


@pytest.mark.parametrize("kind", KINDS)
def test_diff_and_sync_from_host(torch_cuda, kind):
    """chunk_rows smaller than the table and no divisor of it: diff_from_host returns the concatenated delta of the whole
    table; sync_from_host rewrites exactly those rows, carries the digest, and leaves nothing for a second pass."""
    torch = torch_cuda
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    dim, table_rows, chunk_rows = 20, D.MIN_CHUNK + 2 * D.TILE + 9, 700
    assert table_rows % chunk_rows and chunk_rows < table_rows
    old, new, mask = _masters(table_rows, dim, seed=6)
    want_ids, want_report, _o = D.diff_ref(D.ref_bytes(new, kind), D.ref_bytes(old, kind))
    d_old = torch.from_numpy(old).to(dev)
    table = d_old.clone() if kind == "f32" else tables.convert(d_old, kind)
    new_cpu = torch.from_numpy(new)
    ids, rows, report = tables.diff_from_host(table, new_cpu, chunk_rows=chunk_rows)
    assert report == tables.DiffReport(**want_report)
    assert ids.cpu().numpy().tolist() == want_ids.tolist() and rows.shape == (len(want_ids), dim)
    assert (rows.cpu().numpy().view(np.uint32) == new.view(np.uint32)[want_ids]).all()
    assert (_bytes_of(torch, table) == D.ref_bytes(old, kind)).all()                     # the table is only read
    before = tables.digest(table)
    changed, after = tables.sync_from_host(table, new_cpu, digest=before, chunk_rows=chunk_rows)
    assert changed == len(want_ids)
    assert (_bytes_of(torch, table) == D.ref_bytes(new, kind)).all()
    assert after == tables.digest(table) == tables.digest_host(D.ref_bytes(new, kind), kind, dim=dim) and after != before
    assert tables.sync_from_host(table, new_cpu, chunk_rows=chunk_rows) == 0            # in step: nothing is rewritten
    ids, rows, report = tables.diff_from_host(table, new_cpu, chunk_rows=table_rows + 5)
    assert report == tables.DiffReport(table_rows, 0, -1, -1) and ids.shape == (0,) and rows.shape == (0, dim)
    # back to the served master without a digest, one chunk for the whole table
    assert tables.sync_from_host(table, torch.from_numpy(old), chunk_rows=1 << 16) == len(want_ids)
    assert (_bytes_of(torch, table) == D.ref_bytes(old, kind)).all()
