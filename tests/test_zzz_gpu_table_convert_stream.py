"""fcp_table_convert on a non-default stream, and the loader that streams a host table through a pinned buffer (kernels:
recom_amd/csrc/fcp_convert.hip).

A file of its own that sorts behind tests/test_z_gpu_private_streams.py: the first test takes a stream from torch's pool, the second makes the
process's first asynchronous copies out of pinned memory, and every stream or queue a process creates or takes shifts which hardware queue the later ones are mapped to — the one thing the private-stream
tests of that file depend on and cannot see (include/fcp_hip.h, "Verification").  Behind them it disturbs nothing."""
import numpy as np
import pytest

import narrow_output_cases as N
import table16_cases as T16
import table_convert_cases as TC
from recom_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def test_non_default_stream(torch_cuda):
    """A conversion on a non-default stream, read on that stream: the reader sees the result with no device
    synchronisation in between (the stream's order is all there is)."""
    torch = torch_cuda
    from recom_amd import tables
    dim, rows = 64, 1 << 16
    x = TC.family_rows(dim, 1000, 5)
    x = np.tile(x, (rows // 1000 + 1, 1))[:rows]
    src = torch.from_numpy(x).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=src.device)
    assert stream.cuda_stream != torch.cuda.default_stream(src.device).cuda_stream
    out = torch.zeros((rows, dim + 8), dtype=torch.uint8, device=src.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        tables.convert(src, "q8", out=out, stream=stream.cuda_stream)
        copy = out.clone()                                        # enqueued on `stream`, behind the conversion
        back = tables.convert(copy, "f32")                        # the wrapper's default: torch's current stream
    stream.synchronize()
    want = TC.quantize_ref(x)
    assert (copy.cpu().numpy() == want).all()
    T16.assert_same_bits(back.cpu().numpy(), synth.dequantize_q8(want), "stream, back")


@pytest.mark.parametrize("dtype", ("q8", "bf16"))
def test_convert_from_host_streams_chunks_to_their_rows(torch_cuda, dtype):
    """A host table through one pinned bounce buffer, in chunks that do not divide the row count; dim 7: q8 chunks land at
    byte offsets that are no multiples of 4, which only dst_row0 can express."""
    torch = torch_cuda
    from recom_amd import tables
    dim = 7
    x = TC.quant_rows(dim)
    got = tables.convert_from_host(torch.from_numpy(x.copy()), dtype, "cuda:0", chunk_rows=301)
    torch.cuda.synchronize()
    if dtype == "q8":
        assert (got.cpu().numpy() == TC.quant_expectation(dim)).all()
    else:
        assert (got.cpu().view(torch.int16).numpy().view(np.uint16) == N.narrow(x, dtype)).all()
