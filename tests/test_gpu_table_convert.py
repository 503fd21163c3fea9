"""fcp_table_convert on the GPU (kernels: recom_amd/csrc/fcp_convert.hip).  Every expectation is computed on the CPU — by the
restatement tests/test_table_convert_host.py pins to quantized::embedding_bag_byte_prepack, by synth.dequantize_q8, by torch's
CPU casts — and compared as bytes; nothing has a tolerance.  Only the convert kernels run here (the plans on converted tables:
tests/test_gpu_table_convert_plans.py; a call on a non-default stream and the pinned-buffer loader: tests/test_zzz_gpu_table_convert_stream.py)."""
import numpy as np
import pytest

import narrow_output_cases as N
import table16_cases as T16
import table_convert_cases as TC
from recom_amd import synth

pytestmark = pytest.mark.gpu

POISON = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from recom_amd import lib
    lib.load()  # fail loudly if the HIP extension is missing
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))      # (a copy: the cases' arrays are read-only)


def _same_rows(got: np.ndarray, want: np.ndarray, what) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).reshape(got.shape[0], -1).any(axis=1))[:, 0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} rows differ, first row {bad[0]}: {got[bad[0]]} want {want[bad[0]]}"


@pytest.mark.parametrize("dim", TC.QUANT_DIMS, ids=[f"dim{d}-V{TC.vec_of(d)}-G{TC.group_of(d)}" for d in TC.QUANT_DIMS])
def test_quantiser_cells(torch_cuda, dim):
    """float32 -> q8 at one dim, for every row count of TC.QUANT_ROWS (row groups straddle wave and block ends, the last
    block is partial): the bytes of the restatement, and not a byte behind the last row."""
    torch = torch_cuda
    from recom_amd import tables
    src = _dev(torch, TC.quant_rows(dim))
    want = TC.quant_expectation(dim)
    for rows in TC.QUANT_ROWS:
        out = torch.full((rows + 3, dim + 8), POISON, dtype=torch.uint8, device=src.device)
        assert tables.convert(src[:rows], "q8", out=out) is out
        got = out.cpu().numpy()
        _same_rows(got[:rows], want[:rows], ("q8", dim, rows))
        assert (got[rows:] == POISON).all(), (dim, rows, "bytes behind the last row were written")
    fresh = tables.convert(src[:65], "q8")                      # the allocating form
    assert fresh.dtype == torch.uint8 and tuple(fresh.shape) == (65, dim + 8)
    _same_rows(fresh.cpu().numpy(), want[:65], ("q8 fresh", dim))


@pytest.mark.parametrize("dim", (7, 6), ids=["odd", "2mod4"])
def test_dst_row0(torch_cuda, dim):
    """Rows [0, 37) and [37, 100) in two calls equal the one-call result — a q8 row of these dims is 15 / 14 bytes, so row
    37 starts at no multiple of 4; and with dst_row0 = 5 into a zeroed 20-row table the rows outside the range stay zero."""
    torch = torch_cuda
    from recom_amd import tables
    x = TC.quant_rows(dim)[:100]
    src = _dev(torch, x)
    want = TC.quant_expectation(dim)[:100]
    one = tables.convert(src, "q8")
    two = torch.full((100, dim + 8), POISON, dtype=torch.uint8, device=src.device)
    tables.convert(src[:37], "q8", out=two, dst_row0=0)
    tables.convert(src[37:], "q8", out=two, dst_row0=37)
    _same_rows(one.cpu().numpy(), want, ("one call", dim))
    _same_rows(two.cpu().numpy(), want, ("two calls", dim))
    small = torch.zeros((20, dim + 8), dtype=torch.uint8, device=src.device)
    tables.convert(src[:9], "q8", out=small, dst_row0=5)
    got = small.cpu().numpy()
    _same_rows(got[5:14], want[:9], ("dst_row0 5", dim))
    assert (got[:5] == 0).all() and (got[14:] == 0).all()
    for dtype, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16)):      # the 16-bit directions take dst_row0 too
        t = torch.zeros((20, dim), dtype=tdt, device=src.device)
        tables.convert(src[:9], dtype, out=t, dst_row0=5)
        g = t.cpu().view(torch.int16).numpy().view(np.uint16)
        assert (g[5:14] == N.narrow(x[:9], dtype)).all() and (g[:5] == 0).all() and (g[14:] == 0).all()
    back = torch.zeros((20, dim), dtype=torch.float32, device=src.device)
    tables.convert(one[:9], "f32", out=back, dst_row0=5)
    g = back.cpu().numpy()
    T16.assert_same_bits(g[5:14], synth.dequantize_q8(want[:9]), ("q8 -> f32, dst_row0", dim))
    assert (g[:5] == 0).all() and (g[14:] == 0).all()


@pytest.mark.parametrize("dim", (1, 3, 4, 6, 64))
def test_dequantise_arbitrary_bytes(torch_cuda, dim):
    """q8 -> float32 on random bytes (scales and biases of every kind, NaN and infinity among them) equals
    synth.dequantize_q8 bit for bit; both NaN counts as equal."""
    torch = torch_cuda
    from recom_amd import tables
    rows = 1027                                                  # more than a block of slots at every dim, a partial last one
    q = np.random.default_rng(50 + dim).integers(0, 256, (rows, dim + 8), dtype=np.uint8)
    want = synth.dequantize_q8(q)
    out = torch.full((rows + 1, dim), float("nan"), dtype=torch.float32, device="cuda:0")
    out.view(torch.int32).fill_(0x5A5A5A5A)
    tables.convert(_dev(torch, q), "f32", out=out)
    got = out.cpu().numpy()
    n_nan = T16.assert_same_bits(got[:rows], want, ("q8 -> f32", dim))
    assert n_nan > 0 or dim == 1
    assert (got[rows:].view(np.uint32) == 0x5A5A5A5A).all()


@pytest.mark.parametrize("dtype", T16.DTYPES)
def test_widening_every_pattern_is_exact(torch_cuda, dtype):
    """All 65 536 patterns of the type, as tables of dim 4, 2 and 1 (V = 4, 2, 1)."""
    torch = torch_cuda
    from recom_amd import tables
    bits = np.arange(65536, dtype=np.uint16)
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    for dim in (4, 2, 1):
        src = _dev(torch, bits.view(np.int16).reshape(-1, dim)).view(tdt)
        got = tables.convert(src, "f32").cpu().numpy()
        want = T16.widen(bits.reshape(-1, dim), dtype)
        T16.assert_same_bits(got, want, ("widen", dtype, dim))
        if dtype == "bf16":                                       # widened in integers: a NaN keeps sign and payload
            assert (got.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("dtype", T16.DTYPES)
def test_narrowing_equals_torch_cpu_cast(torch_cuda, dtype):
    """The edge values of the narrow-output cases and random float32 bit patterns: where the result is not NaN, the pattern
    torch's CPU .to(bfloat16 / float16) gives; NaN stays NaN."""
    torch = torch_cuda
    from recom_amd import tables
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    rnd = np.random.default_rng(17).integers(0, 2 ** 32, 60000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    vals = np.concatenate([N.EDGE_VALUES, rnd])
    for dim in (4, 2, 1, 12, 6, 3):
        x = np.resize(vals, (len(vals) // dim + 1, dim)).astype(np.float32)
        want = torch.from_numpy(x.copy()).to(tdt).view(torch.int16).numpy().view(np.uint16)
        assert (want == N.narrow(x, dtype))[~N.is_nan16(want, dtype)].all()        # (the project's restatement agrees)
        got = tables.convert(_dev(torch, x), dtype)
        assert got.dtype == tdt and tuple(got.shape) == x.shape
        got = got.cpu().view(torch.int16).numpy().view(np.uint16)
        nan = N.is_nan16(want, dtype)
        assert nan.any() and (nan == np.isnan(x)).all()
        assert (N.is_nan16(got, dtype) == nan).all(), (dtype, dim, "NaN did not stay NaN")
        bad = np.argwhere(~nan & (got != want))
        assert bad.size == 0, (dtype, dim, len(bad), [hex(int(x.view(np.uint32)[tuple(b)])) for b in bad[:4]])


def test_offsets_beyond_32_bits(torch_cuda):
    """One table of dim 64 and 2^24 + 3 rows, filled by a closed form on the device: a 4.29 GB source and a 1.21 GB
    destination — the source's byte offsets pass 2^32, the source's element offsets 2^30.  The first 64, the last 64 and
    1 000 sampled rows against the restatement of the same closed form."""
    torch = torch_cuda
    from recom_amd import tables
    rows, dim = TC.BIG_ROWS, TC.BIG_DIM
    free, _total = torch.cuda.mem_get_info()
    need = rows * dim * 4 + rows * (dim + 8) + (1 << 30)
    assert free >= need, f"needs {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free"
    dev = torch.device("cuda", 0)
    src = TC.big_rows_torch(torch, dev)
    out = tables.convert(src, "q8")
    sample = np.unique(np.concatenate([np.arange(64), np.arange(rows - 64, rows),
                                       np.random.default_rng(3).integers(0, rows, 1000),
                                       [(1 << 32) // (4 * dim) - 1, (1 << 32) // (4 * dim), (1 << 32) // (4 * dim) + 1]]))
    assert sample.max() == rows - 1 and rows * dim * 4 > 2 ** 32 and rows * dim > 2 ** 30
    idx = torch.from_numpy(sample).to(dev)
    x = TC.big_rows_numpy(sample)
    assert (src[idx].cpu().numpy() == x).all()
    _same_rows(out[idx].cpu().numpy(), TC.quantize_ref(x), "2^24 + 3 rows")
    del src, out
    torch.cuda.empty_cache()
