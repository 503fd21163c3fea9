"""fcp_outputs_compare on non-default streams (kernels: recom_amd/csrc/fcp_outputs_compare.hip): a call from another stream with a
workspace of its own leaves the bytes of a call on the default stream, for all nine pairs of element kinds; and
ops.compare_outputs_async enqueued directly behind its two requests on a stream of its own, nothing synchronised in between,
gives the records of the synchronous form.

A file that sorts behind tests/test_z_gpu_private_streams.py, for the reason tests/test_zzz_gpu_table_convert_stream.py
gives: a stream taken from torch's pool shifts which hardware queue later streams are mapped to, the one thing the
private-stream tests depend on and cannot see.  Behind them it disturbs nothing."""
import numpy as np
import pytest

import outputs_compare_cases as OC
from test_zzz_gpu_outputs_compare import KEYS, Buffers, _side_arrays, _torch_elems, served, torch_cuda  # noqa: F401  (two fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kinds", OC.KIND_PAIRS, ids=["-".join(p) for p in OC.KIND_PAIRS])
def test_edge_matrix_from_another_stream(torch_cuda, kinds):
    torch = torch_cuda
    from recom_amd import lib
    L = lib.load()
    dev = torch.device("cuda", 0)
    m = OC.edge_matrix(*kinds)
    n = len(m["columns"])
    ta, tb = _torch_elems(torch, m["a"]["arena"], dev), _torch_elems(torch, m["b"]["arena"], dev)
    pa, sa = _side_arrays(m["a"], ta)
    pb, sb = _side_arrays(m["b"], tb)
    shapes = [v for rd in m["columns"] for v in rd]

    def run(buffers, stream):
        status = OC.call(L, pa, sa, kinds[0], pb, sb, kinds[1], shapes, n, buffers.out.data_ptr(), buffers.ws.data_ptr(), 0, stream)
        assert status == 0, L.fcp_last_error().decode()

    first, other = Buffers(torch, L, n, dev), Buffers(torch, L, n, dev)
    run(first, torch.cuda.current_stream(dev).cuda_stream)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))       # (the arenas were filled on the default stream)
    run(other, side.cuda_stream)                           # concurrent with the first call: each has its workspace
    run(other, side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()
    got = first.records()
    OC.assert_records(got, m["want"], kinds, m["finite_pairs"])
    assert other.out.cpu().numpy().tobytes() == got.tobytes(), "another stream, different bytes"
    assert first.guards_intact() and other.guards_intact()
    for t, side_ in ((ta, m["a"]), (tb, m["b"])):
        assert t.cpu().numpy().tobytes() == side_["arena"].tobytes(), "an arena changed"


@pytest.mark.parametrize("key", KEYS, ids=[k[0] for k in KEYS])
def test_compare_behind_its_requests(torch_cuda, served, key):
    torch = torch_cuda
    from recom_amd import ops
    case, serve, ref = served(key)
    want = ops.compare_outputs(ref, serve("q8"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(side):
        a = serve("f32", stream=side.cuda_stream)
        b = serve("q8", stream=side.cuda_stream)
        records = ops.compare_outputs_async(a, b, stream=side.cuda_stream)
    side.synchronize()
    got = np.frombuffer(records.cpu().numpy().tobytes(), OC.RECORD)
    assert not want.identical
    assert got[:-1].tobytes() == np.asarray(want.columns).tobytes() and got[-1:].tobytes() == np.asarray(want.total).tobytes()
