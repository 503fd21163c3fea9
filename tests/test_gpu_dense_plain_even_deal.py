"""The plain dense kernel's block mapping on the device (recom_amd/csrc/fcp_plain_map.h): the partial last group of eight
spans dealt evenly over the XCDs (FCP_DIAG=plain_even_deal=1) against the generic kernel's mapping in the same kernel
(plain_even_deal=0) and against the generic kernel (dense_generic), bit for bit, and against the NumPy restatement.

Plans of 9, 15, 17 and 23 spans (one or two full groups and a last group of 1 or 7 spans): gather columns of dims 8, 16,
32, 64 cycling, vocab 1000, int32 ids, int64 ids and bucketized float32 values in turn.  Requests of 64, 65, 80 and 100
rows: 4, 5, 5 and 7 row tiles, the last one partial but for 64 and 80 — with a last group of 1 span every one of them
leaves dead blocks, with 7 spans 64 rows leave 4 and the others live blocks that the two mappings place differently.  One
column (dim 16; int32 ids at 9 and 15 spans, int64 ids at 17 and 23) straddles from the last full group into the last
group; one id of it is out of vocabulary per request, and with FCP_FLAG_COUNT_BAD_IDS it must be counted once, as the
generic kernel counts it.  Every store policy is forced."""
import functools
import os

import numpy as np
import pytest

import dense_plain_cases as D

pytestmark = pytest.mark.gpu

SPANS = (9, 15, 17, 23)
ROWS = (64, 65, 80, 100)
STORES = ("nt", "sc1_nt", "plain")
DIMS = (8, 16, 32, 64)
VOCAB = 1000
BOUNDARIES = np.arange(0.0, 5.0 * (VOCAB - 1), 5.0, dtype=np.float32)   # 999 boundaries, reproducible as fma(i, 5, 0): 1000 buckets
SPAN = 256                                                              # elements of a 64-slot span
MAPPINGS = (("even", "plain", ("plain_even_deal=1",)), ("generic_map", "plain", ("plain_even_deal=0",)),
            ("generic_kernel", "generic", ("dense_generic",)))


@functools.lru_cache(maxsize=None)
def build_case(nspans):
    """(spec, tables, index of the column that straddles from the last full group into the partial last group)"""
    from recom_amd.plan import FLAG_COUNT_BAD_IDS, IDS_F32_BUCKETIZE, IDS_I32, IDS_I64, PlanSpec
    edge = nspans // 8 * 8 * SPAN       # first element of the partial last group
    for phase in range(len(DIMS)):      # where the dim cycle starts: the first start that puts a column across `edge`
        dims, width = [], 0
        while width <= (nspans - 1) * SPAN:
            dims.append(DIMS[(phase + len(dims)) % len(DIMS)])
            width += dims[-1]
        offs = np.concatenate([[0], np.cumsum(dims)])
        straddle = [k for k, d in enumerate(dims) if offs[k] < edge < offs[k] + d]
        if straddle:
            break
    assert straddle and (width + SPAN - 1) // SPAN == nspans, (nspans, width)
    rng = np.random.default_rng(nspans)
    cols, ranks, esz, tables = [], [], [], []
    first = (nspans // 8 - 1 - straddle[0]) % 3     # the straddling column's ids: int32 (9, 15 spans) or int64 (17, 23)
    for k, dim in enumerate(dims):
        src = (IDS_I32, IDS_I64, IDS_F32_BUCKETIZE)[(k + first) % 3]
        tables.append(rng.standard_normal((VOCAB, dim)).astype(np.float32))
        ranks.append(1)
        esz.append(8 if src == IDS_I64 else 4)
        cols.append(D.gather(dim, VOCAB, src, k, k, k, BOUNDARIES if src == IDS_F32_BUCKETIZE else None))
    spec = PlanSpec(cols, ranks, esz, len(tables), flags=FLAG_COUNT_BAD_IDS)
    spec.validate()
    return spec, tables, straddle[0]


def make_inputs(spec, rows, seed, bad_col):
    """In-vocabulary ids everywhere but one: row `seed % rows` of the straddling column."""
    from recom_amd.plan import IDS_F32_BUCKETIZE, IDS_I64
    assert spec.columns[bad_col].id_source != IDS_F32_BUCKETIZE      # (a bucket is always a row of the table)
    rng = np.random.default_rng(seed)
    out = []
    for k, c in enumerate(spec.columns):
        if c.id_source == IDS_F32_BUCKETIZE:
            out.append(rng.uniform(-3.0, float(BOUNDARIES[-1]) + 3.0, rows).astype(np.float32))   # buckets 0 .. 999
        else:
            wide = c.id_source == IDS_I64
            ids = rng.integers(0, c.vocab, rows).astype(np.int64 if wide else np.int32)
            if k == bad_col:
                ids[seed % rows] = 2 ** 32 + 5 if wide else c.vocab    # (the whole 64-bit id is compared: not row 5)
            out.append(ids)
    return out


@functools.lru_cache(maxsize=None)
def device_tables(nspans):
    import torch
    return [torch.from_numpy(t).to(torch.device("cuda", 0)) for t in build_case(nspans)[1]]


def _diag(monkeypatch, *keys):
    drop = ("dense_generic", "wide_rows", "plain_even_deal")
    kept = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] not in drop]
    monkeypatch.setenv("FCP_DIAG", ",".join(kept + list(keys)))


def _blocks(nspans, rows):
    return 8 * ((nspans + 7) // 8) * ((rows + 15) // 16)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("nspans", SPANS)
def test_even_deal_equals_generic_mapping_generic_kernel_and_numpy(monkeypatch, nspans, store):
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec, tables, bad_col = build_case(nspans)
    dev = torch.device("cuda", 0)
    d_tabs = device_tables(nspans)
    if store == "nt":
        monkeypatch.delenv("FCP_STORE_THROUGH_BYTES", raising=False)
    else:
        monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    ops = []
    for _, _, keys in MAPPINGS:
        _diag(monkeypatch, *keys)
        ops.append(FeatureColumnProcess(spec, 0))
    _diag(monkeypatch)
    nbytes = max(ops[0].plan.arena_bytes(concat_inputs(make_inputs(spec, r, 0, bad_col))[2], None) for r in ROWS)
    # `plain`: one arena, reused, and one request ahead of the checked ones (an arena's first request stores `sc1 nt`)
    rings = [[torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if store == "plain" else 3)] for _ in ops]
    sequence = ((ROWS[-1],) if store == "plain" else ()) + ROWS
    for t, rows in enumerate(sequence):
        inputs = make_inputs(spec, rows, 1000 * nspans + 10 * t + rows, bad_col)
        blob, offsets, shapes = concat_inputs(inputs)
        d_blob = torch.from_numpy(blob).to(dev)
        want, bad = D.restate(spec, tables, inputs, rows)
        assert bad == 1
        got = []
        for (name, front, _), op, ring in zip(MAPPINGS, ops, rings):
            what = (nspans, store, rows, name)
            arena = ring[t % len(ring)]
            arena.fill_(0xFF)
            out = op(d_blob, offsets, shapes, d_tabs, None, arena=arena)
            torch.cuda.synchronize()
            assert op.plan.last_dense_front() == front, what
            launch = op.plan.last_launch()
            assert launch == dict(launch, kernel="dense", vec=4, rows_per_wave=4, dense_blocks=_blocks(nspans, rows),
                                  store=store if not (store == "plain" and t == 0) else "sc1_nt"), what
            g = out.groups[0].cpu().numpy().view(np.uint32)
            assert g.shape == want.shape, what
            diff = g != want.view(np.uint32)
            if diff.any():
                r, c = np.argwhere(diff)[0]
                raise AssertionError(f"{what}: {int(diff.sum())} elements differ from the NumPy restatement, first [{r}, {c}] "
                                     f"(span {c // SPAN}, row tile {r // 16}) got {g[r, c]:#x} want {want.view(np.uint32)[r, c]:#x}")
            assert bool((arena[out.groups[0].numel() * 4:] == 0xFF).all()), what      # nothing outside the group was written
            assert op.plan.read_bad_ids() == t + 1, what                             # one per request, counted once
            got.append(g)
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), (nspans, store, rows)
