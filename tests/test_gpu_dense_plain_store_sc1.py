"""The plain dense kernel's fourth output-store form, write-through without the streaming hint (`sc1`,
FCP_LAUNCH_STORE_SC1; recom_amd/csrc/fcp_dense_plain.hip), and the rule that hands it out (store_policy_for,
recom_amd/csrc/fcp_process.hip).

The form is forced with FCP_DIAG=store_policy=sc1 at plan creation.  Every width of tests/dense_plain_cases.py, with and
without bad-id counting, requests of 64, 65, 79 and 80 rows, once into one reused arena and once into a ring of three: the
plain front and `sc1` are reported, the bits equal the NumPy restatement and those of the same spec created with
FCP_DIAG=dense_generic plus the key — a plan on the generic kernel ignores the key and reports what the rule gives it
(FCP_STORE_THROUGH_BYTES=0 here: `plain` into the reused arena from its second request on, `sc1 nt` otherwise) — the
0xFF tail of the arena is untouched and the bad-id counts agree.

The rule, without the key, at its threshold of 32 MiB (the capacity of the eight L2s): dims 512 + 16 (2 112 bytes per row),
vocabulary 1 000, 16 400 rows = 34.6 MB (1 025 full row tiles) and 16 401 rows (the last tile holds one row).
profiles/dense_plain_store_sc1_ab.txt decides the two cells — (A) an arena one of the plan's last two requests wrote, up
to 160 MiB, (B) any other arena: A adopted `sc1`, B keeps `sc1_nt`.  15 880 rows (33.5 MB, below the threshold) keep what they
had: `plain` in cell A."""
import functools
import os

import numpy as np
import pytest

import dense_plain_cases as D

pytestmark = pytest.mark.gpu

KEY = "store_policy=sc1"
CELL_A, CELL_B = "sc1", "sc1_nt"          # what the committed rule reports at 32 MiB and above (see the module docstring)
RULE_DIMS, RULE_VOCAB = (512, 16), 1000
RULE_ROWS = (16400, 16401, 15880)


def _diag(monkeypatch, *keys):
    drop = ("dense_generic", "wide_rows", "plain_even_deal", "store_policy")
    kept = [k for k in os.environ.get("FCP_DIAG", "").split(",") if k and k.split("=")[0] not in drop]
    monkeypatch.setenv("FCP_DIAG", ",".join(kept + list(keys)))


def _blocks(spec, rows):
    nspans = (spec.group_width(0) // 4 + 63) // 64
    return (8 * ((nspans + 7) // 8) if nspans >= 8 else nspans) * ((rows + 15) // 16)


def _check_bits(out, want, what):
    g = out.groups[0].cpu().numpy().view(np.uint32)
    assert g.shape == want.shape, what
    diff = g != want.view(np.uint32)
    if diff.any():
        r, c = np.argwhere(diff)[0]
        raise AssertionError(f"{what}: {int(diff.sum())} elements differ from the NumPy restatement, first [{r}, {c}] "
                             f"got {g[r, c]:#x} want {want.view(np.uint32)[r, c]:#x}")
    return g


@pytest.mark.parametrize("count_bad", (True, False), ids=("count", "nocount"))
@pytest.mark.parametrize("arenas", ("one", "ring3"))
@pytest.mark.parametrize("width", sorted(D.WIDTHS))
def test_forced_sc1_equals_generic_and_numpy(monkeypatch, width, arenas, count_bad):
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    case = D.build_case(width, count_bad)
    spec = case.spec
    dev = torch.device("cuda", 0)
    d_tabs = [torch.from_numpy(t).to(dev) for t in case.tables]
    monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    _diag(monkeypatch, KEY)
    forced = FeatureColumnProcess(spec, 0)
    _diag(monkeypatch, "dense_generic", KEY)
    generic = FeatureColumnProcess(spec, 0)
    _diag(monkeypatch)
    ops = (forced, generic)
    nbytes = max(forced.plan.arena_bytes(concat_inputs(D.make_inputs(spec, r, 0))[2], None) for r in D.ROWS)
    rings = [[torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if arenas == "one" else 3)] for _ in ops]
    bad_total = 0
    for t, rows in enumerate(D.ROWS):
        inputs = D.make_inputs(spec, rows, 300 * t + rows)
        blob, offsets, shapes = concat_inputs(inputs)
        d_blob = torch.from_numpy(blob).to(dev)
        want, bad = D.restate(spec, case.tables, inputs, rows)
        assert bad > 0
        bad_total += bad
        today = "plain" if arenas == "one" and t > 0 else "sc1_nt"      # (an arena's first request stores `sc1 nt`)
        got = []
        for op, ring, front, store in zip(ops, rings, ("plain", "generic"), ("sc1", today)):
            what = (width, arenas, count_bad, rows, front)
            arena = ring[t % len(ring)]
            arena.fill_(0xFF)
            out = op(d_blob, offsets, shapes, d_tabs, None, arena=arena)
            torch.cuda.synchronize()
            assert op.plan.last_dense_front() == front, what
            launch = op.plan.last_launch()
            assert launch == dict(launch, kernel="dense", vec=4, rows_per_wave=4, wide_rows=False, shard_world=1, ragged_blocks=0,
                                  dense_blocks=_blocks(spec, rows), store=store), what
            got.append(_check_bits(out, want, what))
            assert bool((arena[out.groups[0].numel() * 4:] == 0xFF).all()), what      # nothing outside the group was written
            assert op.plan.read_bad_ids() == (bad_total if count_bad else 0), what
        assert np.array_equal(got[0], got[1]), (width, arenas, rows)


@functools.lru_cache(maxsize=None)
def _rule_case():
    from recom_amd.plan import IDS_I32, IDS_I64, PlanSpec
    rng = np.random.default_rng(512)
    cols, tables = [], []
    for k, (dim, src) in enumerate(zip(RULE_DIMS, (IDS_I32, IDS_I64))):
        tables.append(rng.standard_normal((RULE_VOCAB, dim)).astype(np.float32))
        cols.append(D.gather(dim, RULE_VOCAB, src, k, k, k))
    spec = PlanSpec(cols, [1, 1], [4, 8], len(tables))
    spec.validate()
    return spec, tables


@functools.lru_cache(maxsize=None)
def _rule_request(rows):
    """(inputs, restatement): computed once per size, shared by the two arena cells, never written"""
    spec, tables = _rule_case()
    inputs = D.make_inputs(spec, rows, rows)
    want, _ = D.restate(spec, tables, inputs, rows)
    want.setflags(write=False)
    return inputs, want


@pytest.mark.parametrize("rows", RULE_ROWS)
@pytest.mark.parametrize("arenas", ("reused", "fresh_ring"))
def test_rule_at_the_threshold_without_the_key(monkeypatch, arenas, rows):
    """profiles/dense_plain_store_sc1_ab.txt: cell A adopted `sc1`, cell B did not.  At 16 400 and 16 401 rows (34.6 MB, at least
    32 MiB) a reused arena reports `sc1` from its second request on (its first request finds an arena the plan has not seen:
    cell B) and a ring of three `sc1_nt`; at 15 880 rows (below 32 MiB; FCP_STORE_THROUGH_BYTES=0 keeps the three-policy rule
    in force there) the reused arena reports `plain`, as before."""
    import torch
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    spec, tables = _rule_case()
    assert (spec.group_width(0) * 4 * rows >= 32 << 20) == (rows != 15880)
    dev = torch.device("cuda", 0)
    d_tabs = [torch.from_numpy(t).to(dev) for t in tables]
    monkeypatch.setenv("FCP_STORE_THROUGH_BYTES", "0")
    _diag(monkeypatch)
    op = FeatureColumnProcess(spec, 0)
    inputs, want = _rule_request(rows)
    blob, offsets, shapes = concat_inputs(inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    nbytes = op.plan.arena_bytes(shapes, None)
    ring = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(1 if arenas == "reused" else 3)]
    above = rows != 15880
    for t in range(2):
        arena = ring[t % len(ring)]
        arena.fill_(0xFF)
        out = op(d_blob, offsets, shapes, d_tabs, None, arena=arena)
        torch.cuda.synchronize()
        what = (arenas, rows, t)
        assert op.plan.last_dense_front() == "plain", what
        cell_a = arenas == "reused" and t > 0
        expect = (CELL_A if cell_a else CELL_B) if above else ("plain" if cell_a else "sc1_nt")
        assert op.plan.last_launch()["store"] == expect, what
        _check_bits(out, want, what)
        assert bool((arena[out.groups[0].numel() * 4:] == 0xFF).all()), what
