"""Shape evaluation, field by field: the host half of the plan (recom_amd/csrc/fcp_plan_shape.cc) is linked with the
descriptor unit and nothing else into a stand-alone program (tests/native/plan_shape_san.cc) built with
-fsanitize=address,undefined, which evaluates every request of plan_shape_cases.py — with the offsets and concated_bytes
that ConcatInputs really produced — and prints every record field, the arena layout, the regular-CSR decision and the launch
geometry, or the refusal.  All of it must equal the Python restatement exactly.  No GPU."""
import os
import shutil
import subprocess

import pytest

import plan_shape_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return S.all_cases()


@pytest.fixture(scope="module")
def restated(cases):
    return {c.name: c.restated() for c in cases}


@pytest.fixture(scope="module")
def printed(cases, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("plan_shape")
    csrc = os.path.join(ROOT, "recom_amd", "csrc")
    exe = str(tmp / "plan_shape_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                            os.path.join(ROOT, "tests", "native", "plan_shape_san.cc"), os.path.join(csrc, "fcp_plan_desc.cc"),
                            os.path.join(csrc, "fcp_plan_shape.cc"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        pytest.skip("libasan / libubsan not installed")
    assert build.returncode == 0, build.stderr
    requests = str(tmp / "requests.txt")
    S.write_requests(requests, cases, str(tmp))
    env = {k: v for k, v in os.environ.items() if k not in ("FCP_DIAG", "FCP_SEG_PREPASS", "FCP_SEG_SEARCH_MAX_PAIRS")}
    run = subprocess.run([exe, requests], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stderr == "" and run.stdout.endswith(f"end {len(cases)}\n"), run.stdout[-2000:] + run.stderr[-4000:]
    return S.parse_output(run.stdout)


def test_the_cases_cover_what_they_are_meant_to(cases, restated):
    """Every path of the rule is taken by some request, judged by the restatement alone."""
    assert len({c.name for c in cases}) == len(cases)
    good = [restated[c.name] for c in cases if c.fault is None]
    assert all(isinstance(r, dict) for r in good)
    for c in cases:                                          # a fault case is refused with exactly the recorded answer
        if c.fault is not None:
            assert restated[c.name] == c.fault, c.name
    assert len({c.fault for c in cases if c.fault}) == 16    # (the three misaligned inputs and the two missing symbols share a text)
    geo = lambda r, kind: [v for k, v in r.items() if k.startswith(f"geo.{kind}.")]
    assert {r["geo.0"][0] for r in good} == {1, 2, 4} and {r["geo.1"][0] for r in good} == {1}
    assert {r["csr_reg"][0] for r in good} == {0, 1, 2}
    assert {r["seg_search"][0] for r in good} == {0, 1}
    nsp8 = {g[4] for r in good for kind in (0, 1) for g in geo(r, kind)}
    assert -1 in nsp8 and any(v < -1 for v in nsp8) and any(v >= 2 for v in nsp8)   # no span, fewer than 8, more than one eight
    assert any(g[2] == 10 and g[4] == 2 for r in good for g in geo(r, 1))          # 10 spans: two eights, not 1.25
    assert any(g[3] > 0 for r in good for kind in (0, 1) for g in geo(r, kind))    # a strict subset of the spans, not the first list
    assert any(g[3] == -1 and g[2] > 0 for r in good for g in geo(r, 0))
    assert {r["group_rows"][0] for r in good} >= {0, 1, 31, 32, 63, 64}
    assert any("wts" in r and any(w >= 0 for w in r["wts"]) and -1 in r["wts"] for r in good)
    assert any(any(v[8] != 1 for k, v in r.items() if k.startswith("dyn.")) for r in good)            # a map's symbol
    per_col = restated["per_column-permuted"]                # out_base ascends in PLAN order, which is not concat order there
    spec = next(c.spec for c in cases if c.name == "per_column-permuted")
    pos_of = S.plan_facts(spec)["pos_of"]
    bases = [per_col[f"dyn.{pos_of[k]}"][2] for k in range(spec.n_columns)]
    assert bases == sorted(bases) and [pos_of[k] for k in range(spec.n_columns)] != list(range(spec.n_columns))
    assert [per_col[f"dyn.{pos}"][2] for pos in range(spec.n_columns)] != sorted(bases)


def test_every_field_equals_the_restatement(cases, restated, printed):
    assert sorted(printed) == sorted(restated)
    for c in cases:
        got, want = printed[c.name], restated[c.name]
        if isinstance(want, tuple):
            assert got == want, c.name
            continue
        assert isinstance(got, dict), (c.name, got)
        assert sorted(got) == sorted(want), c.name
        for key in want:
            assert got[key] == want[key], (c.name, key)
