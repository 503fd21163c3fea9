"""What a plan descriptor is answered — status and message — is pinned case by case against tests/golden/plan_refusals.json,
recorded with the library as it was before its four per-format validators became one rule list (plan_refusal_cases.py), and
the Python mirror (PlanSpec.validate) raises the matching exception with the same words.  No GPU."""
import json

import pytest

import plan_refusal_cases as R
from recom_amd import lib as _lib
from recom_amd import plan as _plan

with open(R.GOLDEN) as _f:
    GOLDEN = json.load(_f)
CASES = dict(R.cases())


def test_the_golden_file_covers_the_matrix():
    assert sorted(GOLDEN) == sorted(CASES) and len(CASES) == len(R.FAMILIES) * (len(R.SINGLES) + len(R.PAIRS))
    # every family's subject, every status, and both "column k:" positions of a two-column pair are in it
    messages = [e["message"] for e in GOLDEN.values()]
    for subject in ("narrow output", "per-input table formats", "8-bit tables", "16-bit tables"):
        assert any(m.startswith(subject) for m in messages) and any(m.startswith("column 0: " + subject) for m in messages)
    assert {e["status"] for e in GOLDEN.values()} == {_lib.FCP_OK, _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_UNSUPPORTED}


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_the_library_answers_what_it_answered(family):
    L = _lib.load()
    names = [n for n in CASES if n.startswith(family + "/")]
    got = {n: dict(zip(("status", "message"), R.create_raw(L, _lib, CASES[n]))) for n in names}
    want = {n: {k: GOLDEN[n][k] for k in ("status", "message")} for n in names}
    assert got == want


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_the_python_mirror_raises_the_same(family):
    checked = 0
    for name, d in CASES.items():
        if not name.startswith(family + "/"):
            continue
        got = R.python_answer(d)
        if got is None:                                  # PlanSpec cannot express the case
            continue
        g = GOLDEN[name]
        want = tuple(g["python"]) if "python" in g else R.expected_python(g["status"], g["message"])
        assert got == want, name
        if got[0]:
            assert issubclass(getattr(_plan, got[0], ValueError), ValueError)
        checked += 1
    assert checked >= len(R.SINGLES) + len(R.PAIRS) - 3   # all but the table_kind1 cases only the raw entry can express


def _plan_files(tmp_path):
    """One plan file per format version 1..8, from the small specs of the host tests; between them the weights, segmaps and
    stage sections, boundaries and id-transform intervals."""
    import dataclasses
    import table_mixed_cases as M
    from segmap_cases import build
    from recom_amd import plan_io, synth
    small = M.small_mixed_spec()
    mapped, *_ = build(1)
    cols = list(mapped.columns)
    cols[0] = dataclasses.replace(cols[0], weights_input=mapped.n_host_inputs)
    both = dataclasses.replace(mapped, columns=cols, host_input_ranks=list(mapped.host_input_ranks) + [1],
                               host_input_elem_sizes=list(mapped.host_input_elem_sizes) + [4])
    staged, stage = both.staged_for_concat_inputs()
    plain_stage = _plan.StageInfo([_plan.STAGE_COPY] * small.n_host_inputs, [-1] * small.n_host_inputs)
    specs = {2: (synth.model_mixed(batch=21, vocab=97).spec, None), 3: (small, plain_stage), 4: (mapped, None), 5: (staged, stage),
             6: (small.with_out_dtype("bf16"), None), 7: (small.with_table_dtype("q8"), None),
             8: (small.with_table_dtypes(M.SMALL_KINDS), None)}
    paths = {}
    for version, (spec, st) in specs.items():
        paths[version] = tmp_path / f"v{version}.plan"
        plan_io.save_plan(spec, str(paths[version]), st)
        assert paths[version].read_text().startswith(f"fcp_plan {version}\n") and paths[version].stat().st_size < 8192, version
    # version 1 is version 2 without the id-transform fields behind every column (no writer produces it any more)
    lines = paths[3].read_text().replace("fcp_plan 3\n", "fcp_plan 1\n").split("\nstage ")[0].split("\n")
    at = lines.index(f"columns {small.n_columns}")
    for i in range(at + 1, at + 1 + small.n_columns):
        assert lines[i].endswith(" 0 0 0 0")
        lines[i] = lines[i][:-len(" 0 0 0 0")]
    paths[1] = tmp_path / "v1.plan"
    paths[1].write_text("\n".join(lines) + "\n")
    text = "".join(p.read_text() for p in paths.values())
    assert all(f"\n{section} " in text for section in ("weights", "segmaps", "stage"))
    return [str(paths[v]) for v in sorted(paths)]


def test_the_descriptor_unit_alone_under_address_and_undefined_sanitizers(tmp_path):
    """recom_amd/csrc/fcp_plan_desc.cc links without the GPU runtime; a stand-alone program (tests/native/plan_desc_san.cc),
    both built with -fsanitize=address,undefined, loads a plan file of every format version and every proper prefix of it,
    and runs check_desc over the refusal matrix."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "recom_amd", "csrc")
    exe = str(tmp_path / "plan_desc_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                            os.path.join(root, "tests", "native", "plan_desc_san.cc"), os.path.join(csrc, "fcp_plan_desc.cc"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        pytest.skip("libasan / libubsan not installed")
    assert build.returncode == 0, build.stderr
    cases = str(tmp_path / "cases.txt")
    R.write_cases(cases, GOLDEN)
    run = subprocess.run([exe, cases] + _plan_files(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "" and run.stdout == "0 failures\n", run.stdout + run.stderr[-4000:]
