"""fcp_tables_delta_distinct / fcp_tables_delta_launches / fcp_tables_delta_workspace_bytes without a GPU: the C ABI's surface,
the workspace formula and its stated bound, the status order with its `entry k` messages — per entry the single-table entry's
own sentences — the launch count (the point of the feature: it does not grow with the number of entries), the deal of blocks,
the Python wrappers' refusals, the code object of recom_amd/csrc/fcp_tables_delta.hip, and the host-only plan unit
(recom_amd/csrc/fcp_tables_delta_plan.cc) alone under the sanitizers.  (The kernels themselves:
tests/test_zzz_gpu_tables_delta.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import table_convert_cases as TC
import table_delta_cases as DC
import tables_delta_cases as GC
from recom_amd import lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fcp_hip.h")
CSRC = os.path.join(ROOT, "recom_amd", "csrc")
A = 1 << 20                                                   # an address aligned for everything
WHO = "fcp_tables_delta_distinct"
NAMES = ("fcp_tables_delta_workspace_bytes", "fcp_tables_delta_launches", "fcp_tables_delta_deal_blocks", "fcp_tables_delta_grid", WHO)
INV, NODEV, OK = _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_NO_DEVICE, _lib.FCP_OK


def _entry(dim=64, n=5, table_rows=100, id_bytes=8, ids=A, rows=A, ids_out=A, rows_out=A, pos_out=0):
    """dim 0: ids only"""
    return _lib.TableDeltaEntry(ids, rows if dim else 0, ids_out, rows_out if dim else 0, pos_out, table_rows, n, id_bytes, dim)


def _array(entries):
    return (_lib.TableDeltaEntry * max(len(entries), 1))(*entries)


def _call(entries, n_tables=None, reports=A, workspace=A, device=0):
    L = _lib.load()
    status = L.fcp_tables_delta_distinct(_array(entries) if entries is not None else None, len(entries) if n_tables is None else n_tables,
                                         C.c_void_p(reports), C.c_void_p(workspace), device, None)
    return status, L.fcp_last_error().decode()


def _single(e, report=A, workspace=A):
    """the single-table entry with entry e's arguments"""
    L = _lib.load()
    status = L.fcp_table_delta_distinct(C.c_void_p(e.row_ids), e.id_bytes, C.c_void_p(e.rows), e.dim, e.n, e.table_rows, C.c_void_p(e.ids_out),
                                        C.c_void_p(e.rows_out), C.c_void_p(e.pos_out), C.c_void_p(report), C.c_void_p(workspace), 0, None)
    return status, L.fcp_last_error().decode()


def _launches(entries, n_tables=None):
    return int(_lib.load().fcp_tables_delta_launches(_array(entries), len(entries) if n_tables is None else n_tables))


def _prose():
    """the header with its comments' line leaders taken out and white space folded"""
    return re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", "\n", open(HEADER).read()))


def _ws(ns, n_tables=None):
    arr = (C.c_int64 * max(len(ns), 1))(*ns)
    return int(_lib.load().fcp_tables_delta_workspace_bytes(arr, len(ns) if n_tables is None else n_tables))


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert "int64_t fcp_tables_delta_workspace_bytes(const int64_t *n /* host [n_tables] */, int32_t n_tables);" in text
    assert "int32_t fcp_tables_delta_launches(const fcp_table_delta_entry_t *entries, int32_t n_tables);" in text
    assert ("int fcp_tables_delta_distinct(const fcp_table_delta_entry_t *entries, int32_t n_tables, fcp_table_delta_report_t *reports "
            "/* device [n_tables] */, void *workspace, int32_t device, void *stream);") in text
    assert "} fcp_table_delta_entry_t;" in text
    assert "must be merged into one entry first" in _prose()                # ids that repeat across entries
    assert set(NAMES) <= set(_lib.EXPORTS)
    L = _lib.load()
    for name in NAMES:
        assert hasattr(L, name), name
    # behind the single-table entry
    assert text.index("int fcp_table_delta_distinct(") < text.index("typedef struct fcp_table_delta_entry {") < text.index("int fcp_tables_delta_distinct(")


def test_the_entry_struct_is_64_bytes_in_c_and_in_python(tmp_path):
    assert C.sizeof(_lib.TableDeltaEntry) == 64
    offsets = {f: getattr(_lib.TableDeltaEntry, f).offset for f, _t in _lib.TableDeltaEntry._fields_}
    assert offsets == {"row_ids": 0, "rows": 8, "ids_out": 16, "rows_out": 24, "pos_out": 32, "table_rows": 40, "n": 48, "id_bytes": 56, "dim": 60}
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fcp_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(fcp_table_delta_entry_t), offsetof(fcp_table_delta_entry_t, pos_out), offsetof(fcp_table_delta_entry_t, n), '
                   'offsetof(fcp_table_delta_entry_t, id_bytes), offsetof(fcp_table_delta_entry_t, dim)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["64", "32", "48", "56", "60"]


# ---- the workspace ---------------------------------------------------------------------------------------------------------------
def _bound(ns):
    """what the header states: at most 40 N + 1024 n_tables + 2^10"""
    return 40 * sum(ns) + 1024 * len(ns) + 1024


def test_workspace_formula():
    """A function of the n values alone: -1 for an invalid argument, a multiple of 8, non-decreasing in every n[k], within the
    bound the header states — which follows from the layout: per entry with ids a 128-byte record, 12 bytes of first-block
    values and a 16-byte run (156), at most max(512, 32 n) bytes of cells, n + 7 of flags and 32 (n / 1024 + 2) of partial
    records, 739 + 33.04 n together; per call 16 bytes, 22 first-block values and the sections' padding, below 2^10."""
    text = _prose()
    assert "at most 40 * N + 1024 * n_tables + 2^10 with N the sum of the n[k]" in text
    L = _lib.load()
    assert _ws([1], n_tables=-1) == -1 and _ws([1], n_tables=65537) == -1 and _ws([1], n_tables=-2 ** 31) == -1
    assert int(L.fcp_tables_delta_workspace_bytes(None, 1)) == -1
    assert _ws([5, -1]) == -1 and _ws([DC.LIMIT]) == -1 and _ws([DC.LIMIT - 1]) > 0
    assert _ws([DC.LIMIT - 6, 5]) > 0 and _ws([DC.LIMIT - 5, 5]) == -1                      # the sum
    assert 0 < _ws([]) <= 1024 and int(L.fcp_tables_delta_workspace_bytes(None, 0)) == _ws([])
    assert 0 < _ws([0] * 65536) <= _bound([0] * 65536) and 0 < _ws([1] * 65536) <= _bound([1] * 65536)
    rng = np.random.default_rng(5)
    edges = [0, 1, 2, 16, 17, 32, 33, 1023, 1024, 1025, 4096, 4097, DC.FULL_PASS - 1, DC.FULL_PASS, DC.FULL_PASS + 1, 5 * DC.FULL_PASS + 3]
    for n in edges:
        assert 0 < _ws([n]) <= _bound([n]) and _ws([n]) % 8 == 0, n
    # one entry: room for what the single-table entry takes, whose layout it repeats per entry
    for n in edges[1:]:
        assert _ws([n]) >= 8 * DC.cells_for(n) + n
    for _ in range(300):
        ns = [int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(0, 300000)) for _k in range(int(rng.integers(1, 40)))]
        w = _ws(ns)
        assert w > 0 and w % 8 == 0 and w <= _bound(ns), ns
        k = int(rng.integers(0, len(ns)))
        for step in (1, 7, 1024, 99999):
            more = list(ns)
            more[k] += step
            assert _ws(more) >= w, (ns, k, step)
        assert _ws(ns + [0]) >= w                                             # and in n_tables


# ---- status order ------------------------------------------------------------------------------------------------------------
def test_status_codes_arrive_in_the_stated_order():
    """n_tables; `entries`; the entries in ascending order, each by the single-table entry's own order and text; the sum of the
    ids; `reports`; `workspace`.  Then FCP_OK without entries, without a device; then, on a machine without a GPU,
    FCP_ERR_NO_DEVICE.  (Pointers are never dereferenced on the host: plain numbers serve.)"""
    import torch
    no_gpu = not torch.cuda.is_available()
    good = _entry()
    for n_tables in (-1, 65537, -2 ** 31, 2 ** 31 - 1):
        status, msg = _call([good], n_tables=n_tables)
        assert status == INV and msg == f"{WHO}: `n_tables` must lie in [0, 65536]", (n_tables, status, msg)
    status, msg = _call(None, n_tables=3)
    assert status == INV and msg == f"{WHO}: `entries` is null", msg
    assert "`n_tables`" in _call(None, n_tables=-5)[1]                                         # n_tables comes before entries
    # per entry: the single-table entry refuses the same arguments by the same sentence, in full
    bad_entries = [_entry(n=-1), _entry(n=2 ** 32 - 3), _entry(table_rows=0), _entry(table_rows=2 ** 32 - 3), _entry(id_bytes=2), _entry(id_bytes=0),
                   _entry(dim=-3), _lib.TableDeltaEntry(A, 0, A, A, 0, 100, 5, 8, 4), _lib.TableDeltaEntry(A, A, A, 0, 0, 100, 5, 8, 4),
                   _entry(ids=0), _entry(ids_out=0), _entry(ids=A + 4), _entry(id_bytes=4, ids=A + 2), _entry(rows=A + 8), _entry(dim=6, rows=A + 4),
                   _entry(dim=3, rows=A + 2), _entry(ids_out=A + 4), _entry(rows_out=A + 8), _entry(dim=2, rows_out=A + 4), _entry(pos_out=A + 4),
                   _entry(n=0, table_rows=0), _entry(n=0, id_bytes=3)]
    sentences = set()
    for bad in bad_entries:
        s_status, s_msg = _single(bad)
        assert s_status == INV and s_msg.startswith("fcp_table_delta_distinct: "), s_msg
        sentence = s_msg[len("fcp_table_delta_distinct: "):]
        sentences.add(sentence)
        for k in (0, 1, 4):
            status, msg = _call([good] * k + [bad] + [good] * 2)
            assert status == INV and msg == f"{WHO}: entry {k}: {sentence}", (k, status, msg, s_msg)
    assert len(sentences) >= 16
    # inside an entry the order is the single-table entry's: n, table_rows, id_bytes, dim, rows_out / rows, null pointers, alignment
    E = _lib.TableDeltaEntry
    for bad, word in ((E(0, A + 1, 0, 0, A + 1, 0, -1, 3, 0), "n"), (E(0, A + 1, 0, 0, A + 1, 0, 5, 3, 0), "table_rows"),
                      (E(0, A + 1, 0, 0, A + 1, 9, 5, 3, 0), "id_bytes"), (E(0, A + 1, 0, 0, A + 1, 9, 5, 8, 0), "dim"),
                      (E(0, 0, 0, A + 1, A + 1, 9, 5, 8, 4), "rows_out"), (E(0, A + 1, 0, 0, A + 1, 9, 5, 8, 4), "rows_out"),
                      (E(0, A + 1, 0, A + 1, A + 1, 9, 5, 8, 4), "row_ids"), (E(A + 1, A + 1, 0, A + 1, A + 1, 9, 5, 8, 4), "ids_out"),
                      (E(A + 1, A + 1, A + 1, A + 1, A + 1, 9, 5, 8, 4), "row_ids"), (E(A, A + 1, A + 1, A + 1, A + 1, 9, 5, 8, 4), "rows"),
                      (E(A, A, A + 1, A + 1, A + 1, 9, 5, 8, 4), "ids_out"), (E(A, A, A, A + 1, A + 1, 9, 5, 8, 4), "rows_out"),
                      (E(A, A, A, A, A + 1, 9, 5, 8, 4), "pos_out")):
        status, msg = _call([bad], reports=0, workspace=0)
        assert status == INV and msg.startswith(f"{WHO}: entry 0: `{word}`"), (word, status, msg)
        assert _single(bad)[1] == "fcp_table_delta_distinct: " + msg[len(f"{WHO}: entry 0: "):]
    # the first bad entry wins; an entry wins over the sum, the reports and the workspace
    status, msg = _call([good, _entry(id_bytes=5), _entry(n=-1)], reports=A + 4, workspace=A + 4)
    assert status == INV and "entry 1: `id_bytes`" in msg, msg
    # the ids of a call, summed: the single-table limit
    half = (DC.LIMIT - 1) // 2
    big = _entry(dim=0, n=half, table_rows=1000)
    assert _launches([big, big]) == 6                                                          # 2^32 - 4 together: passes
    status, msg = _call([big, big, _entry(dim=0, n=1)], reports=0, workspace=0)
    assert status == INV and msg == f"{WHO}: `entries` name 2^32 - 3 ids or more together", msg
    assert _launches([big, big, _entry(n=1)]) == -INV
    # reports, then the workspace
    for reports, workspace, sentence in ((0, 0, "`reports` is null"), (A + 4, 0, "`reports` is not 8-byte aligned"), (A, 0, "`workspace` is null"),
                                         (A, A + 4, "`workspace` is not 8-byte aligned")):
        status, msg = _call([good], reports=reports, workspace=workspace)
        assert status == INV and msg == f"{WHO}: {sentence}", msg
    assert _call([_entry(n=0)], workspace=0)[0] == INV                      # an invalid argument wins over "nothing to install"
    # nothing to do: FCP_OK with no device
    assert _call([], reports=0, workspace=0, device=12345)[0] == OK
    assert _call(None, n_tables=0, reports=0, workspace=0, device=12345)[0] == OK
    # work, the reports of empty entries included: no device here
    if no_gpu:
        assert _call([good])[0] == NODEV
        assert _call([_entry(n=0, ids=0, ids_out=0, rows=0, rows_out=0)])[0] == NODEV        # reports[0] is written on the device
        assert _call([_entry(dim=0, n=7, id_bytes=4, pos_out=A + 8), good, _entry(n=0)])[0] == NODEV
        assert _call([_entry(dim=0, n=2 ** 32 - 4, table_rows=2 ** 32 - 4)])[0] == NODEV       # the last values below both limits


def test_the_single_table_messages_did_not_move():
    """both entries refuse through one routine; the single-table entry's texts are what they were"""
    assert _single(_entry(n=-1))[1] == "fcp_table_delta_distinct: `n` is negative"
    assert _single(_entry(id_bytes=3))[1] == "fcp_table_delta_distinct: `id_bytes` is 4 (int32 ids) or 8 (int64 ids)"
    assert _single(_entry(), report=0)[1] == "fcp_table_delta_distinct: `report` is null"
    assert _single(_entry(), workspace=0)[1] == "fcp_table_delta_distinct: `workspace` is null"
    assert _single(_entry(), report=A + 4)[1] == "fcp_table_delta_distinct: `report` is not 8-byte aligned"
    assert _single(_entry(rows=A + 4))[1] == "fcp_table_delta_distinct: `rows` is not 16-byte aligned (float32 rows of this dim)"


# ---- the launch count --------------------------------------------------------------------------------------------------------
def _class_of(dim):
    """ids only, or the (V, G) of the entry's rows"""
    return (0, 1) if dim == 0 else (TC.vec_of(dim), TC.group_of(dim))


def test_launches_is_five_plus_one_per_compact_class():
    assert _launches([]) == 0 and _launches([_entry()], n_tables=0) == 0
    assert _launches([_entry(n=0)] * 7) == 1                                  # the fold alone: zeros into the reports
    assert _launches([_entry()]) == 6 and _launches([_entry(dim=0)]) == 6
    rng = np.random.default_rng(3)
    for _ in range(40):
        entries, classes = [], set()
        for _k in range(int(rng.integers(1, 60))):
            dim, n = int(rng.choice((0, 0) + DC.ROW_DIMS)), int(rng.choice((0, 0, 1, 63, 64, 65, 257, 100000)))
            entries.append(_entry(dim=dim, n=n, id_bytes=int(rng.choice((4, 8)))))
            if n:
                classes.add(_class_of(dim))
        assert _launches(entries) == (5 + len(classes) if classes else 1), [(e.dim, e.n) for e in entries]
    assert _launches([_entry()], n_tables=-1) == -INV and _launches([_entry(), _entry(id_bytes=1)]) == -INV
    assert "entry 1: " in _lib.load().fcp_last_error().decode()


def test_launches_do_not_grow_with_the_number_of_entries():
    """The same entries repeated 1, 10 and 1000 times enqueue the same launches; every compact class there is — ids only and
    every (V, G) a dim can have — reaches the most a call can take, which stays within the documented 27."""
    base = [_entry(dim=d, n=n) for d, n in ((64, 1024), (16, 16), (0, 1024), (6, 3), (7, 1), (0, 9), (300, 2))]
    one = _launches(base)
    assert one == 5 + len({_class_of(e.dim) for e in base}) == 11
    assert _launches(base * 10) == one and _launches(base * 1000) == one
    # every (V, G) a dim can have — 18 of the 21 (tests/test_tables_rows_host.py says which three have no dim) — and ids only
    dims = {}
    for dim in list(DC.ROW_DIMS) + list(range(1, 300)):
        dims.setdefault(_class_of(dim), dim)
    assert len(dims) == 18
    full = [_entry(dim=d) for d in dims.values()] + [_entry(dim=0)]
    text = _prose()
    assert "a call enqueues at most 27 launches (of the 21, the dims that exist reach 18: 24)" in text
    assert _launches(full) == 24 <= 27 and _launches(full * 50) == 24
    rng = np.random.default_rng(11)
    for _ in range(20):
        picks = [full[i] for i in rng.integers(0, len(full), int(rng.integers(1, 400)))]
        assert 6 <= _launches(picks) <= 24


def test_the_deal_of_blocks():
    """Alone and while the lone grids sum to the cap or less an entry takes the single-table grid; past the cap every grid
    shrinks, no entry is left without a block, no block is idle and the call's grid stays within cap + n_tables.  The case
    file's own statement of the rule is checked against the library's."""
    L = _lib.load()
    assert int(L.fcp_tables_delta_deal_blocks()) == GC.DEAL_BLOCKS == 8192
    for ns in ([1], [DC.FULL_PASS + 1], [0, 5, 0], list(DC.SIZES), [DC.FULL_PASS + 1] + [1] * 200, GC.SCALED_NS, [3 * DC.FULL_PASS] * 20 + [1] * 50):
        entries = [_entry(dim=0, n=n, table_rows=1000) for n in ns]
        blocks = (C.c_int32 * len(ns))()
        grid = int(L.fcp_tables_delta_grid(_array(entries), len(ns), blocks))
        want = GC.deal(ns)
        assert list(blocks) == [b for b, _chunk in want] and grid == sum(blocks), ns[:5]
        lone = [GC.lone_blocks(n) for n in ns]
        if sum(lone) <= GC.DEAL_BLOCKS:
            assert list(blocks) == lone
        else:
            assert grid <= GC.DEAL_BLOCKS + len(ns) and all(1 <= b <= lb for b, lb, n in zip(blocks, lone, ns) if n)
        for (b, chunk), n in zip(want, ns):
            assert (b == 0) == (n == 0) and (n == 0 or (b - 1) * chunk < n <= b * chunk)     # no idle block
    assert sum(GC.lone_blocks(n) for n in GC.SCALED_NS) > GC.DEAL_BLOCKS
    assert int(L.fcp_tables_delta_grid(_array([_entry(n=-1)]), 1, None)) == -INV


# ---- the Python wrappers -----------------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_what_they_can_see():
    import torch
    from recom_amd import tables
    ids, rows = torch.arange(4), torch.zeros((4, 8))
    with pytest.raises(ValueError, match="entry 0: .*device to device"):              # host tensors
        tables.delta_distinct_grouped([ids], [rows], [10])
    with pytest.raises(ValueError, match="rows 1"):                                   # sequences of different lengths
        tables.delta_distinct_grouped_async([ids, ids], [rows], [10, 10])
    with pytest.raises(ValueError, match="table_rows"):
        tables.delta_distinct_grouped_async([ids, ids], None, [10])
    with pytest.raises(ValueError, match="table_rows"):
        tables.delta_distinct_grouped_async([ids], None, 10)
    assert tables.delta_distinct_grouped([], None, []) == [] and tables.delta_distinct_grouped_async([], [], []) == []
    with pytest.raises(ValueError, match="row_ids 1"):
        tables.apply_delta_grouped([rows, rows], [ids], [rows, rows])
    with pytest.raises(ValueError, match="digests 2"):
        tables.apply_delta_grouped([rows], [ids], [rows], digests=[1, 2])
    with pytest.raises(ValueError, match="entry 0: "):
        tables.apply_delta_grouped([rows], [ids], [rows])
    assert tables.apply_delta_grouped([], [], []) == [] and tables.apply_delta_grouped([], [], [], digests=[]) == ([], [])


# ---- code object -----------------------------------------------------------------------------------------------------------
def test_code_object_of_the_grouped_kernels(tmp_path):
    """clear, insert, classify, fold and the 22 compact kernels.  No kernel has scratch; LDS is what the unit's header states:
    the insert kernel's row table (16 KiB), the compact kernels' winner list and wave counts (ids only: the counts), the
    classify kernel's fold."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    asm = tmp_path / "fcp_tables_delta.s"
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S",
                           os.path.join(CSRC, "fcp_tables_delta.hip"), "-o", str(asm)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    kernels = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm.read_text(), re.S)}
    compact = {k for k in kernels if "fcp_tables_delta_compact_kernel" in k}
    assert len(compact) == 22 and len(kernels) == 26, sorted(kernels)

    def field(desc, name):
        return int(re.search(r"\.amdhsa_" + name + r" (\d+)", desc).group(1))
    for name, desc in sorted(kernels.items()):
        assert field(desc, "private_segment_fixed_size") == 0, f"{name}: uses scratch"
        lds = field(desc, "group_segment_fixed_size")
        if "insert_kernel" in name:
            assert lds == 2 * 4 * DC.LDS_SLOTS, name
        elif name in compact:
            assert lds == (16 if "ILi0ELi1E" in name else 1024 + 16), name
        elif "classify_kernel" in name:
            assert lds == 48, name
        else:
            assert lds == 0, name


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------
def test_the_plan_unit_alone_under_address_and_undefined_sanitizers(tmp_path):
    """recom_amd/csrc/fcp_tables_delta_plan.cc links without the GPU runtime and without any other unit; a stand-alone program
    (tests/native/tables_delta_plan_san.cc), both built with -fsanitize=address,undefined, drives the builder over random entry
    sets — prefix tables, record bounds, disjoint sections, the workspace formula — and the refusals, and prints `0 failures`
    with no sanitizer report.  Nothing is loaded into python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "tables_delta_plan_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "native", "tables_delta_plan_san.cc"), os.path.join(CSRC, "fcp_tables_delta_plan.cc"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr.lower() or "ubsan" in build.stderr.lower()):
        pytest.skip("libasan / libubsan not installed")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "20261021", "400"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-2:] == ["400 sets", "0 failures"], run.stdout[-2000:]
