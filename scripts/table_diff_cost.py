"""What diffing a new float32 master against a served table costs (profiles/table_diff.txt).

One master of 16 M rows of dim 64 against a q8, a bf16 and a float32 table of the same rows, with 0 %, 1 % and 100 % of the rows
changed (every 100th row / every row + 1.0 in every element).  Per table format and share, in ONE process, the median of warm
HIP-event timings of
  diff              fcp_table_diff with rows_out (its three launches), outputs and workspace allocated once;
  diff ids only     the same without rows_out;
  convert           fcp_table_convert of the same rows into a temporary table of the format (float32: none — a copy is all
                    there is);
  copy              a device-to-device copy of the bytes the diff reads — the new rows and the stored rows: the floor;
  composition       what the entry replaces: fcp_table_convert into a temporary + a torch byte compare + nonzero + index_select
                    of the changed rows (float32: the compare on the rows themselves).  Its ids and rows are compared with the
                    entry's: the line says `equal`.
No threshold anywhere: the times are recorded.

    python scripts/table_diff_cost.py [--rows 16777216] [--dim 64] [--reps 20] [--out profiles/table_diff.txt]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD = """fcp_table_diff: what it costs beside the conversion, a copy and the composition it replaces
=======================================================================================
Produced by scripts/table_diff_cost.py (one MI355X, one child process under its own timeout; medians of {reps} warm HIP-event
timings per leg).  A float32 master of {rows} rows of dim {dim} against a table of the same rows in each format; `read` is the
bytes the diff reads (the new rows and the stored rows), and GB/s is read / median.

    {cmdline}

"""
KINDS = ("q8", "bf16", "f32")
SHARES = ((0, "0 %"), (100, "1 %"), (1, "100 %"))       # (every how-manieth row changes, 0: none), label


def timed(torch, fn, reps: int):
    """median and spread, in ms, of `reps` warm runs of fn between two events on the current stream"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def child(rows: int, dim: int, reps: int, out_path: str, cmdline: str) -> None:
    import torch
    from recom_amd import lib as _lib
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    base = torch.randn((rows, dim), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    new = torch.empty_like(base)
    twin = torch.empty_like(base)
    ids_out = torch.empty((rows,), dtype=torch.int64, device=dev)
    rows_out = torch.empty_like(base)
    report = torch.empty((4,), dtype=torch.int64, device=dev)
    ws = torch.empty((int(L.fcp_table_diff_workspace_bytes(rows)) // 8,), dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    lines = []

    def say(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    for kind in KINDS:
        table = base.clone() if kind == "f32" else tables.convert(base, kind)
        table_twin = torch.empty_like(table)
        temporary = None if kind == "f32" else torch.empty_like(table)
        read = rows * (4 * dim + tables.row_bytes(kind, dim))
        for every, label in SHARES:
            new.copy_(base)
            if every:
                new[::every] += 1.0

            def diff(with_rows=True):
                _lib.check(L.fcp_table_diff(p(table), _lib.TABLE_KINDS[kind], rows, dim, p(new), _lib.TABLE_KINDS["f32"], 0, rows, p(ids_out),
                                            p(rows_out) if with_rows else None, p(report), p(ws), 0, C.c_void_p(stream)), "fcp_table_diff")

            def convert():
                tables.convert(new, kind, out=temporary)

            def copy():
                twin.copy_(new)
                table_twin.copy_(table)

            def composition():
                if kind == "f32":
                    changed = (new.view(torch.int32) != table.view(torch.int32)).any(dim=1)
                else:
                    convert()
                    as_words = torch.int16 if kind != "q8" else torch.uint8
                    changed = (temporary.view(as_words) != table.view(as_words)).any(dim=1)
                ids = torch.nonzero(changed).view(-1)
                return ids, new.index_select(0, ids)

            diff()
            want_ids, want_rows = composition()
            torch.cuda.synchronize()
            m = int(report[1])
            same = (m == want_ids.numel() and bool((ids_out[:m] == want_ids).all()) and bool((ids_out[m:] == -1).all())
                    and bool((rows_out[:m].view(torch.int32) == want_rows.view(torch.int32)).all()))
            del want_ids, want_rows
            say(f"{kind:4s} {label:5s} report (rows, changed, first, last) = {tuple(report.cpu().tolist())}; read {read / 1e9:.2f} GB; "
                f"the composition's result: {'equal' if same else 'DIFFERENT'}")
            legs = [("diff", diff), ("diff ids only", lambda: diff(False))]
            legs += [("convert", convert)] if kind != "f32" else []
            legs += [("copy", copy), ("composition", composition)]
            for name, fn in legs:
                med, lo, hi = timed(torch, fn, reps)
                rate = f"  {read / med / 1e6:7.0f} GB/s" if name.startswith("diff") or name == "copy" else ""
                say(f"{kind:4s} {label:5s} {name:14s} median {1e3 * med:9.1f} us  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f}){rate}")
        del table, table_twin, temporary
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(HEAD.format(reps=reps, dim=dim, rows=rows, cmdline=cmdline) + "\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_diff.txt"), help="the record this run writes")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        child(args.rows, args.dim, args.reps, args.out, f"python scripts/table_diff_cost.py --rows {args.rows} --dim {args.dim} --reps {args.reps}")
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows),
           "--dim", str(args.dim), "--reps", str(args.reps), "--out", args.out]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
