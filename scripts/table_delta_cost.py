"""What making a delta's ids distinct costs (profiles/table_delta.txt).

One delta of 2^20 ids and float32 rows of dim 64 against a q8 table of 16 M rows, in four id patterns: pairwise distinct, 10 % of
the positions repeating another position's id, Zipf(1.05), all equal.  Per pattern, the median of warm HIP-event timings of
  distinct          fcp_table_delta_distinct (its five launches), outputs and workspace allocated once — once per library:
                    the one the package loads and every `--variant NAME=LIBRARY`, another build's (how the insert phase was
                    chosen: the variant on file was a build of the commit that introduced the kernel with the plain kernel
                    in it, one global claim and max per position; `make -C recom_amd/csrc OUT=<dir>` at any commit gives
                    such a library);
  distinct+update   the same followed by fcp_table_update_rows of the padded outputs into the q8 table;
  update            plain fcp_table_update_rows of the delta as it stands (what a distinct delta costs today; with repeated ids
                    its bytes are unspecified, its time is not);
  copy              a device-to-device copy of the rows: the floor for the row traffic;
  torch             the composition the entry replaces: unique(return_inverse) + scatter_reduce(amax) of the positions + a sort
                    of the winners + index_select of ids and rows (its result is compared with the entry's: the line says `equal`).
No threshold anywhere: the times are recorded.

    python scripts/table_delta_cost.py [--ids 1048576] [--dim 64] [--rows 16777216] [--reps 20] [--variant NAME=LIBRARY ...]
                                       [--out profiles/table_delta.txt]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD = """fcp_table_delta_distinct: what it costs beside the update, a copy and the torch composition
=========================================================================================
Produced by scripts/table_delta_cost.py (one MI355X, one child process under its own timeout; medians of {reps} warm HIP-event
timings per leg).  {ids} ids (int64) and float32 rows of dim {dim} against a q8 table of {rows} rows.  `shipped` is the library
the package loads; the other names are other builds of the library (--variant).

    {cmdline}

"""
PATTERNS = ("distinct", "repeat10", "zipf", "equal")


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


def draw(torch, pattern: str, n: int, rows: int, dev):
    import numpy as np
    g = torch.Generator().manual_seed(11)
    if pattern == "distinct":
        return torch.randperm(rows, generator=g)[:n].to(dev)
    if pattern == "repeat10":
        ids = torch.randperm(rows, generator=g)[:n]
        at = torch.randperm(n, generator=g)[:n // 10]
        ids[at] = ids[torch.randint(0, n, (n // 10,), generator=g)]
        return ids.to(dev)
    if pattern == "zipf":
        return torch.from_numpy((np.random.default_rng(11).zipf(1.05, size=n).astype(np.int64) - 1) % rows).to(dev)
    return torch.full((n,), rows // 3, dtype=torch.int64, device=dev)


def child(n: int, dim: int, rows: int, reps: int, variants, out_path: str, cmdline: str) -> None:
    import torch
    from recom_amd import lib as _lib
    from recom_amd import tables
    dev = torch.device("cuda", 0)
    shipped = _lib.load()
    libs = [("shipped", shipped)]
    for name, path in variants:
        V = C.CDLL(path)
        V.fcp_table_delta_distinct.argtypes = shipped.fcp_table_delta_distinct.argtypes
        libs.append((name, V))
    stream = torch.cuda.current_stream(dev).cuda_stream
    table = torch.zeros((rows, dim + 8), dtype=torch.uint8, device=dev)
    delta_rows = torch.randn((n, dim), generator=torch.Generator().manual_seed(3)).to(dev)
    ids_out = torch.empty((n,), dtype=torch.int64, device=dev)
    pos_out = torch.empty((n,), dtype=torch.int64, device=dev)
    rows_out = torch.empty_like(delta_rows)
    twin = torch.empty_like(delta_rows)
    report = torch.empty((4,), dtype=torch.int64, device=dev)
    ws = torch.empty((int(shipped.fcp_table_delta_workspace_bytes(n)) // 8,), dtype=torch.int64, device=dev)
    arange = torch.arange(n, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    lines = []

    def say(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    for pattern in PATTERNS:
        ids = draw(torch, pattern, n, rows, dev)

        def distinct(L=shipped):
            _lib.check(L.fcp_table_delta_distinct(p(ids), 8, p(delta_rows), dim, n, rows, p(ids_out), p(rows_out), p(pos_out), p(report), p(ws),
                                                  0, C.c_void_p(stream)), "fcp_table_delta_distinct")

        def update(i=ids, r=delta_rows):
            _lib.check(shipped.fcp_table_update_rows(p(table), _lib.TABLE_KINDS["q8"], rows, dim, p(i), p(r), n, None, 0, C.c_void_p(stream)),
                       "fcp_table_update_rows")

        def both():
            distinct()
            update(ids_out, rows_out)

        def composition():
            u, inv = torch.unique(ids, return_inverse=True)
            last = torch.full((u.numel(),), -1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, arange, "amax")
            win = torch.sort(last).values
            return ids.index_select(0, win), delta_rows.index_select(0, win), win

        distinct()
        want_ids, want_rows, want_pos = composition()
        torch.cuda.synchronize()
        m = int(report[1])
        same = (m == want_ids.numel() and bool((ids_out[:m] == want_ids).all()) and bool((pos_out[:m] == want_pos).all())
                and bool((rows_out[:m].view(torch.int32) == want_rows.view(torch.int32)).all()) and bool((ids_out[m:] == -1).all()))
        say(f"{pattern:9s} report (n, distinct, duplicates, skipped) = {tuple(report.cpu().tolist())}; the torch composition's result: "
            f"{'equal' if same else 'DIFFERENT'}")
        legs = [(f"distinct [{name}]", lambda L=L: distinct(L)) for name, L in libs]
        legs += [("distinct+update", both), ("update", update), ("copy", lambda: twin.copy_(delta_rows)), ("torch", composition)]
        for name, fn in legs:
            med, lo, hi = timed(torch, fn, reps)
            say(f"{pattern:9s} {name:22s} median {1e3 * med:9.1f} us  (min {1e3 * lo:.1f}, max {1e3 * hi:.1f})")
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(HEAD.format(reps=reps, ids=n, dim=dim, rows=rows, cmdline=cmdline) + "\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIBRARY", help="another build of libfcp_hip.so to time the entry of")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_delta.txt"), help="the record this run writes")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    variants = [tuple(v.split("=", 1)) for v in args.variant]
    if args.child:
        cmdline = f"python scripts/table_delta_cost.py --ids {args.ids} --dim {args.dim} --rows {args.rows} --reps {args.reps}"
        cmdline += "".join(f" --variant {n}=<its build of libfcp_hip.so>" for n, _ in variants)
        child(args.ids, args.dim, args.rows, args.reps, variants, args.out, cmdline)
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--ids", str(args.ids),
           "--dim", str(args.dim), "--rows", str(args.rows), "--reps", str(args.reps), "--out", args.out] + [f"--variant={n}={p}" for n, p in variants]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
