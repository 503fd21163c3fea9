"""What a model's delta costs in one call: fcp_tables_update_rows / fcp_tables_read_rows against one fcp_table_update_rows /
fcp_table_read_rows per table, timed with HIP events and, per call, with perf_counter around the enqueue (the loop's cost is
expected on the host side):

    grouped       ONE fcp_tables_update_rows (fcp_tables_read_rows) over all entries, through the C ABI with the entry array and
                  the workspace made once — what a serving host does
    loop          one fcp_table_update_rows (fcp_table_read_rows) per entry, through the C ABI: unchanged code, the parent's
    grouped (py)  tables.update_rows_grouped / read_rows_grouped: the wrapper validates every entry and builds the array per call
    loop (py)     a Python loop of tables.update_rows / read_rows
    single        ONE fcp_table_update_rows (fcp_table_read_rows) of the same total rows into one table: the floor

    shapes  many   1000 entries x 1024 rows of dim 16 into 65 536-row tables, q8 and bf16
            skew   1000 entries of dim 16: one of 1 M rows (a 2 M-row table), the rest 16 rows, q8
            one    1 entry x 1 M rows of dim 64 into a 16 M-row table, q8: the shape of scripts/table_update_cost.py, whose
                   figure for the single call (profiles/table_update.txt) the `single` leg here should reproduce

    python scripts/tables_update_grouped_cost.py [--out profiles/tables_update_grouped.txt] [--min-ms 50]

The driver starts every (op, shape, kind) step as a process of its own under `timeout` and stops at the first that fails; a
step first checks the grouped result against the loop's, byte for byte (a wrong kernel is refused, not timed).  Within a step
the legs alternate: five rounds, in each one window per leg of as many back-to-back calls as fill --min-ms, closed by an event
synchronise; the median window is reported with the spread.  No threshold: the figures are recorded.  Without a GPU the script
fails: it never falls back."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("many", "q8"), ("many", "bf16"), ("skew", "q8"), ("one", "q8"))
OPS = ("update", "read")
ROUNDS = 5
STEP_TIMEOUT_S = 240


def window(torch, fn, calls: int):
    """(ms per call between two events, host us per call around the enqueue) of `calls` back-to-back calls"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    host = time.perf_counter() - t0
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls, host * 1e6 / calls


def alternate(torch, legs: dict, min_ms: float) -> dict:
    """name -> (median ms per call, spread ms, median host us per call, calls per window): a warm-up of every leg, then ROUNDS
    rounds of one window per leg, the legs taking turns."""
    calls = {}
    for name, fn in legs.items():
        fn()
        fn()
        torch.cuda.synchronize()
        calls[name] = max(3, int(min_ms / max(window(torch, fn, 1)[0], 1e-3)) + 1)
    seen = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            seen[name].append(window(torch, fn, calls[name]))
    return {name: (statistics.median(w[0] for w in v), max(w[0] for w in v) - min(w[0] for w in v), statistics.median(w[1] for w in v),
                   calls[name]) for name, v in seen.items()}


def shape_of(shape: str):
    """(dim, [(table_rows, n)] per entry)"""
    if shape == "many":
        return 16, [(65536, 1024)] * 1000
    if shape == "skew":
        return 16, [(65536, 16)] * 500 + [(1 << 21, 1_000_000)] + [(65536, 16)] * 499
    return 64, [(16_000_000, 1_000_000)]


def step(args) -> dict:
    import torch
    from recom_amd import lib, synth, tables
    if not torch.cuda.is_available():
        raise SystemExit("NOT MEASURED: no GPU (there is no CPU fallback)")
    L = lib.load()
    dev = torch.device("cuda", 0)
    kind, op = args.kind, args.op
    dim, sizes = shape_of(args.shape)
    dtype = {"q8": torch.uint8, "bf16": torch.bfloat16}[kind]
    width = dim + (8 if kind == "q8" else 0)
    total = sum(n for _tr, n in sizes)
    # the tables: views of one allocation (zeros: valid rows in every format); ids pairwise distinct per entry; rows from one master
    all_rows = sum(tr for tr, _n in sizes)
    store = torch.zeros((all_rows, width), dtype=dtype, device=dev)
    twin_store = torch.zeros_like(store)
    delta = synth.hash_table_torch(11, total, dim, dev)
    outs = torch.empty((total, dim), dtype=torch.float32, device=dev)
    tabs, twins, ids, xs, os_ = [], [], [], [], []
    r0 = d0 = 0
    perm = {}
    for tr, n in sizes:
        if tr not in perm or n > 4096:
            perm[tr] = torch.randperm(tr, device=dev)
        start = int(torch.randint(0, tr - n + 1, (1,)).item())
        ids.append(perm[tr][start:start + n].contiguous())
        tabs.append(store[r0:r0 + tr]), twins.append(twin_store[r0:r0 + tr])
        xs.append(delta[d0:d0 + n]), os_.append(outs[d0:d0 + n])
        r0, d0 = r0 + tr, d0 + n
    # the single call: the same total rows, distinct ids over the whole store
    one_ids = torch.randperm(all_rows, device=dev)[:total].contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    K = lib.TABLE_KINDS[kind]

    def entries_for(tables_, rows_):
        return (lib.TableRows * len(sizes))(*[lib.TableRows(t.data_ptr(), i.data_ptr(), r.data_ptr(), int(t.shape[0]), int(i.shape[0]), K, dim)
                                             for t, i, r in zip(tables_, ids, rows_)])
    workspace = torch.empty((int(L.fcp_tables_rows_workspace_bytes(len(sizes))) // 8,), dtype=torch.int64, device=dev)
    launches = int(L.fcp_tables_rows_launches(entries_for(tabs, xs), len(sizes)))

    if op == "update":
        arr, twin_arr = entries_for(tabs, xs), entries_for(twins, xs)
        loop_args = [(p(t), K, int(t.shape[0]), dim, p(i), p(r), int(i.shape[0]), None, 0, C.c_void_p(stream)) for t, i, r in zip(twins, ids, xs)]

        def grouped(a=arr):
            lib.check(L.fcp_tables_update_rows(a, len(sizes), None, p(workspace), 0, C.c_void_p(stream)), "fcp_tables_update_rows")

        def loop():
            for a in loop_args:
                L.fcp_table_update_rows(*a)
        legs = {"grouped": grouped, "loop": loop,
                "grouped (py)": lambda: tables.update_rows_grouped(tabs, ids, xs), "loop (py)": lambda: [tables.update_rows(t, i, r) for t, i, r in zip(twins, ids, xs)],
                "single": lambda: tables.update_rows(store, one_ids, delta)}
        grouped()
        loop()
        torch.cuda.synchronize()
        if not torch.equal(store.view(torch.uint8), twin_store.view(torch.uint8)) or not bool((store != 0).any()):
            raise SystemExit(f"{op} {args.shape} {kind}: the grouped call and the loop disagree; nothing timed")
        del twin_arr
    else:
        for t, i, r in zip(tabs, ids, xs):
            tables.update_rows(t, i, r)
        twin_outs = torch.empty_like(outs)
        touts, d0 = [], 0
        for _tr, n in sizes:
            touts.append(twin_outs[d0:d0 + n])
            d0 += n
        arr = entries_for(tabs, os_)
        loop_args = [(p(o), p(t), K, int(t.shape[0]), dim, p(i), int(i.shape[0]), 0, C.c_void_p(stream)) for t, i, o in zip(tabs, ids, touts)]

        def grouped():
            lib.check(L.fcp_tables_read_rows(arr, len(sizes), p(workspace), 0, C.c_void_p(stream)), "fcp_tables_read_rows")

        def loop():
            for a in loop_args:
                L.fcp_table_read_rows(*a)
        legs = {"grouped": grouped, "loop": loop,
                "grouped (py)": lambda: tables.read_rows_grouped(tabs, ids, out=os_), "loop (py)": lambda: [tables.read_rows(t, i, out=o) for t, i, o in zip(tabs, ids, touts)],
                "single": lambda: tables.read_rows(store, one_ids, out=outs)}
        grouped()
        loop()
        torch.cuda.synchronize()
        if not torch.equal(outs.view(torch.int32), twin_outs.view(torch.int32)) or not bool((outs != 0).any()):
            raise SystemExit(f"{op} {args.shape} {kind}: the grouped call and the loop disagree; nothing timed")
    timed = alternate(torch, legs, args.min_ms)
    row_bytes = tables.row_bytes(kind, dim)
    need = total * (8 + 4 * dim + row_bytes)
    return {"op": op, "shape": args.shape, "kind": kind, "entries": len(sizes), "rows": total, "dim": dim, "launches": launches,
            "device": torch.cuda.get_device_name(0),
            "legs": {name: {"us_per_call": ms * 1e3, "spread_us": spread * 1e3, "host_us_per_call": host, "calls_per_window": calls,
                            "gbps_needed_bytes": need / ms / 1e6} for name, (ms, spread, host, calls) in timed.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables_update_grouped.txt"))
    ap.add_argument("--min-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--op", choices=OPS, help="(one step, as the driver starts it)")
    ap.add_argument("--shape", choices=("many", "skew", "one"))
    ap.add_argument("--kind", choices=("q8", "bf16"))
    ap.add_argument("--note", default="", help="a paragraph appended to the profile")
    args = ap.parse_args()
    if args.op:
        print("RECORD " + json.dumps(step(args)), flush=True)
        return
    records = []
    for op in OPS:
        for shape, kind in STEPS:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--op", op, "--shape", shape,
                   "--kind", kind, "--min-ms", str(args.min_ms)]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if proc.returncode != 0:                          # a failure, a fault, a time limit: nothing more is started
                raise SystemExit(f"step {op} {shape} {kind} ended with status {proc.returncode}; stopped")
            records.append(json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:]))
            print(f"{op} {shape} {kind}: done", flush=True)
    lines = [f"A model's delta in one call: fcp_tables_update_rows / fcp_tables_read_rows against one single-table call per entry ({records[0]['device']})",
             "grouped / loop: through the C ABI, arguments made once; (py): through recom_amd.tables; single: one single-table call of the",
             "same total rows into one table.  many: 1000 x 1024 rows of dim 16; skew: 1000 entries, one of 1 M rows, the rest 16, dim 16;",
             "one: 1 x 1 M rows of dim 64 into a 16 M-row table.  launches: what one grouped call enqueues, the record upload included.",
             f"us per call: median of {ROUNDS} alternating windows between two events (spread = max - min); host us: perf_counter around",
             "the enqueue, per call; GB/s = (ids + float32 rows + table rows) / time",
             f"{'op':>6} {'shape':>5} {'kind':>5} {'launches':>8} {'leg':>13} {'us/call':>10} {'spread':>8} {'host us':>9} {'GB/s':>7} {'vs grouped':>10} calls"]
    for r in records:
        for name, leg in r["legs"].items():
            lines.append(f"{r['op']:>6} {r['shape']:>5} {r['kind']:>5} {r['launches']:>8} {name:>13} {leg['us_per_call']:>10.1f} {leg['spread_us']:>8.1f} "
                         f"{leg['host_us_per_call']:>9.1f} {leg['gbps_needed_bytes']:>7.0f} {leg['us_per_call'] / r['legs']['grouped']['us_per_call']:>10.2f} "
                         f"{leg['calls_per_window']}")
    if args.note:
        lines += ["", args.note]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    print(json.dumps({"records": records}), flush=True)


if __name__ == "__main__":
    main()
