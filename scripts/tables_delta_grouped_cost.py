"""What making a model's delta distinct costs in one call: fcp_tables_delta_distinct against one fcp_table_delta_distinct per
table, timed with HIP events and, per call, with perf_counter around the enqueue (the loop's cost is expected on the host side):

    grouped       ONE fcp_tables_delta_distinct over all entries, through the C ABI with the entry array and the workspace made
                  once — what a serving host does
    loop          one fcp_table_delta_distinct per entry, through the C ABI: the single-table entry of the same library, the
                  baseline
    grouped (py)  tables.delta_distinct_grouped_async: the wrapper validates every entry, allocates and builds the array per call

    steps   many       1000 entries x 1024 ids of dim 16 into 65 536-row tables, the ids of an entry pairwise distinct
            repeats    the same with every tenth id of an entry repeating an earlier one
            one        1 entry x 2^20 ids of dim 64 into a 16 M-row table, beside the single-table call: what the grouped front
                       (the record upload, the search) costs an entry that is alone
            chain      tables.apply_delta_grouped of the `repeats` delta into bf16 tables (distinct, update, one synchronise)
                       beside tables.update_rows_grouped of the same delta alone, each closed by a synchronise

    python scripts/tables_delta_grouped_cost.py [--out profiles/tables_delta_grouped.txt] [--min-ms 50]

The driver starts every step as a process of its own under `timeout` and stops at the first that fails; a step first checks the
grouped result against the loop's, byte for byte (a wrong kernel is refused, not timed).  Within a step the legs alternate: five
rounds, in each one window per leg of as many back-to-back calls as fill --min-ms, closed by an event synchronise; the median
window is reported with the spread.  No threshold: the figures are recorded.  Without a GPU the script fails: it never falls
back."""
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

STEPS = ("many", "repeats", "one", "chain")
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


def shape_of(step_name: str):
    """(dim, [(table_rows, n)] per entry, share of an entry's ids that repeat an earlier one)"""
    if step_name == "one":
        return 64, [(16_000_000, 1 << 20)], 0.0
    return 16, [(65536, 1024)] * 1000, 0.0 if step_name == "many" else 0.1


def step(args) -> dict:
    import torch
    from recom_amd import lib, synth, tables
    if not torch.cuda.is_available():
        raise SystemExit("NOT MEASURED: no GPU (there is no CPU fallback)")
    L = lib.load()
    dev = torch.device("cuda", 0)
    dim, sizes, repeats = shape_of(args.step)
    n_tables, total = len(sizes), sum(n for _tr, n in sizes)
    delta = synth.hash_table_torch(11, total, dim, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    ids, xs, d0 = [], [], 0
    for tr, n in sizes:
        i = torch.randperm(tr, device=dev, generator=gen)[:n].contiguous()
        if repeats:
            k = int(n * repeats)
            at = torch.randperm(n - 1, device=dev, generator=gen)[:k] + 1                      # position at >= 1 repeats position at // 2
            i[at] = i[at // 2]
        ids.append(i)
        xs.append(delta[d0:d0 + n])
        d0 += n
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    ns = (C.c_int64 * n_tables)(*[n for _tr, n in sizes])

    def outputs():
        return (torch.empty((total,), dtype=torch.int64, device=dev), torch.empty((total, dim), dtype=torch.float32, device=dev),
                torch.empty((n_tables, 4), dtype=torch.int64, device=dev))
    g_ids, g_rows, g_reports = outputs()
    l_ids, l_rows, l_reports = outputs()
    workspace = torch.empty((int(L.fcp_tables_delta_workspace_bytes(ns, n_tables)) // 8,), dtype=torch.int64, device=dev)
    one_ws = torch.empty((max(int(L.fcp_table_delta_workspace_bytes(n)) for _tr, n in sizes) // 8,), dtype=torch.int64, device=dev)
    arr = (lib.TableDeltaEntry * n_tables)()
    loop_args, d0 = [], 0
    for k, (tr, n) in enumerate(sizes):
        arr[k] = lib.TableDeltaEntry(ids[k].data_ptr(), xs[k].data_ptr(), g_ids[d0:].data_ptr(), g_rows[d0:].data_ptr(), None, tr, n, 8, dim)
        loop_args.append((p(ids[k]), 8, p(xs[k]), dim, n, tr, p(l_ids[d0:]), p(l_rows[d0:]), None, C.c_void_p(l_reports[k].data_ptr()), p(one_ws), 0,
                          C.c_void_p(stream)))
        d0 += n
    launches = int(L.fcp_tables_delta_launches(arr, n_tables))

    def grouped():
        lib.check(L.fcp_tables_delta_distinct(arr, n_tables, p(g_reports), p(workspace), 0, C.c_void_p(stream)), "fcp_tables_delta_distinct")

    def loop():
        for a in loop_args:
            L.fcp_table_delta_distinct(*a)
    g_rows.zero_(), l_rows.zero_()
    grouped()
    loop()
    torch.cuda.synchronize()
    m = int(g_reports[:, 1].sum())
    if not (torch.equal(g_ids, l_ids) and torch.equal(g_reports, l_reports) and torch.equal(g_rows.view(torch.int32), l_rows.view(torch.int32))) or \
            m != total - int(g_reports[:, 2].sum()) or bool(repeats) != bool(int(g_reports[:, 2].sum())):
        raise SystemExit(f"{args.step}: the grouped call and the loop disagree; nothing timed")
    if args.step == "chain":
        store = torch.zeros((sum(tr for tr, _n in sizes), dim), dtype=torch.bfloat16, device=dev)
        tabs, r0 = [], 0
        for tr, _n in sizes:
            tabs.append(store[r0:r0 + tr])
            r0 += tr
        d_ids, d0 = [], 0
        for _tr, n in sizes:
            d_ids.append(g_ids[d0:d0 + n])
            d0 += n
        ext = torch.cuda.current_stream(dev)

        def update_alone():
            tables.update_rows_grouped(tabs, d_ids, xs)
            ext.synchronize()
        legs = {"apply_delta_grouped": lambda: tables.apply_delta_grouped(tabs, ids, xs), "update_rows_grouped": update_alone}
    else:
        legs = {"grouped": grouped, "loop": loop,
                "grouped (py)": lambda: tables.delta_distinct_grouped_async(ids, xs, [tr for tr, _n in sizes])}
    timed = alternate(torch, legs, args.min_ms)
    return {"step": args.step, "entries": n_tables, "ids": total, "dim": dim, "launches": launches, "distinct": m,
            "device": torch.cuda.get_device_name(0),
            "legs": {name: {"us_per_call": ms * 1e3, "spread_us": spread * 1e3, "host_us_per_call": host, "calls_per_window": calls}
                     for name, (ms, spread, host, calls) in timed.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables_delta_grouped.txt"))
    ap.add_argument("--min-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--step", choices=STEPS, help="(one step, as the driver starts it)")
    ap.add_argument("--note", default="", help="a paragraph appended to the profile")
    args = ap.parse_args()
    if args.step:
        print("RECORD " + json.dumps(step(args)), flush=True)
        return
    records = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", name, "--min-ms", str(args.min_ms)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if proc.returncode != 0:                          # a failure, a fault, a time limit: nothing more is started
            raise SystemExit(f"step {name} ended with status {proc.returncode}; stopped")
        records.append(json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:]))
        print(f"{name}: done", flush=True)
    lines = [f"A model's delta made distinct in one call: fcp_tables_delta_distinct against one fcp_table_delta_distinct per entry ({records[0]['device']})",
             "grouped / loop: through the C ABI, arguments made once; (py): through recom_amd.tables.  many: 1000 x 1024 distinct ids of dim 16;",
             "repeats: the same, every tenth id repeating an earlier one; one: 1 x 2^20 ids of dim 64 (loop = the single-table call);",
             "chain: tables.apply_delta_grouped of the `repeats` delta into bf16 tables beside tables.update_rows_grouped alone, both with",
             "their synchronise.  launches: what one grouped distinct call enqueues, the record upload included.",
             f"us per call: median of {ROUNDS} alternating windows between two events (spread = max - min); host us: perf_counter around",
             "the enqueue, per call",
             f"{'step':>8} {'entries':>7} {'ids':>8} {'launches':>8} {'leg':>20} {'us/call':>10} {'spread':>8} {'host us':>9} {'vs first':>9} calls"]
    for r in records:
        first = next(iter(r["legs"].values()))["us_per_call"]
        for name, leg in r["legs"].items():
            lines.append(f"{r['step']:>8} {r['entries']:>7} {r['ids']:>8} {r['launches']:>8} {name:>20} {leg['us_per_call']:>10.1f} {leg['spread_us']:>8.1f} "
                         f"{leg['host_us_per_call']:>9.1f} {leg['us_per_call'] / first:>9.2f} {leg['calls_per_window']}")
    if args.note:
        lines += ["", args.note]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    print(json.dumps({"records": records}), flush=True)


if __name__ == "__main__":
    main()
