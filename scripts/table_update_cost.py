"""What a row-granular table update costs: a 16 M-row table of dim 64, n = 1 M pairwise distinct ids — random and sorted —
for q8 and bf16, timed with HIP events:

    fused     tables.update_rows: fcp_table_update_rows, one pass
    two-pass  (a) what a PyTorch caller had before: fcp_table_convert of the n float32 rows into a temporary, then
              torch.index_copy_ of the temporary into the table
    contig    (b) fcp_table_convert of the same n rows into rows [0, n) of the table: the floor without a scatter

and tables.read_rows against tables.convert(table[ids], "f32") (torch's gather into a temporary, then the conversion).

    python scripts/table_update_cost.py [--out profiles/table_update.txt] [--rows 16000000] [--n 1000000] [--dim 64]

The driver starts every (kind, order) step as a process of its own under `timeout` and stops at the first that fails; a step
first checks the fused result against the two-pass one, byte for byte (a wrong kernel is refused, not timed).  Within a
step the legs alternate: five rounds, in each one window per leg of as many back-to-back calls as fill --min-ms, closed by
an event synchronise; the median window is reported with the spread.  No threshold: the figures are recorded.  Without a GPU
the script fails: it never falls back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("q8", "bf16")
ORDERS = ("random", "sorted")
ROUNDS = 5
STEP_TIMEOUT_S = 240


def window(torch, fn, calls: int) -> float:
    """ms per call of `calls` back-to-back calls between two events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def alternate(torch, legs: dict, min_ms: float) -> dict:
    """name -> (median ms per call, spread ms, calls per window): a warm-up of every leg, then ROUNDS rounds of one window
    per leg, the legs taking turns."""
    calls = {}
    for name, fn in legs.items():
        fn()
        fn()
        calls[name] = max(3, int(min_ms / max(window(torch, fn, 1), 1e-3)) + 1)
    seen = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            seen[name].append(window(torch, fn, calls[name]))
    return {name: (statistics.median(v), max(v) - min(v), calls[name]) for name, v in seen.items()}


def step(args) -> dict:
    import torch
    from recom_amd import synth, tables
    if not torch.cuda.is_available():
        raise SystemExit("NOT MEASURED: no GPU (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    rows, n, dim, kind = args.rows, args.n, args.dim, args.kind
    master = synth.hash_table_torch(7, rows, dim, dev)
    table = tables.convert(master, kind)
    del master
    delta = synth.hash_table_torch(11, n, dim, dev)
    ids = torch.randperm(rows, device=dev)[:n].contiguous()
    if args.order == "sorted":
        ids = ids.sort().values.contiguous()
    assert ids.dtype == torch.int64 and int(torch.unique(ids).numel()) == n
    row_bytes = tables.row_bytes(kind, dim)

    def two_pass():
        table.index_copy_(0, ids, tables.convert(delta, kind))

    # the fused entry writes what the two-pass route writes
    twin = table.clone()
    tables.update_rows(table, ids, delta)
    twin.index_copy_(0, ids, tables.convert(delta, kind))
    torch.cuda.synchronize()
    if not bool((table.view(torch.uint8) == twin.view(torch.uint8)).all()):
        raise SystemExit(f"{kind} {args.order}: update_rows and convert + index_copy_ disagree; nothing timed")
    del twin
    out = torch.empty((n, dim), dtype=torch.float32, device=dev)
    got = tables.read_rows(table, ids)
    want = tables.convert(table[ids], "f32")
    torch.cuda.synchronize()
    if not bool((got.view(torch.int32) == want.view(torch.int32)).all()):
        raise SystemExit(f"{kind} {args.order}: read_rows and convert(table[ids]) disagree; nothing timed")
    del got, want
    torch.cuda.empty_cache()
    timed = alternate(torch, {"update fused": lambda: tables.update_rows(table, ids, delta),
                              "update two-pass": two_pass,
                              "update contig": lambda: tables.convert(delta, kind, out=table),
                              "read fused": lambda: tables.read_rows(table, ids, out=out),
                              "read two-pass": lambda: tables.convert(table[ids], "f32", out=out)}, args.min_ms)
    # bytes the algorithm needs: ids + float32 rows on one side, table rows on the other
    need = {"update": n * (8 + 4 * dim + row_bytes), "read": n * (8 + 4 * dim + row_bytes)}
    return {"kind": kind, "order": args.order, "rows": rows, "n": n, "dim": dim, "device": torch.cuda.get_device_name(0),
            "legs": {name: {"us_per_call": ms * 1e3, "spread_us": spread * 1e3, "calls_per_window": calls,
                            "gbps_needed_bytes": need[name.split()[0]] / ms / 1e6} for name, (ms, spread, calls) in timed.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_update.txt"))
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--min-ms", type=float, default=100.0, help="least length of a timed window")
    ap.add_argument("--kind", choices=KINDS, help="(one step, as the driver starts it)")
    ap.add_argument("--order", choices=ORDERS)
    args = ap.parse_args()
    if args.kind:
        print("RECORD " + json.dumps(step(args)), flush=True)
        return
    records = []
    for kind in KINDS:
        for order in ORDERS:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--kind", kind, "--order", order,
                   "--rows", str(args.rows), "--n", str(args.n), "--dim", str(args.dim), "--min-ms", str(args.min_ms)]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if proc.returncode != 0:                          # a failure, a fault, a time limit: nothing more is started
                raise SystemExit(f"step {kind} {order} ended with status {proc.returncode}; stopped")
            records.append(json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:]))
            print(f"{kind} {order}: done", flush=True)
    lines = [f"Row-granular update and read of a [{args.rows}, {args.dim}] table, n = {args.n} pairwise distinct ids ({records[0]['device']})",
             "fused: fcp_table_update_rows / fcp_table_read_rows; two-pass: fcp_table_convert into a temporary + torch.index_copy_, or",
             "torch's gather table[ids] + fcp_table_convert; contig: fcp_table_convert of the same n rows into rows [0, n), no scatter.",
             f"us per call: median of {ROUNDS} alternating windows (spread = max - min); GB/s = (ids + float32 rows + table rows) / time",
             f"{'kind':>5} {'ids':>7} {'leg':>16} {'us/call':>9} {'spread':>7} {'GB/s':>7} {'vs fused':>8} calls"]
    for r in records:
        for name, leg in r["legs"].items():
            fused = r["legs"][name.split()[0] + " fused"]["us_per_call"]
            lines.append(f"{r['kind']:>5} {r['order']:>7} {name:>16} {leg['us_per_call']:>9.1f} {leg['spread_us']:>7.1f} "
                         f"{leg['gbps_needed_bytes']:>7.0f} {leg['us_per_call'] / fused:>8.2f} {leg['calls_per_window']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    print(json.dumps({"records": records}), flush=True)


if __name__ == "__main__":
    main()
