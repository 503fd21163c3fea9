"""What verifying a model's tables costs in one call: fcp_tables_digest against one fcp_table_digest / fcp_table_digest_rows per
table, timed with HIP events and, per call, with perf_counter around the enqueue (the loop's cost is expected on the host side):

    grouped       ONE fcp_tables_digest over all entries, through the C ABI with the entry array, the results and the workspace
                  made once — what a serving host does
    loop          one fcp_table_digest (fcp_table_digest_rows) per entry on the same stream, through the C ABI, no synchronise in
                  between: unchanged code, the parent's
    single        ONE fcp_table_digest of the same total bytes as one table: the floor
    update        (by id) ONE fcp_tables_update_rows of the delta, alone
    tracked       (by id) fcp_tables_digest of the delta's rows, fcp_tables_update_rows, fcp_tables_digest again: three calls
    tracked (py)  (by id) tables.update_rows_grouped_tracked: the wrapper validates, allocates and synchronises per call

    shapes  many   1000 entries x 16 384 rows of dim 16, q8 and bf16
            one    1 entry x 16 M rows of dim 64, q8 and bf16
            ids    the 1000 tables of `many`, 1024 ids each, q8 and bf16

    python scripts/tables_digest_grouped_cost.py [--out profiles/tables_digest_grouped.txt] [--min-ms 50]

The driver starts every (shape, kind) step as a process of its own under `timeout` and stops at the first that fails; a step first
checks the grouped records against the loop's, byte for byte (a wrong kernel is refused, not timed).  Within a step the legs
alternate: five rounds, in each one window per leg of as many back-to-back calls as fill --min-ms, closed by an event
synchronise; the median window is reported with the spread.  No threshold: the figures are recorded.  The kernels' register and
scratch use comes from a device-only compile of the two digest units.  Without a GPU the script fails: it never falls back."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recom_amd", "csrc")
sys.path.insert(0, ROOT)

STEPS = (("many", "q8"), ("many", "bf16"), ("one", "q8"), ("one", "bf16"), ("ids", "q8"), ("ids", "bf16"))
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


def step(args) -> dict:
    import torch
    from recom_amd import lib, synth, tables
    if not torch.cuda.is_available():
        raise SystemExit("NOT MEASURED: no GPU (there is no CPU fallback)")
    L = lib.load()
    dev = torch.device("cuda", 0)
    kind, shape = args.kind, args.shape
    dim, n_tables, table_rows, n_ids = (64, 1, 16_000_000, 0) if shape == "one" else (16, 1000, 16384, 1024 if shape == "ids" else 0)
    dtype = {"q8": torch.uint8, "bf16": torch.bfloat16}[kind]
    width = dim + (8 if kind == "q8" else 0)
    K = lib.TABLE_KINDS[kind]
    rb = tables.row_bytes(kind, dim)
    all_rows = n_tables * table_rows
    # the tables: views of one allocation of random bytes (a digest is about bytes)
    store = torch.randint(0, 256, (all_rows * rb,), dtype=torch.uint8, device=dev).view(dtype).view(all_rows, width)
    tabs = [store[k * table_rows:(k + 1) * table_rows] for k in range(n_tables)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    s = C.c_void_p(stream)
    words = C.sizeof(lib.TableDigest) // 8
    outs, twin_outs, one_out = (torch.zeros((n, words), dtype=torch.int64, device=dev) for n in (n_tables, n_tables, 1))
    workspace = torch.empty((int(L.fcp_tables_digest_workspace_bytes(n_tables)) // 8,), dtype=torch.int64, device=dev)
    single_ws = torch.empty((int(L.fcp_table_digest_workspace_bytes()) // 8,), dtype=torch.int64, device=dev)
    ids = [torch.randperm(table_rows, device=dev)[:n_ids].contiguous() for _ in range(n_tables)] if n_ids else None
    if ids is None:
        arr = (lib.TableDigestEntry * n_tables)(*[lib.TableDigestEntry(t.data_ptr(), None, table_rows, 0, 0, 1, K, dim, 0) for t in tabs])
        loop_args = [(p(t), K, table_rows, dim, 0, 1, C.c_void_p(twin_outs[k].data_ptr()), p(single_ws), 0, s) for k, t in enumerate(tabs)]
        loop_fn = L.fcp_table_digest
    else:
        arr = (lib.TableDigestEntry * n_tables)(*[lib.TableDigestEntry(t.data_ptr(), i.data_ptr(), table_rows, n_ids, 0, 1, K, dim, 0)
                                                  for t, i in zip(tabs, ids)])
        loop_args = [(p(t), K, table_rows, dim, 0, 1, p(i), n_ids, C.c_void_p(twin_outs[k].data_ptr()), p(single_ws), 0, s)
                     for k, (t, i) in enumerate(zip(tabs, ids))]
        loop_fn = L.fcp_table_digest_rows
    blocks = (C.c_int32 * n_tables)()
    launches = int(L.fcp_tables_digest_launches(arr, n_tables, blocks))

    def grouped(out=outs):
        lib.check(L.fcp_tables_digest(arr, n_tables, p(out), p(workspace), 0, s), "fcp_tables_digest")

    def loop():
        for a in loop_args:
            loop_fn(*a)

    def single():
        lib.check(L.fcp_table_digest(p(store), K, all_rows, dim, 0, 1, p(one_out), p(single_ws), 0, s), "fcp_table_digest")
    grouped()
    loop()
    single()
    torch.cuda.synchronize()
    if not torch.equal(outs, twin_outs) or not bool((outs[:, 0] != 0).all()):
        raise SystemExit(f"{shape} {kind}: the grouped call and the loop disagree; nothing timed")
    if ids is None:
        # rows at their global index: the entries' sums add up to the one table's
        arr0 = (lib.TableDigestEntry * n_tables)(*[lib.TableDigestEntry(t.data_ptr(), None, table_rows, 0, k * table_rows, 1, K, dim, 0)
                                                   for k, t in enumerate(tabs)])
        lib.check(L.fcp_tables_digest(arr0, n_tables, p(twin_outs), p(workspace), 0, s), "fcp_tables_digest")
        torch.cuda.synchronize()
        if int(twin_outs[:, 0].sum().item()) != int(one_out[0, 0].item()):
            raise SystemExit(f"{shape} {kind}: the entries do not add up to the whole; nothing timed")
        legs = {"grouped": grouped, "loop": loop, "single": single} if n_tables > 1 else {"grouped": grouped, "single": single}
        need = all_rows * rb
    else:
        delta = synth.hash_table_torch(11, n_tables * n_ids, dim, dev)
        xs = [delta[k * n_ids:(k + 1) * n_ids] for k in range(n_tables)]
        rows_arr = (lib.TableRows * n_tables)(*[lib.TableRows(t.data_ptr(), i.data_ptr(), x.data_ptr(), table_rows, n_ids, K, dim)
                                                for t, i, x in zip(tabs, ids, xs)])
        rows_ws = torch.empty((int(L.fcp_tables_rows_workspace_bytes(n_tables)) // 8,), dtype=torch.int64, device=dev)
        after = torch.zeros_like(outs)
        digests = [0] * n_tables

        def update():
            lib.check(L.fcp_tables_update_rows(rows_arr, n_tables, None, p(rows_ws), 0, s), "fcp_tables_update_rows")

        def tracked():
            grouped(outs)
            update()
            grouped(after)
        legs = {"grouped": grouped, "loop": loop, "update": update, "tracked": tracked,
                "tracked (py)": lambda: tables.update_rows_grouped_tracked(tabs, ids, xs, digests)}
        need = n_tables * n_ids * (8 + rb)
    timed = alternate(torch, legs, args.min_ms)
    return {"shape": shape, "kind": kind, "entries": n_tables, "rows": all_rows if ids is None else n_tables * n_ids, "dim": dim,
            "launches": launches, "blocks": int(sum(blocks)), "device": torch.cuda.get_device_name(0),
            "legs": {name: {"us_per_call": ms * 1e3, "spread_us": spread * 1e3, "host_us_per_call": host, "calls_per_window": calls,
                            "gbps": need / ms / 1e6} for name, (ms, spread, host, calls) in timed.items()}}


def resources() -> list:
    """per (G, by-id) — A plays no part in the figures' spread — the VGPRs of the grouped kernel beside its single-table twin's and
    the scratch of both, from a device-only compile"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit in ("fcp_tables_digest", "fcp_table_digest"):
            asm = os.path.join(tmp, unit + ".s")
            subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "--offload-device-only", "-S", os.path.join(CSRC, unit + ".hip"),
                            "-o", asm], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(asm).read(), re.S):
                field = lambda name: int(re.search(r"\.amdhsa_" + name + r" (\d+)", m.group(2)).group(1))   # noqa: E731
                found[m.group(1)] = (field("next_free_vgpr"), field("private_segment_fixed_size"), field("group_segment_fixed_size"))
    lines = [f"{'A':>3} {'G':>3} {'by id':>5} {'vgpr grouped':>12} {'vgpr single':>11} {'scratch':>7} {'lds':>4}"]
    for name, (vgpr, scratch, lds) in sorted(found.items()):
        m = re.search(r"fcp_tables_digest_kernelILi(\d+)ELi(\d+)ELb([01])EEE", name)
        if not m:
            continue
        (twin,) = [k for k in found if f"fcp_table_digest_kernelILi{m.group(1)}ELi{m.group(2)}ELb{m.group(3)}EEE" in k]
        lines.append(f"{m.group(1):>3} {m.group(2):>3} {m.group(3):>5} {vgpr:>12} {found[twin][0]:>11} {max(scratch, found[twin][1]):>7} {lds:>4}")
    (fold,) = [k for k in found if "fcp_tables_digest_fold_kernel" in k]
    lines.append(f"fold kernel: {found[fold][0]} VGPRs, scratch {found[fold][1]}, LDS {found[fold][2]}")
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables_digest_grouped.txt"))
    ap.add_argument("--min-ms", type=float, default=50.0, help="least length of a timed window")
    ap.add_argument("--shape", choices=("many", "one", "ids"), help="(one step, as the driver starts it)")
    ap.add_argument("--kind", choices=("q8", "bf16"))
    ap.add_argument("--note", default="", help="a paragraph appended to the profile")
    args = ap.parse_args()
    if args.shape:
        print("RECORD " + json.dumps(step(args)), flush=True)
        return
    records = []
    for shape, kind in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--shape", shape, "--kind", kind,
               "--min-ms", str(args.min_ms)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if proc.returncode != 0:                          # a failure, a fault, a time limit: nothing more is started
            raise SystemExit(f"step {shape} {kind} ended with status {proc.returncode}; stopped")
        records.append(json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:]))
        print(f"{shape} {kind}: done", flush=True)
    lines = [f"A model's tables digested in one call: fcp_tables_digest against one single-table call per entry ({records[0]['device']})",
             "grouped / loop: through the C ABI, arguments made once; single: one fcp_table_digest of the same bytes as one table; update:",
             "fcp_tables_update_rows alone; tracked: digest by id, update, digest by id, three calls; (py): tables.update_rows_grouped_tracked.",
             "many: 1000 x 16 384 rows of dim 16; one: 1 x 16 M rows of dim 64; ids: the tables of `many`, 1024 ids each.  launches / blocks:",
             "what one grouped digest enqueues, the record upload and the fold included, and the blocks the deal gave its entries.",
             f"us per call: median of {ROUNDS} alternating windows between two events (spread = max - min); host us: perf_counter around",
             "the enqueue, per call; GB/s = table bytes read (ids: ids + the rows they name) / time",
             f"{'shape':>5} {'kind':>5} {'launches':>8} {'blocks':>6} {'leg':>13} {'us/call':>10} {'spread':>8} {'host us':>9} {'GB/s':>7} {'vs grouped':>10} calls"]
    for r in records:
        for name, leg in r["legs"].items():
            lines.append(f"{r['shape']:>5} {r['kind']:>5} {r['launches']:>8} {r['blocks']:>6} {name:>13} {leg['us_per_call']:>10.1f} {leg['spread_us']:>8.1f} "
                         f"{leg['host_us_per_call']:>9.1f} {leg['gbps']:>7.0f} {leg['us_per_call'] / r['legs']['grouped']['us_per_call']:>10.2f} "
                         f"{leg['calls_per_window']}")
    lines += ["", "Compiler's resource usage (gfx950, -O3): every grouped kernel beside its single-table twin"] + resources()
    if args.note:
        lines += ["", args.note]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    print(json.dumps({"records": records}), flush=True)


if __name__ == "__main__":
    main()
