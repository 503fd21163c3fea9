"""What 8-bit row-quantised tables cost in time: S2 and S2-Zipf at batch 512, the q8 plan (PlanSpec.table_dtype "q8") against
the float32 plan on the DEQUANTISED values of the same tables — the float32 leg is the yardstick — through the native
harness.  No threshold: the figures are recorded (profiles/tables_q8_ab.txt).

    python scripts/tables_q8_cost.py [--workloads s2,s2_zipf] [--steps 2000] [--rounds 5] [--leg-timeout 420]

The driver starts one child process per leg and round, ALTERNATING the two legs, each child under its own `timeout`; the
driver itself never opens the GPU.  A child builds its leg's tables (38 GB of q8 rows; 120 GB of float32, dequantised from
them one table at a time: both never have to be resident at once), checks every resident request against the closed-form
table contents (synth.q8_rows, dequantised: a wrong kernel is refused, not timed), warms up for at least 0.25 s and times
at least 2000 requests with HIP events.  A leg that fails, or that runs into its time limit, ends the measurement: nothing
more is started.  One line per leg and round, and one JSON summary per workload (medians, spreads, q8 over float32)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("f32", "q8")


def build(workload: str, table_dtype: str):
    from recom_amd import synth
    if workload == "s2":
        return synth.model_s2(table_dtype=table_dtype)
    if workload == "s2_zipf":
        return synth.model_s2(dist="zipf", table_dtype=table_dtype)
    raise SystemExit(f"unknown workload {workload}")


def leg(workload: str, table_dtype: str, steps: int, warmup_s: float, arena_ring: int) -> None:
    """One leg in this process: prints one JSON line."""
    import torch
    from recom_amd.harness import ServingHarness
    from recom_amd import synth
    model = build(workload, table_dtype)
    if table_dtype == "q8":
        h = ServingHarness(model, n_requests=16, arena_ring=arena_ring)
    else:       # the float32 plan on the dequantised values of the q8 tables
        dev = torch.device("cuda", 0)
        tables = [synth.dequantize_q8_torch(synth.q8_table_torch(t.seed, t.vocab, t.dim, dev)) for t in model.tables]
        h = ServingHarness(model, n_requests=16, arena_ring=arena_ring, tables=tables,
                           expected_rows=lambda seed, rows, dim: synth.dequantize_q8(synth.q8_rows(seed, rows, dim)))
    check = h.verify_resident()
    h.run(16)
    t0 = time.time()
    while time.time() - t0 < warmup_s:
        h.run(200)
    _, dev_ms, _ = h.run(steps)
    b = h.algorithmic_bytes()
    launch = h.plan.last_launch()
    print(json.dumps({"workload": workload, "leg": table_dtype, "us_per_request": dev_ms * 1e3 / steps, "steps": steps,
                      "kernel": launch["kernel"], "store": launch["store"], "verified": check["checked"],
                      "table_gb": model.table_bytes() / 1e9, "algorithmic_bytes_per_request": b["total"],
                      "row_bytes_per_request": b["rows"]}), flush=True)
    h.close()
    torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="s2,s2_zipf")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=0.25)
    ap.add_argument("--arena-ring", type=int, default=1, help="arenas per worker (bench.py's default: 1, the arena reused)")
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a leg may take, table fill included")
    ap.add_argument("--leg", default=None, help="(internal) run this one leg in this process: WORKLOAD:DTYPE")
    args = ap.parse_args()
    steps = max(args.steps, 2000)
    if args.leg:
        workload, dt = args.leg.split(":")
        leg(workload, dt, steps, args.warmup_s, args.arena_ring)
        return
    for workload in args.workloads.split(","):
        us = {name: [] for name in LEGS}
        last = {}
        for rnd in range(args.rounds):
            for name in LEGS:
                cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", f"{workload}:{name}",
                       "--steps", str(steps), "--warmup-s", str(args.warmup_s), "--arena-ring", str(args.arena_ring)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:           # a failed or timed-out leg ends the measurement: nothing more is started
                    print(r.stdout[-2000:], r.stderr[-4000:], sep="\n", flush=True)
                    raise SystemExit(f"{workload} round {rnd} {name}: exit status {r.returncode}; stopping")
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                us[name].append(rec["us_per_request"])
                last[name] = rec
                print(f"{workload} round {rnd} {name}: {rec['us_per_request']:.2f} us per request "
                      f"({rec['kernel']}, {rec['table_gb']:.0f} GB of tables, verified {rec['verified']})", flush=True)
        out = {"workload": workload, "arena_ring": args.arena_ring, "steps": steps}
        for name in LEGS:
            med = statistics.median(us[name])
            out[name] = {"us_per_request": us[name], "median_us": med, "spread_us": max(us[name]) - min(us[name]),
                         "kernel": last[name]["kernel"], "table_gb": last[name]["table_gb"],
                         "algorithmic_bytes_per_request": last[name]["algorithmic_bytes_per_request"]}
        out["q8_over_f32"] = {"time": out["q8"]["median_us"] / out["f32"]["median_us"],
                              "bytes": out["q8"]["algorithmic_bytes_per_request"] / out["f32"]["algorithmic_bytes_per_request"]}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
