"""What per-input table formats cost in time: S2 at full size (1000 columns x 1 M rows, batch 512) through the native harness,
four legs — float32 tables, plan-wide bf16, plan-wide q8, and MIXED by dim (8 -> f32, 16 -> bf16, 32 -> f16, 64 -> q8:
PlanSpec.table_dtypes, the kernels of fcp_tables_mixed.hip).  No threshold on the mixed leg: its time is recorded
(profiles/tables_mixed_ab.txt).  The plan-wide legs are the yardstick of "nothing else moved": their kernels are
byte-identical to the parent commit's, so the same script run from a checkout of the parent commit (--legs f32,bf16,q8: it
uses nothing that commit lacks for those legs) in the same GPU visit must agree with them within the spread of the parent's
own repeated legs.

    python scripts/tables_mixed_cost.py [--legs f32,bf16,q8,mixed] [--steps 2000] [--rounds 5] [--timeout 900]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself.  The child builds every leg's
tables once (120 + 60 + 38 + 50 GB: they are resident together), checks every resident request of every leg against the
closed-form table contents (a wrong kernel is refused, not timed), warms every leg up and then times the legs ALTERNATING,
round after round, at least 2000 requests per leg and round, with HIP events.  One line per leg and round and one JSON
summary."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("f32", "bf16", "q8", "mixed")
MIXED_BY_DIM = {8: "f32", 16: "bf16", 32: "f16", 64: "q8"}


def build(leg: str, columns: int, vocab: int):
    from recom_amd import synth
    if leg == "mixed":
        return synth.model_s2(columns=columns, vocab=vocab, table_dtypes=MIXED_BY_DIM)
    return synth.model_s2(columns=columns, vocab=vocab, table_dtype=leg)


def mixed_rows(seed, rows, dim):
    """the closed form of what a table of the mixed leg holds, by its width"""
    from recom_amd import synth
    kind = MIXED_BY_DIM[dim]
    if kind == "q8":
        return synth.dequantize_q8(synth.q8_rows(seed, rows, dim))
    return synth.round_to_table(synth.hash_rows(seed, rows, dim), kind)


def child(legs, steps: int, rounds: int, warmup_s: float, arena_ring: int, columns: int, vocab: int) -> None:
    import torch
    from recom_amd.harness import ServingHarness
    dev = torch.device("cuda", 0)
    hs = {}
    for leg in legs:
        model = build(leg, columns, vocab)
        if leg == "mixed":
            h = ServingHarness(model, n_requests=16, arena_ring=arena_ring, tables=model.torch_tables(dev), expected_rows=mixed_rows)
        else:
            h = ServingHarness(model, n_requests=16, arena_ring=arena_ring)
        check = h.verify_resident()
        h.run(16)
        hs[leg] = (model, h, check["checked"])
        print(f"{leg}: {model.table_bytes() / 1e9:.0f} GB of tables resident, verified {check['checked']}", flush=True)
    for leg in legs:
        t0 = time.time()
        while time.time() - t0 < warmup_s:
            hs[leg][1].run(200)
    us = {leg: [] for leg in legs}
    for rnd in range(rounds):
        for leg in legs:
            _, dev_ms, _ = hs[leg][1].run(steps)
            us[leg].append(dev_ms * 1e3 / steps)
            print(f"round {rnd} {leg}: {us[leg][-1]:.2f} us per request", flush=True)
    out = {"workload": "s2", "columns": columns, "vocab": vocab, "steps": steps, "arena_ring": arena_ring}
    for leg in legs:
        model, h, checked = hs[leg]
        launch = h.plan.last_launch()
        out[leg] = {"us_per_request": us[leg], "median_us": statistics.median(us[leg]), "spread_us": max(us[leg]) - min(us[leg]),
                    "kernel": launch["kernel"], "table_gb": model.table_bytes() / 1e9, "verified": checked,
                    "algorithmic_bytes_per_request": h.algorithmic_bytes()["total"]}
    if "f32" in legs:
        for leg in legs:
            out[leg]["time_over_f32"] = out[leg]["median_us"] / out["f32"]["median_us"]
    print(json.dumps(out), flush=True)
    for _, h, _ in hs.values():
        h.close()
    torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=0.25)
    ap.add_argument("--arena-ring", type=int, default=1, help="arenas per worker (bench.py's default: 1, the arena reused)")
    ap.add_argument("--columns", type=int, default=1000)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--timeout", type=int, default=900, help="seconds the child may take, table fill included")
    ap.add_argument("--child", action="store_true", help="(internal) run the legs in this process")
    args = ap.parse_args()
    legs = [leg for leg in args.legs.split(",") if leg]
    if any(leg not in LEGS for leg in legs):
        raise SystemExit(f"legs are {LEGS}")
    if args.child:
        child(legs, max(args.steps, 2000), args.rounds, args.warmup_s, args.arena_ring, args.columns, args.vocab)
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--legs", ",".join(legs),
           "--steps", str(args.steps), "--rounds", str(args.rounds), "--warmup-s", str(args.warmup_s), "--arena-ring", str(args.arena_ring),
           "--columns", str(args.columns), "--vocab", str(args.vocab)]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
