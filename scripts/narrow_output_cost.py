"""What bf16 / fp16 output is worth: S2, RAGGED (CSR form) and the reference's model E, each as a float32 plan and as its
two narrow twins (PlanSpec.out_dtype) — one process, the three legs of a workload bound to the SAME tables and the same
resident requests, alternating, each warmed for at least 0.25 s and timed with HIP events over at least 2000 requests, five
alternations.  Beside each leg its launch report and algorithmic bytes (narrow: 2 B per written element).  Prints one line
per leg and round, and one JSON summary per workload (medians, spreads, narrow over float32).

    python scripts/narrow_output_cost.py [--workloads s2,ragged,e] [--steps 2000] [--rounds 5] [--arena-ring 1]

The float32 leg is the yardstick of the narrow legs; `bench.py --workload s2` of the parent commit, run the same way (one
arena, 2000 steps), is the yardstick of the float32 leg: the float32 kernels are instruction for instruction the parent's.

(The kernels' own time: run this script under `rocprofv3 --kernel-trace --stats -- python scripts/narrow_output_cost.py
--rounds 1` and read the averages of fcp_dense_kernel / fcp_dense_narrow_kernel, fcp_ragged_kernel /
fcp_ragged_narrow_kernel and fcp_hybrid_kernel / fcp_hybrid_narrow_kernel.)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recom_amd import synth  # noqa: E402
from recom_amd.harness import ServingHarness  # noqa: E402

LEGS = ("f32", "bf16", "f16")


def build(workload: str):
    if workload == "s2":
        return synth.model_s2(), 16
    if workload == "ragged":
        return synth.model_ragged(seg="csr"), 64
    if workload == "e":       # in the form the rewritten graph's ConcatInputs leaves in HBM, as bench.py times it
        return synth.staged_model(synth.model_ae("E")), 64
    raise SystemExit(f"unknown workload {workload}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="s2,ragged,e")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=0.25)
    ap.add_argument("--arena-ring", type=int, default=1, help="arenas per worker (bench.py's default: 1, the arena reused)")
    args = ap.parse_args()
    import torch
    steps = max(args.steps, 2000)
    for workload in args.workloads.split(","):
        model, n_requests = build(workload)
        tables = model.torch_tables(torch.device("cuda", 0))     # one set for the three legs (three S2 sets do not fit)
        legs = {}
        for name in LEGS:
            spec = model.spec if name == "f32" else model.spec.with_out_dtype(name)
            h = ServingHarness(model, n_requests=n_requests, arena_ring=args.arena_ring, tables=tables, spec=spec)
            check = h.verify_resident()                          # a wrong kernel is refused here, not timed
            h.run(16)
            legs[name] = h
            print(f"{workload} {name}: launch {h.plan.last_launch()}, algorithmic bytes per request {h.algorithmic_bytes()}, "
                  f"verified {check['checked']}", flush=True)
        us = {name: [] for name in legs}
        for rnd in range(args.rounds):
            for name, h in legs.items():
                t0 = time.time()
                while time.time() - t0 < args.warmup_s:
                    h.run(200)
                _, dev_ms, _ = h.run(steps)
                us[name].append(dev_ms * 1e3 / steps)
                print(f"{workload} round {rnd} {name}: {us[name][-1]:.2f} us per request", flush=True)
        out = {"workload": workload, "arena_ring": args.arena_ring, "steps": steps}
        for name, h in legs.items():
            b = h.algorithmic_bytes()
            med = statistics.median(us[name])
            launch = h.plan.last_launch()
            out[name] = {"us_per_request": us[name], "median_us": med, "spread_us": max(us[name]) - min(us[name]),
                         "algorithmic_bytes_per_request": b["total"], "out_bytes_per_request": b["out"],
                         "algorithmic_tb_per_s": b["total"] / med / 1e6, "kernel": launch["kernel"], "store": launch["store"]}
        for name in LEGS[1:]:
            out[f"{name}_over_f32"] = {"time": out[name]["median_us"] / out["f32"]["median_us"],
                                       "bytes": out[name]["algorithmic_bytes_per_request"] / out["f32"]["algorithmic_bytes_per_request"]}
        print(json.dumps(out), flush=True)
        for h in legs.values():
            h.close()
        del legs, tables
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
