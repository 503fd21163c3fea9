"""What per-id weights cost: BASELINE configs[3] (RAGGED, 512 multi-hot columns, batch 256) in the CSR form with every
pooled column weighted against the same plan unweighted — one process, the two legs alternating, each warmed for at least
0.25 s and timed with HIP events over at least 2000 requests, five alternations.  Beside each leg its algorithmic bytes
(weighted: + 4 B per id).  Prints one line per leg and a JSON summary (medians, spreads).

    python scripts/weighted_bags_cost.py [--steps 2000] [--rounds 5]

(The kernel's own time: run this script under `rocprofv3 --kernel-trace --stats -- python scripts/weighted_bags_cost.py
--rounds 1` and read the average of fcp_weighted_bag_kernel / fcp_ragged_kernel.)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recom_amd import synth  # noqa: E402
from recom_amd.harness import ServingHarness  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup-s", type=float, default=0.25)
    args = ap.parse_args()
    legs = {}
    for name, weighted in (("unweighted", False), ("weighted", True)):
        h = ServingHarness(synth.model_ragged(seg="csr", weighted=weighted))
        h.run(16)
        legs[name] = h
        print(f"{name}: launch {h.plan.last_launch()}, algorithmic bytes per request {h.algorithmic_bytes()}", flush=True)
    us = {name: [] for name in legs}
    for rnd in range(args.rounds):
        for name, h in legs.items():
            t0 = time.time()
            while time.time() - t0 < args.warmup_s:
                h.run(200)
            _, dev_ms, _ = h.run(max(args.steps, 2000))
            us[name].append(dev_ms * 1e3 / max(args.steps, 2000))
            print(f"round {rnd} {name}: {us[name][-1]:.2f} us per request", flush=True)
    out = {}
    for name, h in legs.items():
        b = h.algorithmic_bytes()
        med = statistics.median(us[name])
        out[name] = {"us_per_request": us[name], "median_us": med, "spread_us": max(us[name]) - min(us[name]),
                     "algorithmic_bytes_per_request": b["total"], "algorithmic_tb_per_s": b["total"] / med / 1e6,
                     "kernel": h.plan.last_launch()["kernel"]}
    out["weighted_over_unweighted"] = {"time": out["weighted"]["median_us"] / out["unweighted"]["median_us"],
                                       "bytes": out["weighted"]["algorithmic_bytes_per_request"] /
                                       out["unweighted"]["algorithmic_bytes_per_request"]}
    print(json.dumps(out))
    for h in legs.values():
        h.close()


if __name__ == "__main__":
    main()
