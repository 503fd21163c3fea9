"""What fcp_outputs_compare costs: S2's shape (1000 columns, dims 8 / 16 / 32 / 64, batch 512: two arenas of 61 MB) served by the
float32 plan into one arena and by the plan with table kinds by dim (8 -> f32, 16 -> bf16, 32 -> f16, 64 -> q8, as in
scripts/tables_mixed_cost.py) into another, then compared.  Four times per call, each by HIP events over at least 200 calls
after a warm-up, the legs alternating round after round, each leg as Python issues it back to back and once more behind a backlog
of copies that keeps the device's queue full (the device's own time: the Python wrappers need longer to enqueue a call):

    compare    ops.compare_outputs_async of the two results (upload, compare, fold, total: four launches)
    request    the float32 request itself
    copy       a device-to-device copy of one arena — both arenas are read once by the compare, so this is its natural floor
    torch      the composition the entry replaces: per column a slice of each side, sub, square().sum(), abs().max(), isfinite
               (no host read: the per-column results stay on the device)

and the compare once more with both arenas as bf16 (the narrow-output twins of the float32 plan).  The compare's time does not
depend on the tables' size; the request's does, so --vocab is recorded with it.  No threshold: what comes out is written to
profiles/outputs_compare.txt (--out).  The records of the timed pair are checked against the torch composition first.

    python scripts/outputs_compare_cost.py [--vocab 100000] [--calls 200] [--rounds 5] [--timeout 600] [--out FILE]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIXED_BY_DIM = {8: "f32", 16: "bf16", 32: "f16", 64: "q8"}


def torch_composition(torch, a, b, exact: bool = False):
    """per column: (sum of e^2, max |e|, non-finite pairs) as device tensors — thousands of launches, no host read.  `exact`:
    the squares in float64, as the entry forms them (the check; the timed form squares in float32)"""
    out = []
    for k in range(len(a.output_ptrs)):
        x, y = a.column(k).float(), b.column(k).float()
        e = y - x
        sq = e.double().square().sum() if exact else e.square().sum()
        out.append((sq, e.abs().max(), (~(torch.isfinite(x) & torch.isfinite(y))).sum()))
    return out


def child(vocab: int, calls: int, rounds: int, out_path: str, with_torch: bool = True) -> None:
    import numpy as np
    import torch
    from recom_amd import ops, synth, tables
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    m32 = synth.model_s2(vocab=vocab)
    mix = synth.model_s2(vocab=vocab, table_dtypes=MIXED_BY_DIM)      # (its spec; the tables are the float32 model's, converted)
    req = m32.make_request(1)
    blob, offsets, shapes = ops.concat_inputs(req.inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    tabs32 = m32.torch_tables(dev)
    plans = {"f32": (ops.FeatureColumnProcess(m32.spec, 0), tabs32),
             "mixed": (ops.FeatureColumnProcess(mix.spec, 0),
                       [t if MIXED_BY_DIM[t.shape[1]] == "f32" else tables.convert(t, MIXED_BY_DIM[t.shape[1]]) for t in tabs32]),
             "out_bf16": (ops.FeatureColumnProcess(m32.spec.with_out_dtype("bf16"), 0), tabs32)}
    nbytes = plans["f32"][0].plan.arena_bytes(shapes)
    arenas = {k: torch.empty(nbytes, dtype=torch.uint8, device=dev) for k in ("a", "b", "c", "d", "copy")}

    def serve(which, arena):
        op, tabs = plans[which]
        return op(d_blob, offsets, shapes, tabs, req.symbols, arena=arenas[arena])

    a, b = serve("f32", "a"), serve("mixed", "b")
    na, nb = serve("out_bf16", "c"), serve("out_bf16", "d")
    torch.cuda.synchronize()
    # the timed pair is right before it is timed
    got = ops.compare_outputs(a, b)
    ref = torch_composition(torch, a, b, exact=True)
    sse = np.asarray([float(r[0]) for r in ref])
    assert np.allclose(got.columns.sum_sq_err, sse, rtol=1e-9, atol=0.0), "sum_sq_err disagrees with torch"
    assert np.array_equal(got.columns.max_abs_err, np.asarray([float(r[1]) for r in ref], np.float32)), "max_abs_err disagrees with torch"
    assert int(got.total.nonfinite) == sum(int(r[2]) for r in ref)
    assert ops.compare_outputs(na, nb).identical and not got.identical
    legs = {
        "compare": lambda: ops.compare_outputs_async(a, b, stream),
        "compare_bf16": lambda: ops.compare_outputs_async(na, nb, stream),
        "request": lambda: serve("f32", "a"),
        "copy": lambda: arenas["copy"].copy_(arenas["a"]),
        "torch": lambda: torch_composition(torch, a, b),
    }
    if not with_torch:       # (a kernel trace: the composition alone would be 140 000 records)
        del legs["torch"]
    n_calls = {k: (max(calls, 200) if k != "torch" else 20) for k in legs}    # (the composition: ~7000 launches per call)
    for k, f in legs.items():
        for _ in range(20 if k != "torch" else 2):
            f()
    torch.cuda.synchronize()
    # Two times per leg.  "back to back": the calls as Python issues them, between two events — where the host needs longer to
    # enqueue a call than the device to run it, this is the host's time.  "queue kept full": the same calls behind a backlog of
    # arena copies long enough that every call is enqueued before the device reaches the first — the device's own time.
    us = {k: [] for k in legs}
    host_us = {k: [] for k in legs}
    full_us = {k: [] for k in legs if k != "torch"}      # (the composition is thousands of launches: the host's pace is its pace)

    def timed(f, n, backlog=0):
        for _ in range(backlog):
            legs["copy"]()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        h0 = time.perf_counter()
        for _ in range(n):
            f()
        h1 = time.perf_counter()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n, (h1 - h0) * 1e6 / n

    copy_us = timed(legs["copy"], 200)[0]
    for rnd in range(rounds):
        for k, f in legs.items():
            d, h = timed(f, n_calls[k])
            us[k].append(d)
            host_us[k].append(h)
            line = f"round {rnd} {k}: {d:.2f} us per call back to back, {h:.2f} us to enqueue"
            if k in full_us:
                backlog = int(1.5 * n_calls[k] * h / copy_us) + 100
                full_us[k].append(timed(f, n_calls[k], backlog)[0])
                line += f", {full_us[k][-1]:.2f} us with the queue kept full ({backlog} copies in front)"
            print(line, flush=True)
    med = {k: statistics.median(v) for k, v in us.items()}
    hmed = {k: statistics.median(v) for k, v in host_us.items()}
    fmed = {k: statistics.median(v) for k, v in full_us.items()}
    arena_mb = nbytes / 1e6
    lines = [
        f"fcp_outputs_compare on S2's shape: {len(a.output_ptrs)} columns, batch {m32.batch}, arena {arena_mb:.1f} MB per side (float32), vocab {vocab}",
        f"HIP events, {n_calls['compare']} calls per round ({n_calls.get('torch', 0)} for the torch composition), {rounds} rounds alternating, after warm-up; us per call, median [min .. max]",
        "",
    ]
    names = {"compare": "compare, float32 arena against float32 arena (tables f32 | kinds by dim)", "compare_bf16": "compare, both arenas bf16",
             "request": "the float32 request itself", "copy": "device-to-device copy of one float32 arena",
             "torch": "torch composition (slices, sub, square().sum(), abs().max(), isfinite)"}
    lines.append(f"  {'':<80s} {'back to back':>14s} {'host enqueue':>14s} {'queue kept full':>16s}")
    for k in [k for k in ("compare", "compare_bf16", "request", "copy", "torch") if k in legs]:
        full = f"{fmed[k]:10.2f}  [{min(full_us[k]):.2f} .. {max(full_us[k]):.2f}]" if k in fmed else "        -"
        lines.append(f"  {names[k]:<80s} {med[k]:14.2f} {hmed[k]:14.2f}   {full}")
    read_gbs = 2 * nbytes / (fmed["compare"] * 1e-6) / 1e9
    lines += ["",
              "device times (queue kept full):",
              f"compare / copy = {fmed['compare'] / fmed['copy']:.2f}   (the copy reads one arena and writes one; the compare reads two)",
              f"compare / request = {fmed['compare'] / fmed['request']:.2f}   compare bf16 / compare = {fmed['compare_bf16'] / fmed['compare']:.2f}",
              f"compare reads {2 * arena_mb:.0f} MB per call: {read_gbs:.0f} GB/s",
              f"as Python issues them: torch composition / compare = {med['torch'] / med['compare']:.0f}" if with_torch else "",
              f"records of the timed pair: differ {int(got.total.differ)} of {int(got.total.elems)} pairs, rel rms {got.rel_rms():.3e}, "
              f"max |e| {float(got.total.max_abs_err):.3e}, non-finite {int(got.total.nonfinite)}"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    print(json.dumps({"back_to_back_us": us, "host_enqueue_us": host_us, "queue_full_us": full_us, "arena_bytes": nbytes, "vocab": vocab}), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=100_000, help="rows per table (S2 itself: 1 000 000, 120 + 50 GB of tables)")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600, help="seconds the child may take, table fill included")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outputs_compare.txt"))
    ap.add_argument("--no-torch", action="store_true", help="leave the torch composition out (for a kernel trace)")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        child(args.vocab, args.calls, args.rounds, args.out, not args.no_torch)
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--vocab", str(args.vocab),
           "--calls", str(args.calls), "--rounds", str(args.rounds), "--out", args.out] + (["--no-torch"] if args.no_torch else [])
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
