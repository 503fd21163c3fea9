"""What counting a request's table traffic costs (profiles/plan_traffic.txt).

Per workload — S2 at batch 512 (1000 columns, every 10th bucketized), RAGGED (BASELINE configs[3]: 512 multi-hot columns,
SparseTensor indices, int64 ids) and RAGGED with bags of up to 300 Zipf-distributed ids — one resident request, and for it
  (a) fcp_plan_traffic_count: one launch — the library's kernel (a block counts in an LDS table first) and, for every
      `--variant NAME=LIBRARY`, another build's, called on the same plan object (how the kernel's shape was chosen: the
      variant on file was a build of the commit that introduced the kernel with the plainer kernel in it, one global atomic
      per counted id and no LDS table; `make -C recom_amd/csrc OUT=<dir>` at any commit gives such a library);
  (b) the composition it replaces: per lookup column the ids transformed in torch (torch.bucketize for the bucketized
      columns; the others carry row ids already) and one fcp_table_count_ids per column, called through ctypes with
      arguments built beforehand — its device code is the same in every build, so it is measured here, in the same run;
  (c) the request's own fcp_process_feature_columns into one reused arena, for scale (arguments built beforehand too).
Every leg is `--calls` back-to-back calls between two HIP events on one stream, ended by a synchronise, divided by the calls:
what a serving loop pays per request, host time included where the host is the slower side (leg (b) is a thousand launches).
The legs alternate `--rounds` times in ONE process; the median, minimum and maximum over the rounds are recorded.  Before any
timing the counts of (a), of every build, are compared with those of (b), cell by cell.  No threshold anywhere.

    python scripts/plan_traffic_cost.py [--workloads s2,ragged,ragged300] [--calls 50] [--rounds 5] [--timeout 900]
                                        [--variant NAME=LIBRARY ...] [--out profiles/plan_traffic.txt]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def build(workload: str):
    from recom_amd import synth
    if workload == "s2":
        return synth.model_s2(batch=512)
    if workload == "ragged":
        return synth.model_ragged(seg="indices")
    if workload == "ragged300":
        return synth.model_ragged(seg="indices", max_len=300, dist="zipf")
    raise SystemExit(f"unknown workload {workload!r}")


def loop_us(torch, fn, calls: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def measure(torch, workload: str, calls: int, rounds: int, variants, say) -> None:
    from recom_amd import lib as _lib
    from recom_amd import tables
    from recom_amd.ops import FeatureColumnProcess, concat_inputs
    from recom_amd.plan import IDS_F32_BUCKETIZE
    dev = torch.device("cuda", 0)
    L = _lib.load()
    m = build(workload)
    spec = m.spec
    op = FeatureColumnProcess(spec, 0)
    req = m.make_request(0)
    blob, offsets, shapes = concat_inputs(req.inputs)
    d_blob = torch.from_numpy(blob).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lookups = [c for c in spec.columns if c.form in (1, 2, 3)]
    n_ids = sum(int(np.asarray(req.inputs[c.ids_input]).size) for c in lookups)
    say(f"== {workload}: {m.description}; {len(lookups)} lookup columns, {n_ids} ids in the request, blob {blob.nbytes} bytes")

    # (a) one launch
    counts = tables.new_plan_counts(op.plan, dev)
    skipped = torch.zeros((1,), dtype=torch.int64, device=dev)
    op.traffic_bind(counts, skipped)
    sym = None if req.symbols is None else np.ascontiguousarray(req.symbols, np.int32)
    args = _lib.ProcessArgs(d_blob.data_ptr(), blob.nbytes, offsets.ctypes.data_as(C.POINTER(C.c_int32)), shapes.ctypes.data_as(C.POINTER(C.c_int32)),
                            None, None, None if sym is None else sym.ctypes.data_as(C.POINTER(C.c_int32)), stream)

    counters = [("the library (LDS table)", L.fcp_plan_traffic_count)]
    for name, path in variants:
        fn = C.CDLL(path).fcp_plan_traffic_count
        fn.argtypes = L.fcp_plan_traffic_count.argtypes
        counters.append((name, fn))

    def count_with(fn):
        return lambda: _lib.check(fn(op.plan.handle, C.byref(args)), "fcp_plan_traffic_count")

    # (b) per column: transform in torch, then fcp_table_count_ids
    by_hand = tables.new_plan_counts(op.plan, dev)
    skipped_b = torch.zeros((1,), dtype=torch.int64, device=dev)
    steps, keep = [], []          # (keep: the id tensors whose addresses the prepared calls hold)
    for c in lookups:
        if c.xform_mode or c.hash_buckets:
            raise SystemExit("the composition leg restates bucketize only; this workload hashes or filters")
        raw = torch.from_numpy(np.ascontiguousarray(req.inputs[c.ids_input]).reshape(-1)).to(dev)
        target = by_hand[c.table_input]
        if c.id_source == IDS_F32_BUCKETIZE:
            bnd = torch.from_numpy(np.ascontiguousarray(c.boundaries, np.float32)).to(dev)
            ids = torch.empty(raw.shape, dtype=torch.int64, device=dev)
            steps.append((lambda raw=raw, bnd=bnd, ids=ids: torch.bucketize(raw, bnd, right=True, out=ids)))
        else:
            ids = raw
        keep.append(ids)
        call = (C.c_void_p(target.data_ptr()), int(c.vocab), C.c_void_p(ids.data_ptr()), int(ids.element_size()), int(ids.numel()),
                C.c_void_p(skipped_b.data_ptr()), 0, C.c_void_p(stream))
        steps.append((lambda call=call: _lib.check(L.fcp_table_count_ids(*call), "fcp_table_count_ids")))

    def count_b():
        for s in steps:
            s()

    # (c) the request itself, into one arena
    tabs = m.torch_tables(dev)
    arena = torch.empty((op.plan.arena_bytes(shapes, sym),), dtype=torch.uint8, device=dev)

    pargs, keep_args = op._args(d_blob, offsets, shapes, tabs, sym, stream, arena)
    groups = (C.c_void_p * spec.n_groups)()
    group_shapes = (C.c_int32 * (2 * spec.n_groups))()
    result = _lib.ProcessResult(None, None, None, groups, group_shapes, None, 0)

    def process():
        _lib.check(L.fcp_process_feature_columns(op.plan.handle, C.byref(pargs), C.byref(result)), "fcp_process_feature_columns")

    # (a) of every build against (b), cell by cell, before anything is timed
    count_b()
    for name, fn in counters:
        for t in counts:
            if t is not None:
                t.zero_()
        skipped.zero_()
        count_with(fn)()
        torch.cuda.synchronize()
        for t, (x, y) in enumerate(zip(counts, by_hand)):
            assert (x is None and y is None) or np.array_equal(x.cpu().numpy(), y.cpu().numpy()), f"{name}: table {t} is miscounted"
        assert int(skipped.item()) == int(skipped_b.item()), name
    total = sum(int(x.cpu().numpy().view(np.uint32).astype(np.int64).sum()) for x in counts if x is not None)
    say(f"   counts of every build equal the composition's: {total} reads counted, {int(skipped.item())} ids outside their vocab")

    legs = [(f"(a) fcp_plan_traffic_count, {name}", count_with(fn), calls) for name, fn in counters]
    legs += [("(b) torch transform + fcp_table_count_ids per column", count_b, max(2, calls // 10)),
             ("(c) fcp_process_feature_columns", process, calls)]
    us = {name: [] for name, _, _ in legs}
    for name, fn, n in legs:          # warm every leg
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn, n in legs:
            us[name].append(loop_us(torch, fn, n))
    for name, _, n in legs:
        v = us[name]
        say(f"   {name:54s} median {statistics.median(v):10.2f} us per request  (min {min(v):.2f}, max {max(v):.2f}; {rounds} rounds of {n} calls)")
    op.traffic_bind(None)
    torch.cuda.synchronize()


def child(workloads, calls: int, rounds: int, variants, out: str, cmdline: str) -> None:
    import torch
    lines = []

    def say(s: str) -> None:
        print(s, flush=True)
        lines.append(s)

    say(f"$ {cmdline}")
    say(f"device: {torch.cuda.get_device_name(0)}; every figure: HIP events around back-to-back calls on one stream, per call")
    for w in workloads:
        measure(torch, w, calls, rounds, variants, say)
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="s2,ragged,ragged300")
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per timed loop (a tenth of it for leg (b))")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the legs")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIBRARY",
                    help="another build of libfcp_hip.so whose fcp_plan_traffic_count is timed beside the library's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_traffic.txt"))
    ap.add_argument("--timeout", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    variants = [tuple(v.split("=", 1)) for v in args.variant]
    if args.child:
        cmdline = "python scripts/plan_traffic_cost.py " + " ".join(f"--{k} {getattr(args, k)}" for k in ("workloads", "calls", "rounds"))
        cmdline += "".join(f" --variant {n}=<its build of libfcp_hip.so>" for n, _ in variants)
        child(args.workloads.split(","), args.calls, args.rounds, variants, args.out, cmdline)
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workloads", args.workloads,
           "--calls", str(args.calls), "--rounds", str(args.rounds), "--out", args.out] + [f"--variant={n}={p}" for n, p in variants]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
