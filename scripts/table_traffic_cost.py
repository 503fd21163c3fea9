"""What counting traffic and weighing the audit by it cost (profiles/table_traffic.txt).

(a) fcp_table_count_ids of `--ids` ids (2^24) into a count array of `--rows` rows (2^24), for uniform, Zipf (synth's rule:
    numpy's Zipf(1.05) folded into the table) and all-equal ids, int64 and int32, against
      torch      counts.index_add_(0, ids, ones), the composition it replaces;
      NAME       every `--variant NAME=LIBRARY` given: another build of the kernel unit that exports fcp_table_count_ids with
                 the same signature (how the kernel's shape was chosen: a scratch build with one global atomic per id and
                 nothing else).  Each variant's counts are compared with np.bincount once, like the library's.
(b) fcp_table_audit_weighted of a `--rows` x 64 float32 table under the Zipf counts, against fcp_table_audit of the same table;
    with `--other-lib LIBRARY` (another build of libfcp_hip.so, the parent commit's for instance) that build's fcp_table_audit
    is timed in alternation with this one's, `--rounds` times each, so the spread of either shows.
Every figure is the median (min, max) of `--reps` warm HIP-event timings in ONE process.  No threshold anywhere: the times are
recorded.

    python scripts/table_traffic_cost.py [--ids 16777216] [--rows 16777216] [--reps 20] [--rounds 3] [--timeout 900]
                                         [--variant NAME=LIBRARY ...] [--other-lib LIBRARY]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps: int):
    """median and spread, in ms, of `reps` warm runs of fn between two events on the current stream"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def draw(dist: str, n: int, rows: int) -> np.ndarray:
    rng = np.random.default_rng(11)
    if dist == "uniform":
        return rng.integers(0, rows, n, dtype=np.int64)
    if dist == "zipf":
        return ((rng.zipf(1.05, size=n).astype(np.int64) - 1) % rows).astype(np.int64)
    return np.full(n, rows // 3, np.int64)


def child(n: int, rows: int, reps: int, rounds: int, variants, other_lib) -> None:
    import torch
    from recom_amd import lib as _lib
    from recom_amd import synth, tables
    dev = torch.device("cuda", 0)
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    counters = [("count_ids", L.fcp_table_count_ids)]
    for name, path in variants:
        fn = C.CDLL(path).fcp_table_count_ids
        fn.argtypes = argtypes
        counters.append((name, fn))
    results = {"ids": n, "rows": rows, "count": [], "audit": []}
    counts = torch.zeros((rows,), dtype=torch.int32, device=dev)
    ones = torch.ones((n,), dtype=torch.int32, device=dev)
    zipf_counts = None
    for dist in ("uniform", "zipf", "equal"):
        host = draw(dist, n, rows)
        want = np.bincount(host, minlength=rows).astype(np.uint32)
        print(f"{dist}: {n} ids, {int((want > 0).sum())} distinct rows, the hottest read {int(want.max())} times", flush=True)
        for dtype, tname in ((torch.int64, "int64"), (torch.int32, "int32")):
            ids = torch.from_numpy(host).to(dev).to(dtype)
            legs = {}
            for name, fn in counters:
                def call(fn=fn):
                    _lib.check(fn(C.c_void_p(counts.data_ptr()), rows, C.c_void_p(ids.data_ptr()), ids.element_size(), n, None, 0,
                                  C.c_void_p(stream)), name)
                counts.zero_()
                call()
                torch.cuda.synchronize()
                assert np.array_equal(counts.cpu().numpy().view(np.uint32), want), f"{name} miscounts {dist} {tname} ids"
                legs[name] = timed(torch, call, reps)
            legs["torch"] = timed(torch, lambda: counts.index_add_(0, ids, ones), max(3, reps // 4))
            for name, (med, lo, hi) in legs.items():
                print(f"{dist:8s} {tname}  {name:12s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f})  {n / (med * 1e-3) / 1e9:8.2f} G ids/s", flush=True)
            results["count"].append({"dist": dist, "ids": tname, **{k: {"median_ms": v[0], "min_ms": v[1], "max_ms": v[2]} for k, v in legs.items()}})
            if dist == "zipf" and zipf_counts is None:
                zipf_counts = torch.from_numpy(want.view(np.int32)).to(dev)
            del ids
    del ones, counts

    # (b) the audit, unweighted and weighted, of rows x 64
    dim = 64
    t = synth.hash_table_torch(7, rows, dim, dev)
    out = torch.empty(((C.sizeof(_lib.TableAudit) + 7) // 8,), dtype=torch.int64, device=dev)
    ws = torch.empty((L.fcp_table_audit_workspace_bytes() // 8,), dtype=torch.int64, device=dev)

    def audit_of(lib):
        return lambda: _lib.check(lib.fcp_table_audit(C.c_void_p(t.data_ptr()), rows, dim, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 0,
                                                      C.c_void_p(stream)), "fcp_table_audit")

    def weighted():
        _lib.check(L.fcp_table_audit_weighted(C.c_void_p(t.data_ptr()), rows, dim, C.c_void_p(zipf_counts.data_ptr()), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(ws.data_ptr()), 0, C.c_void_p(stream)), "fcp_table_audit_weighted")

    legs = [("audit", audit_of(L))]
    if other_lib:
        O = C.CDLL(other_lib)
        O.fcp_table_audit.argtypes = L.fcp_table_audit.argtypes
        legs.append(("audit, other build", audit_of(O)))
    legs.append(("weighted", weighted))
    gb = t.numel() * 4 / 1e9
    for r in range(rounds):
        for name, fn in legs:
            med, lo, hi = timed(torch, fn, reps)
            print(f"{rows} x {dim}  round {r}  {name:19s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f})  {gb / (med * 1e-3):8.1f} GB/s of float32 read", flush=True)
            results["audit"].append({"round": r, "leg": name, "median_ms": med, "min_ms": lo, "max_ms": hi})
    plain, w = tables.audit(t), tables.audit(t, row_counts=zipf_counts)
    for name, a in (("unweighted", plain), ("zipf-weighted", w)):
        print(f"{rows} x {dim}  {name}: " + ", ".join(f"{k} rel. sq. err {a.kinds[k].sum_sq_err / a.sum_sq:.3e}" for k in ("bf16", "f16", "q8")), flush=True)
    print(json.dumps(results), flush=True)
    torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=1 << 24)
    ap.add_argument("--rows", type=int, default=1 << 24, help="rows of the count array and of the dim-64 table")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the audit's legs")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIBRARY",
                    help="another build that exports fcp_table_count_ids, timed beside the library's")
    ap.add_argument("--other-lib", default="", help="another build of libfcp_hip.so whose fcp_table_audit is timed beside this one's")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    variants = [tuple(v.split("=", 1)) for v in args.variant]
    if args.child:
        child(args.ids, args.rows, args.reps, args.rounds, variants, args.other_lib)
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--ids", str(args.ids), "--rows", str(args.rows),
           "--reps", str(args.reps), "--rounds", str(args.rounds), "--other-lib", args.other_lib] + [f"--variant={n}={p}" for n, p in variants]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
