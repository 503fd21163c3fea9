"""What the table audit costs, and what the chooser picks for S2 (profiles/table_audit.txt).

Per table shape — 16 M x 64, and S2's own tables, 1 M rows of dim 8 / 16 / 32 / 64 — the median of warm HIP-event timings of
  audit     fcp_table_audit (the audit kernel and its fold), result and workspace allocated once;
  quantise  fcp_table_convert float32 -> q8 of the same table in the same process: it reads the same bytes and writes a quarter;
  copy      a device-to-device copy of the table (reads and writes 4 bytes an element);
  torch     the composition the audit replaces: per format tables.convert there and back, torch reductions for the non-finite
            rows, the rows a format cannot hold, the error's sum of squares and its maximum.
Then the chooser on S2 (1000 tables, closed-form contents): every table audited, formats chosen at a few budgets between the
all-q8 and the all-float32 totals.  No threshold anywhere: the times are recorded.

    python scripts/table_audit_cost.py [--rows 16777216] [--reps 20] [--vocab 1000000] [--timeout 900]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

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


def torch_composition(torch, tables, t):
    """the audit composed from convert twice and torch reductions: the same fields, per format"""
    finite = torch.isfinite(t).all(dim=1)
    out = {"rows_nonfinite": (~finite).sum(), "sum_sq": (t[finite].double() ** 2).sum()}
    for kind in ("bf16", "f16", "q8"):
        back = tables.convert(tables.convert(t, kind), "f32")
        if kind == "q8":
            bad = finite & ~torch.isfinite(t.max(dim=1).values - t.min(dim=1).values)
        else:
            bad = finite & torch.isinf(back).any(dim=1)
        e = torch.where((finite & ~bad)[:, None], t - back, torch.zeros((), device=t.device))
        out[kind] = (bad.sum(), (e.double() ** 2).sum(), e.abs().max())
    return out


def child(rows: int, reps: int, vocab: int) -> None:
    import torch
    from recom_amd import lib as _lib
    from recom_amd import synth, tables
    dev = torch.device("cuda", 0)
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty(((C.sizeof(_lib.TableAudit) + 7) // 8,), dtype=torch.int64, device=dev)
    ws = torch.empty((L.fcp_table_audit_workspace_bytes() // 8,), dtype=torch.int64, device=dev)
    results = []
    for n_rows, dim in ((rows, 64), (1_000_000, 8), (1_000_000, 16), (1_000_000, 32), (1_000_000, 64)):
        t = synth.hash_table_torch(7, n_rows, dim, dev)
        q8 = torch.empty((n_rows, dim + 8), dtype=torch.uint8, device=dev)
        twin = torch.empty_like(t)

        def audit():
            _lib.check(L.fcp_table_audit(C.c_void_p(t.data_ptr()), n_rows, dim, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 0,
                                         C.c_void_p(stream)), "fcp_table_audit")

        legs = collections.OrderedDict()
        legs["audit"] = timed(torch, audit, reps)
        legs["quantise"] = timed(torch, lambda: tables.convert(t, "q8", out=q8), reps)
        legs["copy"] = timed(torch, lambda: twin.copy_(t), reps)
        legs["torch"] = timed(torch, lambda: torch_composition(torch, tables, t), max(3, reps // 4))
        gb = t.numel() * 4 / 1e9
        a = tables.audit(t)
        for name, (med, lo, hi) in legs.items():
            print(f"{n_rows} x {dim}  {name:9s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f})  {gb / (med * 1e-3):8.1f} GB/s of float32 read", flush=True)
        print(f"{n_rows} x {dim}  audit: nonfinite {a.rows_nonfinite}, " +
              ", ".join(f"{k} bad {a.kinds[k].rows_bad} rel. sq. err {a.kinds[k].sum_sq_err / a.sum_sq:.3e}" for k in ("bf16", "f16", "q8")), flush=True)
        results.append({"rows": n_rows, "dim": dim, **{name: {"median_ms": v[0], "min_ms": v[1], "max_ms": v[2]} for name, v in legs.items()}})
        del t, q8, twin
    # the chooser on S2: one table resident at a time
    model = synth.model_s2(vocab=vocab)
    audits = []
    for i, tab in enumerate(model.tables):
        audits.append(tables.audit(synth.hash_table_torch(tab.seed, tab.vocab, tab.dim, dev)))
    totals = {k: sum(tab.vocab * tables.row_bytes(k, tab.dim) for tab in model.tables) for k in ("f32", "f16", "q8")}
    print(f"S2, vocab {vocab}: float32 {totals['f32']} bytes, 16-bit {totals['f16']}, q8 {totals['q8']}", flush=True)
    chosen = []
    for share in (0.0, 0.1, 0.25, 0.5, 0.75, 1.0):
        budget = int(totals["q8"] + share * (totals["f32"] - totals["q8"]))
        names, nbytes, err = tables.choose_dtypes(model.spec, audits, budget)
        by_dim = collections.Counter((tab.dim, n) for tab, n in zip(model.tables, names))
        print(f"budget {budget} ({share:.2f} of the way from q8 to float32): {nbytes} bytes, weighted error {err:.4e}, "
              + ", ".join(f"dim {d} {n} x{c}" for (d, n), c in sorted(by_dim.items())), flush=True)
        chosen.append({"budget": budget, "bytes": nbytes, "error": err, "by_dim": {f"{d}:{n}": c for (d, n), c in sorted(by_dim.items())}})
    print(json.dumps({"timings": results, "s2_vocab": vocab, "s2_totals": totals, "s2_choices": chosen}), flush=True)
    torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24, help="rows of the dim-64 table")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--vocab", type=int, default=1_000_000, help="rows of S2's tables in the chooser's part")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        child(args.rows, args.reps, args.vocab)
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows),
           "--reps", str(args.reps), "--vocab", str(args.vocab)]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
