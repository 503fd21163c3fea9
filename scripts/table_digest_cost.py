"""What the table digest costs (profiles/table_digest.txt).

One table of 16 M rows of dim 64 as float32 (4.3 GB), bf16 and q8.  Per format, the median of warm HIP-event timings of
  digest       fcp_table_digest (the digest kernel and its fold), result and workspace allocated once;
  copy         a device-to-device copy of the same bytes (reads and writes every byte once);
  digest_rows  fcp_table_digest_rows of 1 M pairwise distinct ids of the table, in a seeded random order;
and, for the float32 table in the same process,
  audit        fcp_table_audit, which reads the same bytes and does far more arithmetic per byte;
and once per format, by the wall clock,
  host         the composition the digest replaces: the table copied to the host and fcp_table_digest_host there (its value
               is compared with the device's: the line says `equal`).
No threshold anywhere: the times are recorded.

    python scripts/table_digest_cost.py [--rows 16777216] [--dim 64] [--ids 1000000] [--reps 20] [--out profiles/table_digest.txt]

The driver starts ONE child process under its own `timeout` and never opens the GPU itself."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD = """fcp_table_digest: what it costs beside a copy, the audit and the host
====================================================================
Produced by scripts/table_digest_cost.py (one MI355X, one child process under its own timeout; medians of {reps} warm HIP-event
timings per device leg; the host leg once, by the wall clock; table contents the closed form of synth.hash_table_torch
converted by tables.convert).  GB/s is the bytes of the table in its own format over the median (digest_rows: the bytes of
the rows named).

    python scripts/table_digest_cost.py --rows {rows} --dim {dim} --ids {ids} --reps {reps}

"""


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


def child(rows: int, dim: int, n_ids: int, reps: int, out_path: str) -> None:
    import torch
    from recom_amd import lib as _lib
    from recom_amd import synth, tables
    dev = torch.device("cuda", 0)
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((C.sizeof(_lib.TableDigest) // 8,), dtype=torch.int64, device=dev)
    ws = torch.empty((L.fcp_table_digest_workspace_bytes() // 8,), dtype=torch.int64, device=dev)
    audit_out = torch.empty(((C.sizeof(_lib.TableAudit) + 7) // 8,), dtype=torch.int64, device=dev)
    audit_ws = torch.empty((L.fcp_table_audit_workspace_bytes() // 8,), dtype=torch.int64, device=dev)
    ids = torch.randperm(rows, generator=torch.Generator().manual_seed(5))[:n_ids].to(dev)
    lines = []

    def say(line: str) -> None:
        print(line, flush=True)
        lines.append(line)

    master = synth.hash_table_torch(7, rows, dim, dev)
    for kind in ("f32", "bf16", "q8"):
        t = master if kind == "f32" else tables.convert(master, kind)
        k = _lib.TABLE_KINDS[kind]
        twin = torch.empty_like(t)
        nbytes = t.numel() * t.element_size()

        def digest():
            _lib.check(L.fcp_table_digest(C.c_void_p(t.data_ptr()), k, rows, dim, 0, 1, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                          0, C.c_void_p(stream)), "fcp_table_digest")

        def digest_rows():
            _lib.check(L.fcp_table_digest_rows(C.c_void_p(t.data_ptr()), k, rows, dim, 0, 1, C.c_void_p(ids.data_ptr()), n_ids,
                                               C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 0, C.c_void_p(stream)), "fcp_table_digest_rows")

        def audit():
            _lib.check(L.fcp_table_audit(C.c_void_p(t.data_ptr()), rows, dim, C.c_void_p(audit_out.data_ptr()), C.c_void_p(audit_ws.data_ptr()), 0,
                                         C.c_void_p(stream)), "fcp_table_audit")

        legs = [("digest", digest, nbytes), ("copy", lambda: twin.copy_(t), nbytes)]
        if kind == "f32":
            legs.append(("audit", audit, nbytes))
        legs.append(("digest_rows", digest_rows, n_ids * tables.row_bytes(kind, dim)))
        for name, fn, moved in legs:
            med, lo, hi = timed(torch, fn, reps)
            say(f"{rows} x {dim} {kind:4s} {name:11s} median {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f})  {moved / 1e9 / (med * 1e-3):8.1f} GB/s")
        del twin
        on_device = tables.digest(t)
        t0 = time.perf_counter()
        host = t.cpu()
        t1 = time.perf_counter()
        on_host = tables.digest_host(host, kind)
        t2 = time.perf_counter()
        say(f"{rows} x {dim} {kind:4s} host        copy to the host {1e3 * (t1 - t0):9.1f} ms + fcp_table_digest_host {1e3 * (t2 - t1):9.1f} ms  "
            f"({nbytes / 1e9 / (t2 - t0):.2f} GB/s); device {on_device:016x}, host {on_host:016x}: {'equal' if on_device == on_host else 'DIFFERENT'}")
        del host
        if kind != "f32":
            del t
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(HEAD.format(rows=rows, dim=dim, ids=n_ids, reps=reps) + "\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--ids", type=int, default=1_000_000, help="pairwise distinct ids of the digest_rows leg")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_digest.txt"), help="the record this run writes")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        child(args.rows, args.dim, args.ids, args.reps, args.out)
        return
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows),
           "--dim", str(args.dim), "--ids", str(args.ids), "--reps", str(args.reps), "--out", args.out]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit(f"the measurement ended with exit status {r.returncode}")


if __name__ == "__main__":
    main()
