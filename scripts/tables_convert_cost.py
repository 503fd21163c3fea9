"""What fcp_table_convert reaches: S2's table shapes — dims 8 / 16 / 32 / 64 at 1 M rows each, and one 16 M-row table —
converted in every direction (float32 -> q8 / bf16 / fp16 and back), each timed with HIP events after a warm-up, against a
device-to-device copy of the SAME source bytes in the same process: the copy is the yardstick (there is no parent-commit
figure).  No threshold: GB/s of source read and the ratio to the copy are recorded (profiles/tables_convert.txt).

    python scripts/tables_convert_cost.py [--out profiles/tables_convert.txt] [--big-dim 64] [--min-ms 200]

Every conversion is first checked on sampled rows against the CPU restatement (a wrong kernel is refused, not timed).  A
timed window holds as many back-to-back calls as fill --min-ms and ends in an event synchronise; three windows per figure,
the median is reported with the spread.  Without a GPU the script fails: it never falls back."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 8), (1_000_000, 16), (1_000_000, 32), (1_000_000, 64)]
BIG_ROWS = 16_000_000
COMPACT = ("q8", "bf16", "f16")


def timed(torch, fn, min_ms: float):
    """(median ms per call, spread ms) of fn(): a warm-up, then three windows of enough calls to fill min_ms each."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    fn()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    calls = max(3, int(min_ms / max(start.elapsed_time(stop), 1e-3)) + 1)
    per_call = []
    for _ in range(3):
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        per_call.append(start.elapsed_time(stop) / calls)
    return statistics.median(per_call), max(per_call) - min(per_call), calls


def check(torch, tables, synth, src32, conv, dtype) -> int:
    """Sampled rows of a converted table and of its way back against the CPU restatements."""
    rows = src32.shape[0]
    idx = np.unique(np.concatenate([np.arange(64), np.arange(rows - 64, rows), np.random.default_rng(1).integers(0, rows, 2000)]))
    sel = torch.from_numpy(idx).to(src32.device)
    x = src32[sel].cpu().numpy()
    back = tables.convert(conv, "f32")[sel].cpu().numpy()
    if dtype == "q8":
        want = synth.quantize_q8(x)
        ok = (conv[sel].cpu().numpy() == want).all() and (back.view(np.uint32) == synth.dequantize_q8(want).view(np.uint32)).all()
    else:
        want = synth.table_patterns(x, dtype)
        got = conv[sel].cpu().view(torch.int16).numpy().view(np.uint16)
        ok = (got == want).all() and (back.view(np.uint32) == synth.table_values(want, dtype).view(np.uint32)).all()
    if not ok:
        raise SystemExit(f"{dtype} [{rows}, {src32.shape[1]}]: the converted table is not what the value model says; nothing timed")
    return len(idx)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables_convert.txt"))
    ap.add_argument("--big-dim", type=int, default=64, help="dim of the 16 M-row table")
    ap.add_argument("--min-ms", type=float, default=200.0, help="least length of a timed window")
    args = ap.parse_args()
    import torch
    from recom_amd import synth, tables
    if not torch.cuda.is_available():
        raise SystemExit("NOT MEASURED: no GPU (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    lines = [f"fcp_table_convert against a device-to-device copy of the same source bytes ({torch.cuda.get_device_name(0)})",
             "GB/s = source bytes read / time; ratio = copy time / convert time of the same source (1.0 = the copy's rate)",
             f"{'rows':>9} {'dim':>4} {'direction':>12} {'src MB':>8} {'dst MB':>8} {'us/call':>9} {'spread':>7} {'GB/s':>7} "
             f"{'copy GB/s':>9} {'ratio':>6} calls"]
    records = []
    for rows, dim in SHAPES + [(BIG_ROWS, args.big_dim)]:
        src32 = synth.hash_table_torch(7, rows, dim, dev)
        for dtype in COMPACT:
            conv = tables.convert(src32, dtype)
            torch.cuda.synchronize()
            checked = check(torch, tables, synth, src32, conv, dtype)
            wide = torch.empty_like(src32)
            for name, src, dst, to in ((f"f32->{dtype}", src32, conv, dtype), (f"{dtype}->f32", conv, wide, "f32")):
                twin = torch.empty_like(src)
                copy_ms, copy_spread, _ = timed(torch, lambda: twin.copy_(src), args.min_ms)
                ms, spread, calls = timed(torch, lambda: tables.convert(src, to, out=dst), args.min_ms)
                sb, db = src.numel() * src.element_size(), dst.numel() * dst.element_size()
                rec = {"rows": rows, "dim": dim, "direction": name, "src_bytes": sb, "dst_bytes": db, "us_per_call": ms * 1e3,
                       "spread_us": spread * 1e3, "gbps_source": sb / ms / 1e6, "copy_gbps_source": sb / copy_ms / 1e6,
                       "copy_spread_us": copy_spread * 1e3, "ratio_to_copy": copy_ms / ms, "calls_per_window": calls, "rows_checked": checked}
                records.append(rec)
                lines.append(f"{rows:>9} {dim:>4} {name:>12} {sb / 1e6:>8.1f} {db / 1e6:>8.1f} {ms * 1e3:>9.1f} {spread * 1e3:>7.1f} "
                             f"{rec['gbps_source']:>7.0f} {rec['copy_gbps_source']:>9.0f} {rec['ratio_to_copy']:>6.2f} {calls}")
                print(lines[-1], flush=True)
                del twin
            del conv, wide
        del src32
        torch.cuda.empty_cache()
    lines.append("")
    lines.append("(a copy reads and writes the source's bytes; float32 -> q8 writes (dim + 8) / (4 dim) of what it reads, float32 -> "
                 "16-bit half; the ways back write more than they read)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"records": records}), flush=True)


if __name__ == "__main__":
    main()
