"""fcp_table_audit / fcp_table_formats_choose (recom_amd/csrc/fcp_table_audit.hip, fcp_plan_desc.cc): the value model restated,
the rows the GPU test audits, and the synthetic instances of the chooser's tests (tests/test_table_audit_host.py on the CPU,
tests/native/table_formats_san.cc under the sanitizers, tests/test_gpu_table_audit.py on the GPU).  Test data only.

The audit's rt(x) is what the library does on the way to a format and back, and every half of it has its restatement
already: narrow_output_cases.narrow + table16_cases.widen (float32 -> 16-bit -> float32), table_convert_cases.quantize_ref +
synth.dequantize_q8 (float32 -> q8 -> float32).  `audit_ref` composes them; the squares of the float32 errors are exact in
float64 and summed by numpy in float64."""
import functools
import itertools

import numpy as np

import narrow_output_cases as NO
import table16_cases as T16
import table_convert_cases as TC
from recom_amd import synth

KINDS = TC.KINDS                               # name -> FCP_TAB_*
COMPACT = ("bf16", "f16", "q8")
FLT_MAX = TC.FLT_MAX
GRID_BLOCKS = 2048                             # kAuditBlocks: the fixed grid
BLOCK_THREADS = 256

# every V, every lane-group size, dims on both sides of a group's edge, and — per V — one dim beyond the in-register cap of the
# 64-lane group (64 * 4 * V elements)
DIMS = (1, 2, 3, 4, 5, 8, 12, 20, 61, 62, 64, 128, 130, 300, TC.REGISTER_CAP[4] + 4, TC.REGISTER_CAP[2] + 2, TC.REGISTER_CAP[1] + 1)


def rows_per_block(dim: int) -> int:
    return BLOCK_THREADS // TC.group_of(dim)


def special_rows(dim: int) -> np.ndarray:
    """The rows the issue names, at width `dim`; a value sits at the row's last element (a lane of the group other than the
    first wherever the group has more than one), the rest is a small ramp.  Rows that need two elements are left out at dim 1."""
    ramp = (np.arange(dim, dtype=np.float32) % 7 - 3) / np.float32(8.0)
    rows = []

    def with_last(*vals):
        r = ramp.copy()
        r[dim - len(vals):] = vals
        rows.append(r)

    for v in (np.nan, np.inf, -np.inf):                    # non-finite
        with_last(v)
    with_last(np.float32(65519.996))                       # the largest float32 below 65520: rounds to 65504, good for fp16
    with_last(65520.0)                                     # rounds to +inf in fp16
    with_last(-65520.0)
    with_last(FLT_MAX)                                     # rounds to +inf in bf16 (and fp16)
    with_last(-FLT_MAX)
    with_last(float(np.float32(3.3895314e38)))             # 0x7F7F0000: the largest bf16, good for bf16
    if dim >= 2:
        with_last(-3e38, 3e38)                             # max - min overflows: bad for q8 (and out of fp16's range)
        with_last(np.nan, np.inf)
        with_last(-0.0, 0.0)
    rows.append(np.full(dim, 1.2345678, np.float32))       # constant: q8 error 0
    rows.append(np.full(dim, -0.0, np.float32))
    sub = np.float32(2.0 ** -149)
    rows.append((sub * (np.arange(dim) % 5 + 1)).astype(np.float32))                 # float32 denormals
    rows.append((np.float32(2.0 ** -24) * (np.arange(dim) % 3 - 1)).astype(np.float32))   # fp16 denormal range
    with np.errstate(all="ignore"):
        return np.stack(rows).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pool(dim: int) -> np.ndarray:
    """float32 [n, dim]: table_convert_cases' families and edge list and the special rows, shuffled with a fixed seed so that a
    prefix of any length holds all three."""
    rows = np.concatenate([TC.family_rows(dim, 300, 11), TC.edge_rows(dim)[:120], special_rows(dim)])
    out = rows[np.random.default_rng(100 + dim).permutation(len(rows))]
    out.setflags(write=False)
    return out


# rows a test puts at the first / the last row of a table, by what they are bad for ("q8_bad" needs two elements: dim >= 2)
NAMED = ("nan", "neg_inf", "f16_bad", "bf16_bad", "q8_bad", "good")


def named_row(dim: int, name: str) -> np.ndarray:
    r = ((np.arange(dim, dtype=np.float32) % 5 - 2) / np.float32(4.0)).astype(np.float32)
    if name == "q8_bad":
        r[0], r[-1] = 3e38, -3e38            # (dim 1: -3e38 alone, bad for the 16-bit kinds only)
    elif name != "good":
        r[-1] = {"nan": np.nan, "neg_inf": -np.inf, "f16_bad": -65520.0, "bf16_bad": FLT_MAX}[name]
    return r


@functools.lru_cache(maxsize=None)
def source(dim: int) -> np.ndarray:
    """float32 [n, dim]: the pool, then the NAMED rows.  Every table of the GPU test is rows of this array (`table_index`), so
    the CPU judges each row once (`source_stats`)."""
    out = np.concatenate([pool(dim), np.stack([named_row(dim, n) for n in NAMED])])
    out.setflags(write=False)
    return out


def table_index(dim: int, rows: int, first=None, last=None) -> np.ndarray:
    """int64 [rows]: the pool, cycled; `first` / `last` (a NAMED row, or None) replace the first / the last row."""
    n = len(pool(dim))
    idx = np.arange(rows, dtype=np.int64) % n
    if rows and last is not None:
        idx[-1] = n + NAMED.index(last)
    if rows and first is not None:
        idx[0] = n + NAMED.index(first)
    return idx


def rt(x: np.ndarray, kind: str) -> np.ndarray:
    """float32: x through `kind` and back; q8 rows must be finite with a finite range."""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "q8":
        return synth.dequantize_q8(TC.quantize_ref(x)) if len(x) else x.copy()
    return T16.widen(NO.narrow(x, kind), kind)


def row_stats(x: np.ndarray) -> dict:
    """Every row of float32 [rows, dim] judged on its own: {"finite" (mask), "sq" (float64 sum of squares), kind: {"bad"
    (mask: finite and not held by the kind), "sse" (float64, 0 for rows left out), "max" (float32, 0 for rows left out)}}."""
    x = np.ascontiguousarray(x, np.float32)
    finite = np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        out = {"finite": finite, "sq": np.where(finite, (x.astype(np.float64) ** 2).sum(axis=1), 0.0)}
        for kind in COMPACT:
            if kind == "q8":
                bad = finite & ~np.isfinite((x.max(axis=1) - x.min(axis=1)).astype(np.float32))
            else:
                bad = finite & np.isinf(rt(np.where(finite[:, None], x, np.float32(0.0)), kind)).any(axis=1)
            good = finite & ~bad
            e = np.zeros(x.shape, np.float32)
            e[good] = (x[good] - rt(x[good], kind)).astype(np.float32)
            out[kind] = {"bad": bad, "sse": (e.astype(np.float64) ** 2).sum(axis=1), "max": np.abs(e).max(axis=1).astype(np.float32)}
    return out


@functools.lru_cache(maxsize=None)
def source_stats(dim: int) -> dict:
    return row_stats(source(dim))


def aggregate(stats: dict, idx: np.ndarray) -> dict:
    """The audit of the table whose row r is row idx[r] of the judged array: {"rows", "rows_nonfinite", "first_nonfinite_row",
    "sum_sq", kind: {"rows_bad", "first_bad_row", "sum_sq_err", "max_abs_err" (float32)}}; the sums are numpy's float64 sums of
    the rows' float64 sums."""
    idx = np.asarray(idx, np.int64)

    def first(mask):
        return int(np.argmax(mask)) if mask.any() else -1

    nonfinite = ~stats["finite"][idx]
    out = {"rows": len(idx), "rows_nonfinite": int(nonfinite.sum()), "first_nonfinite_row": first(nonfinite), "sum_sq": float(stats["sq"][idx].sum())}
    for kind in COMPACT:
        bad = stats[kind]["bad"][idx]
        mx = stats[kind]["max"][idx]
        out[kind] = {"rows_bad": int(bad.sum()), "first_bad_row": first(bad), "sum_sq_err": float(stats[kind]["sse"][idx].sum()),
                     "max_abs_err": np.float32(mx.max() if len(idx) else 0.0)}
    return out


def audit_ref(x: np.ndarray) -> dict:
    """The audit of float32 [rows, dim] on the CPU."""
    return aggregate(row_stats(x), np.arange(len(x)))


# ---- the chooser's synthetic instances ----------------------------------------------------------------------------------------
def row_bytes(kind: int, dim: int) -> int:
    return (4 * dim, 2 * dim, 2 * dim, dim + 8)[kind]


def draw_instance(seed: int, n_tables: int) -> dict:
    """One instance: per table rows, dim, sum_sq, rows_nonfinite and, per compact kind, rows_bad and a continuous sum_sq_err (no
    ties); some tables with a bad fp16 / bf16 / q8 row or a NaN row, dims 1 and 2 among the others; `weights` None or drawn."""
    rng = np.random.default_rng(seed)
    tabs = []
    for _ in range(n_tables):
        dim = int(rng.choice([1, 2, 3, 4, 8, 16, 64, 300]))
        rows = int(rng.integers(1, 2000))
        sse = [0.0] + [float(rng.random() * 10.0 ** rng.integers(-6, 1)) for _ in range(3)]
        bad = [0] + [int(rng.random() < 0.15) * int(rng.integers(1, 5)) for _ in range(3)]
        tabs.append({"rows": rows, "dim": dim, "sum_sq": float(rng.random() * 100.0) if rng.random() < 0.9 else 0.0,
                     "rows_nonfinite": int(rng.random() < 0.1), "sse": sse, "bad": bad})
    weights = None if seed % 3 else [float(rng.random() * 3.0) for _ in range(n_tables)]
    allowed = 0b1111 if seed % 5 else int(rng.integers(0, 16))
    return {"tables": tabs, "weights": weights, "allowed": allowed}


def instances():
    return [draw_instance(seed, 1 + seed % 6) for seed in range(60)]


def weight_of(inst: dict, t: int) -> float:
    if inst["weights"] is not None:
        return inst["weights"][t]
    s = inst["tables"][t]["sum_sq"]
    return 1.0 / s if s > 0 else 0.0


def admissible(inst: dict, t: int) -> list:
    tab = inst["tables"][t]
    return [k for k in range(4) if k == 0 or (inst["allowed"] >> k & 1 and tab["rows_nonfinite"] == 0 and tab["bad"][k] == 0)]


def assignment_cost(inst: dict, kinds) -> tuple:
    """(bytes, weighted error) of one kind per table"""
    nbytes = sum(tab["rows"] * row_bytes(k, tab["dim"]) for tab, k in zip(inst["tables"], kinds))
    err = sum(weight_of(inst, t) * tab["sse"][k] for t, (tab, k) in enumerate(zip(inst["tables"], kinds)))
    return nbytes, err


def all_assignments(inst: dict):
    """every admissible assignment with its (bytes, error): at most 4^6"""
    for kinds in itertools.product(*[admissible(inst, t) for t in range(len(inst["tables"]))]):
        yield kinds, assignment_cost(inst, kinds)


def budgets(inst: dict) -> list:
    """budgets from below the smallest assignment to above all-float32, the two ends included"""
    sizes = sorted({b for _, (b, _) in all_assignments(inst)})
    lo, hi = sizes[0], sizes[-1]
    return sorted({lo - 1, lo, hi, hi + 1000} | {lo + (hi - lo) * i // 7 for i in range(1, 7)} | set(sizes[1:4]))


def write_instances(path: str) -> list:
    """The instances and budgets as text for tests/native/table_formats_san.cc, floats as C99 hex; returns the (instance,
    budget) list in file order.  Per case: `n allowed has_weights budget`, then per table `rows dim rows_nonfinite sum_sq`
    `bad1 sse1 bad2 sse2 bad3 sse3 weight`."""
    cases = []
    with open(path, "w") as f:
        for inst in instances():
            for budget in budgets(inst):
                cases.append((inst, budget))
                f.write(f"{len(inst['tables'])} {inst['allowed']} {int(inst['weights'] is not None)} {budget}\n")
                for t, tab in enumerate(inst["tables"]):
                    w = inst["weights"][t] if inst["weights"] is not None else 0.0
                    per_kind = " ".join(f"{tab['bad'][k]} {float(tab['sse'][k]).hex()}" for k in (1, 2, 3))
                    f.write(f"{tab['rows']} {tab['dim']} {tab['rows_nonfinite']} {float(tab['sum_sq']).hex()} {per_kind} {float(w).hex()}\n")
    return cases
