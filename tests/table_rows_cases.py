"""fcp_table_update_rows / fcp_table_read_rows (recom_amd/csrc/fcp_table_rows.hip): the ids, the poisoned tables and the small
served model the GPU tests share (tests/test_gpu_table_rows.py, tests/test_zzz_gpu_table_rows_stream.py).  Test data only;
every expectation comes from the restatements of table_convert_cases / narrow_output_cases / table16_cases / synth."""
import numpy as np

import narrow_output_cases as N
import table_convert_cases as TC
from recom_amd import synth

POISON = 0xA5
SLACK_ROWS = 37                  # rows of a table no delta names: table_rows = n + SLACK_ROWS
BEHIND_ROWS = 3                  # poisoned rows behind the table, inside the allocation
INT64_MIN = -(1 << 63)


def row_bytes(kind: str, dim: int) -> int:
    return {"f32": 4 * dim, "bf16": 2 * dim, "f16": 2 * dim, "q8": dim + 8}[kind]


def distinct_ids(n: int, table_rows: int, seed: int, exclude=()) -> np.ndarray:
    """int64 [n], pairwise distinct, a seeded permutation prefix of [0, table_rows) with row 0 and row table_rows - 1 forced
    in (n == 1 has room for one of them: the last row, the one next to what lies behind the table).  `exclude`: rows that
    are never named."""
    rng = np.random.default_rng(seed)
    last = table_rows - 1
    if n == 1:
        return np.asarray([last], np.int64)
    rest = [int(r) for r in rng.permutation(table_rows) if r not in (0, last) and r not in exclude][:n - 2]
    ids = np.asarray([0, last] + rest, np.int64)[rng.permutation(n)]
    assert ids.shape == (n,) and len(np.unique(ids)) == n and ids.min() == 0 and ids.max() == last
    return ids


def expect_bytes(x: np.ndarray, kind: str) -> np.ndarray:
    """uint8 [rows, row_bytes]: the bytes fcp_table_convert's value model gives the float32 rows x in format `kind`."""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "q8":
        return TC.quantize_ref(x)
    if kind == "f32":
        return x.view(np.uint8).reshape(x.shape[0], -1).copy()
    return np.ascontiguousarray(N.narrow(x, kind)).view(np.uint8).reshape(x.shape[0], -1).copy()


def poisoned(torch, kind: str, dim: int, table_rows: int, device):
    """(buffer, table): a uint8 buffer of table_rows + BEHIND_ROWS rows of `kind`, every byte POISON, and the table
    [table_rows, ...] in the torch dtype of `kind` that is its front."""
    rb = row_bytes(kind, dim)
    buf = torch.full(((table_rows + BEHIND_ROWS) * rb,), POISON, dtype=torch.uint8, device=device)
    front = buf[:table_rows * rb]
    if kind == "q8":
        table = front.view(table_rows, dim + 8)
    else:
        table = front.view({"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]).view(table_rows, dim)
    assert table.data_ptr() == buf.data_ptr() and table.is_contiguous()
    return buf, table


def check_poisoned(buf, kind: str, dim: int, table_rows: int, ids: np.ndarray, want_rows: np.ndarray, what) -> None:
    """The whole buffer, as bytes: `want_rows` at `ids`, POISON everywhere else, the rows behind the table included."""
    rb = row_bytes(kind, dim)
    got = buf.cpu().numpy().reshape(table_rows + BEHIND_ROWS, rb)
    want = np.full_like(got, POISON)
    want[ids] = want_rows
    bad = np.argwhere((got != want).any(axis=1))[:, 0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first row {bad[0]} (named: {bad[0] in set(ids.tolist())}): {got[bad[0]]} want {want[bad[0]]}"


# ---- a small served model: one gather and one pooled column (narrow_output_cases._small_spec) --------------------------------
def small_model(seed: int = 21):
    """(spec, float32 masters [2], deltas [(ids, rows)] naming a third of each table's rows, request (inputs, symbols)) of
    the two-column spec of the refusal cases: a gather of dim 8 over 50 rows, a mean-pooled column of dim 4 over 60 rows.
    The request names every row of both tables and ids outside them."""
    spec = N._small_spec()
    rng = np.random.default_rng(seed)
    masters, deltas = [], []
    for c in spec.columns:
        masters.append(rng.standard_normal((c.vocab, c.dim)).astype(np.float32))
        ids = np.sort(rng.permutation(c.vocab)[:c.vocab // 3]).astype(np.int64)
        deltas.append((ids, (3.0 * rng.standard_normal((len(ids), c.dim))).astype(np.float32)))
    g, p = spec.columns
    rows = g.vocab + 4
    ids0 = np.concatenate([rng.permutation(g.vocab), [g.vocab, -1, 1 << 40, 7]]).astype(np.int64)
    lens = rng.integers(0, 5, rows)
    nnz = int(lens.sum())
    ids1 = np.concatenate([rng.permutation(p.vocab), rng.integers(-2, p.vocab + 2, max(nnz - p.vocab, 0))])[:nnz].astype(np.int64)
    csr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    inputs = [ids0, ids1, csr, np.ones(nnz, np.float32)]
    return spec, masters, deltas, (inputs, np.asarray([rows], np.int32))


def small_model_expected_tables(masters, deltas):
    """(q8 tables, their dequantised float32 twins) after the deltas, from the restatements alone."""
    q8, deq = [], []
    for m, (ids, rows) in zip(masters, deltas):
        m = m.copy()
        m[ids] = rows
        q8.append(TC.quantize_ref(m))
        deq.append(synth.dequantize_q8(q8[-1]))
    return q8, deq
