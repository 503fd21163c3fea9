"""fcp_table_digest / fcp_table_digest_rows / fcp_table_digest_host (recom_amd/csrc/fcp_table_digest.hip,
fcp_table_digest_host.cc): the NumPy reference of the header's value model, the known answers, and the tables the host tests
(tests/test_table_digest_host.py, tests/native/table_digest_san.cc under the sanitizers) and the GPU tests
(tests/test_gpu_table_digest.py) share.  Test data only.  A digest is about BYTES: most tables here are random bytes, whatever
floats they may spell."""
import numpy as np

KINDS = ("f32", "bf16", "f16", "q8")            # index = FCP_TAB_*
KIND = {name: k for k, name in enumerate(KINDS)}
DIMS = (1, 2, 3, 4, 5, 7, 8, 64, 129, 300)      # dim 129 as float32: 65 words, longer than one 64-lane pass
Q8_TAIL_DIMS = tuple(range(1, 9))               # q8 rows of 9 .. 16 bytes: every tail remainder
G = np.uint64(0x9e3779b97f4a7c15)
M64 = (1 << 64) - 1

# the kernel's geometry (fcp_table_digest.hip), restated: what "one full pass of the fixed grid" means
GRID_BLOCKS, BLOCK_THREADS, UNROLL = 2048, 256, 4


def row_bytes(kind: str, dim: int) -> int:
    return {"f32": 4 * dim, "bf16": 2 * dim, "f16": 2 * dim, "q8": dim + 8}[kind]


def mix(x):
    """the 64-bit finaliser on uint64 arrays (arrays wrap silently; scalars would warn)"""
    x = np.atleast_1d(np.asarray(x, np.uint64)).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def row_hashes(raw, kind: str, dim: int, r) -> np.ndarray:
    """uint64 [rows]: H of the rows whose bytes `raw` holds back to back (anything with a buffer), `r` their GLOBAL indices."""
    k = KIND[kind]
    rb = row_bytes(kind, dim)
    raw = np.frombuffer(raw, np.uint8)
    assert raw.size % rb == 0
    rows = raw.size // rb
    nw = (rb + 7) // 8
    pad = np.zeros((rows, nw * 8), np.uint8)
    pad[:, :rb] = raw.reshape(rows, rb)
    w = pad.view("<u8")
    t = mix(w ^ (np.arange(1, nw + 1, dtype=np.uint64) * G)[None, :]).reshape(rows, nw).sum(axis=1, dtype=np.uint64)
    r = np.asarray(r, np.uint64).reshape(rows)
    salt = mix(np.uint64(((k + 1) << 32) | dim))
    return mix(salt + (r + np.uint64(1)) * G + t).reshape(rows)


def digest(raw, kind: str, dim: int, row0: int = 0, step: int = 1) -> int:
    """The header's value model: `raw` is the rows' bytes, back to back; local row i has the global index row0 + i * step."""
    rows = len(np.frombuffer(raw, np.uint8)) // row_bytes(kind, dim)
    r = np.uint64(row0) + np.arange(rows, dtype=np.uint64) * np.uint64(step)
    return int(row_hashes(raw, kind, dim, r).sum(dtype=np.uint64))


def digest_ids(raw, kind: str, dim: int, ids, row0: int = 0, step: int = 1):
    """(sum, rows, skipped) of fcp_table_digest_rows: `raw` the whole table's bytes, every id in [0, table_rows) adds its row's
    hash at global index row0 + id * step, as often as it occurs."""
    rb = row_bytes(kind, dim)
    table = np.frombuffer(raw, np.uint8).reshape(-1, rb)
    ids = np.asarray(ids, np.int64).reshape(-1)
    inside = (ids >= 0) & (ids < table.shape[0])
    named = ids[inside]
    r = np.uint64(row0) + named.astype(np.uint64) * np.uint64(step)
    total = int(row_hashes(np.ascontiguousarray(table[named]).tobytes(), kind, dim, r).sum(dtype=np.uint64))
    return total, int(inside.sum()), int((~inside).sum())


# (raw bytes, kind, dim, digest) with row0 = 0, step = 1: the issue's known answers, from the reference above
KNOWN = ((np.arange(9, dtype=np.float32).tobytes(), "f32", 3, 0xb3c088b12d9a2c7b),
         (bytes(range(26)), "q8", 5, 0xf02c1c2d5524c510),
         (bytes([0x80, 0x3f]), "bf16", 1, 0xfedb7d7a64af8385),
         (bytes([0x80, 0x3f]), "f16", 1, 0x4ed690b53bc2c10f),
         (np.zeros((4, 8), np.float32).tobytes(), "f32", 8, 0xea62b1552a94f6ad))


def draw_raw(kind: str, dim: int, rows: int, seed: int) -> np.ndarray:
    """uint8 [rows, row_bytes]: random bytes"""
    return np.random.default_rng([seed, KIND[kind], dim, rows]).integers(0, 256, (rows, row_bytes(kind, dim)), dtype=np.uint8)


def words_of(kind: str, dim: int) -> int:
    return (row_bytes(kind, dim) + 7) // 8


def group_of(kind: str, dim: int) -> int:
    """lanes that share a row: the largest power of two not above the row's 64-bit words, at most 64"""
    g = 1
    while 2 * g <= words_of(kind, dim) and g < 64:
        g <<= 1
    return g


def full_pass_rows(kind: str, dim: int, steps: int = 1) -> int:
    """rows that `steps` strides of the full grid cover (a block's loop body handles UNROLL strides)"""
    return steps * GRID_BLOCKS * (BLOCK_THREADS // group_of(kind, dim))


def torch_dtype(torch, kind: str):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "q8": torch.uint8}[kind]


def as_table(torch, raw: np.ndarray, kind: str, dim: int, device, front: int = 0):
    """The device table whose bytes are `raw` (uint8 [rows, row_bytes]), in the torch dtype of `kind`.  `front`: bytes in front
    of the table inside its allocation (multiples of the element size), to place the base at a chosen alignment."""
    rows = raw.shape[0]
    buf = torch.empty((front + raw.size,), dtype=torch.uint8, device=device)
    body = buf[front:]
    body.copy_(torch.from_numpy(np.array(raw, np.uint8).reshape(-1)))        # (a copy: `raw` may be a read-only view of bytes)
    if kind == "q8":
        return body.view(rows, dim + 8)
    return body.view(torch_dtype(torch, kind)).view(rows, dim)


def bytes_of(torch, table) -> np.ndarray:
    """the table's bytes, copied back"""
    return table.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def host_cases():
    """(kind, dim, rows, row0, step, raw) for the host tests and the sanitizer program: every kind at every dim, the q8 tails,
    rows 0 / 1 / several, other row0 / step."""
    out = []
    for kind in KINDS:
        dims = DIMS + (Q8_TAIL_DIMS if kind == "q8" else ())
        for n, dim in enumerate(sorted(set(dims))):
            for rows, row0, step in ((0, 0, 1), (1, 0, 1), (5, 0, 1), (11, 3 + n, 1 + n % 4)):
                out.append((kind, dim, rows, row0, step, draw_raw(kind, dim, rows, 7)))
    out.append(("f32", 8, 3, (1 << 62), 1 << 30, draw_raw("f32", 8, 3, 8)))     # large indices: the arithmetic wraps, the check does not
    return out


def write_cases(path: str) -> int:
    """The known answers and host_cases as text for tests/native/table_digest_san.cc: one case per line,
    `kind dim rows row0 step expected-hex bytes-hex` ("-" for no bytes); returns the number of lines."""
    lines = []
    for raw, kind, dim, want in KNOWN:
        lines.append(f"{KIND[kind]} {dim} {len(raw) // row_bytes(kind, dim)} 0 1 {want:016x} {bytes(raw).hex()}")
    for kind, dim, rows, row0, step, raw in host_cases():
        lines.append(f"{KIND[kind]} {dim} {rows} {row0} {step} {digest(raw.tobytes(), kind, dim, row0, step):016x} {raw.tobytes().hex() or '-'}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
