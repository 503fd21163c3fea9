#!/usr/bin/env python3
"""Golden vectors produced by the REFERENCE's own host functions (oracle/_ref/libref_bucketize.so, built by
oracle/ref_extract.py from the reference's source where that source lies): `Bucketize` (cuda_emitter.cc:233-247) and the
arena alignment `alignmem` (:967-969).  Data only — no reference text — so that the tests pinned to these functions
(the `ref_bucketize` / `ref_alignmem` fixtures of tests/conftest.py) run in a checkout without the reference's source.

  alignmem            alignmem(x) for every x in [0, ALIGNMEM_RANGE)
  bucketize_<k>_b / _x / _want
                      Bucketize over the boundary lists and values of tests/test_oracle.py:_bucketize_cases(default_rng(5)),
                      as drawn there (test_bucketize_is_pinned_by_the_reference_itself) and padded with x[0] to the longest
                      case (test_gpu_parity.py: test_bucketize_tiers_against_the_reference_itself)

  python tests/golden/make_ref_host_goldens.py [out.npz]     (default: tests/golden/ref_host_goldens.npz)
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ALIGNMEM_RANGE = 1 << 16


def bucketize_inputs():
    """[(boundaries, values)] in the order the file stores them."""
    sys.path.insert(0, os.path.dirname(HERE))
    from test_oracle import _bucketize_cases
    cases = list(_bucketize_cases(np.random.default_rng(5)))
    n = max(len(x) for _, _, x in cases)
    out = [(b, x) for _, b, x in cases]
    out += [(b, np.concatenate([x, np.full(n - len(x), x[0], np.float32)])) for _, b, x in cases]
    return out


def main(path):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_extract
    assert ref_extract.build(), "oracle/_ref/libref_bucketize.so is not built (the reference's source is needed once)"
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_bucketize.so"))
    lib.ref_bucketize_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.ref_alignmem.argtypes = [C.c_int]
    lib.ref_alignmem.restype = C.c_int
    rec = {"alignmem": np.asarray([lib.ref_alignmem(x) for x in range(ALIGNMEM_RANGE)], np.int32)}
    for k, (b, x) in enumerate(bucketize_inputs()):
        b, x = np.ascontiguousarray(b, np.float32), np.ascontiguousarray(x, np.float32)
        want = np.empty(x.size, np.int32)
        lib.ref_bucketize_many(b.ctypes.data, int(b.size), x.ctypes.data, int(x.size), want.ctypes.data)
        rec.update({f"bucketize_{k}_b": b, f"bucketize_{k}_x": x, f"bucketize_{k}_want": want})
    np.savez_compressed(path, **rec)
    print(f"{path}: alignmem over [0, {ALIGNMEM_RANGE}), {len(bucketize_inputs())} Bucketize cases")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_host_goldens.npz"))
