// fcp_find_piece.h — the front of the grouped table kernels, written ONCE for fcp_tables_rows.hip and fcp_tables_digest.hip: a
// launch serves many entries, each with a run of the grid's blocks, and block b finds its entry j, prefix[j] <= b <
// prefix[j + 1], by a binary search from blockIdx.x alone.  The table and the records are read through the constant address
// space, so the search and the record are scalar loads into SGPRs and every lane of the block agrees on the entry by
// construction.  Unnamed namespace, as in fcp_table_walk.h.
#pragma once
#include "fcp_fused_bodies.h"

namespace {

constexpr int kSearchSteps = 17; // ceil(log2(65536 + 1)): the most records of one launch

// The piece block b of this launch belongs to, and b's index inside it.  prefix: n_recs + 1 ascending values, prefix[0] == 0,
// prefix[n_recs] == gridDim.x; no two equal (a piece has rows, so blocks).  Scalar throughout: b is blockIdx.x.
template <class R> __device__ __forceinline__ R find_piece(const R *recs, const uint32_t *prefix, uint32_t n_recs, uint32_t b, uint32_t *local) {
  const FCP_CONST uint32_t *p = as_const(prefix);
  uint32_t lo = 0, hi = n_recs, first = 0; // prefix[lo] == first <= b < prefix[hi]
#pragma unroll 1
  for (int step = 0; step < kSearchSteps && hi - lo > 1; ++step) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t v = p[mid];
    if (v <= b) {
      lo = mid;
      first = v;
    } else {
      hi = mid;
    }
  }
  *local = b - first;
  return ld_rec(as_const(recs) + lo);
}

} // namespace
