// fcp_plain_map.h — the block mapping of the plain dense kernel (fcp_dense_plain.hip; `fcp_bench --mix-probe` runs the same
// grid), as one function the host can enumerate (tests/native/plain_map_check.cc).
//
// The grid is the generic dense kernel's: 8 * nsp8 * ntiles blocks, nsp8 = ceil(nlist / 8), every span listed in order;
// fewer than 8 spans are not padded (nsp8 = -nlist, nlist * ntiles blocks).  Blocks with equal (bid & 7) have been
// observed to land on one XCD (the hardware deals blocks round robin; nothing but speed rests on that).  A block owns one
// 64-slot span `idx` for one row tile `tile`, or is dead.
//
//   deal_tiles == 0   the generic kernel's mapping (locate_block): idx = g * 8 + (bid & 7), g = (bid >> 3) % nsp8,
//                     tile = (bid >> 3) / nsp8, dead when idx >= nlist.  The dead blocks of a partial last group
//                     (nlist % 8 = rem != 0) all have bid & 7 >= rem: XCDs rem .. 7 serve ntiles blocks fewer each.
//   deal_tiles == the grid's number of row tiles
//                     the even deal: full groups as above; the rem * ntiles (span, tile) pairs of the partial last group
//                     are numbered k = tile * 8 + (bid & 7) over that group's 8 * ntiles blocks, pair k is span
//                     F * 8 + k % rem (F = nlist / 8) at row tile k / rem, and k >= rem * ntiles is dead.  Every XCD
//                     serves floor(rem * ntiles / 8) or one more of them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FCP_PLAIN_MAP_FN __host__ __device__ inline
#else
#define FCP_PLAIN_MAP_FN inline
#endif

// What a plan (and the probe) does without FCP_DIAG=plain_even_deal=0|1 (profiles/dense_plain_even_deal_ab.txt).
constexpr int FCP_PLAIN_EVEN_DEAL_DEFAULT = 1;

// false: the block is dead
FCP_PLAIN_MAP_FN bool fcp_plain_locate(int bid, int nsp8, int nlist, int deal_tiles, int &idx, int &tile) {
  if (nsp8 > 0) {
    const int xcd = bid & 7, j8 = bid >> 3, full = nlist & ~7, rem = nlist & 7;
    idx = j8 % nsp8 * 8 + xcd;
    tile = j8 / nsp8;
    if (idx >= full && rem != 0 && deal_tiles > 0) { // a block of the partial last group
      const int k = tile * 8 + xcd;
      if (k >= rem * deal_tiles) return false;
      idx = full + k % rem;
      tile = k / rem;
      return true;
    }
  } else {
    idx = bid % (-nsp8);
    tile = bid / (-nsp8);
  }
  return idx < nlist;
}
