// plain_map_check.cc — enumerates the block mapping of the plain dense kernel (recom_amd/csrc/fcp_plain_map.h) on the
// host: every block of the grid, for span counts around the groups of eight and for several row-tile counts.
// Built and run by tests/test_plain_map_host.py.  Exit status 0: every condition holds.
//
//   even deal (deal_tiles = ntiles)   every (span, tile) pair exactly once, grid - nlist * ntiles dead blocks, a block of
//                                     a full group (and every block when nlist < 8 or nlist % 8 == 0) where the generic
//                                     mapping puts it, live blocks of any two XCDs (bid & 7) differ by at most 1
//   generic (deal_tiles = 0)          every pair exactly once, the same dead count; uneven at 118 spans x 32 tiles
//                                     (480 against 448), so the evenness condition cannot pass vacuously
#include <algorithm>
#include <cstdio>
#include <vector>

#include "fcp_plain_map.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s: ", #cond);         \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++failures;                              \
    }                                          \
  } while (0)

// the mapping as the generic dense kernel has it (locate_block, fcp_fused_bodies.h), restated
bool generic_locate(int bid, int nsp8, int nlist, int &idx, int &tile) {
  if (nsp8 > 0) {
    idx = ((bid >> 3) % nsp8) * 8 + (bid & 7);
    tile = (bid >> 3) / nsp8;
  } else {
    idx = bid % (-nsp8);
    tile = bid / (-nsp8);
  }
  return idx < nlist;
}

struct Deal {
  int live[8] = {}; // per XCD (bid & 7)
  int dead = 0;
  int spread() const { return *std::max_element(live, live + 8) - *std::min_element(live, live + 8); }
};

Deal enumerate(int nlist, int ntiles, bool even) {
  const int nsp8 = nlist >= 8 ? (nlist + 7) / 8 : -nlist; // as the plan computes it
  const int grid = (nsp8 > 0 ? 8 * nsp8 : nlist) * ntiles;
  const int full = nlist / 8 * 8;
  std::vector<int> seen((size_t)nlist * ntiles, 0);
  Deal d;
  for (int bid = 0; bid < grid; ++bid) {
    int idx = -1, tile = -1, gidx = -1, gtile = -1;
    const bool live = fcp_plain_locate(bid, nsp8, nlist, even ? ntiles : 0, idx, tile);
    const bool glive = generic_locate(bid, nsp8, nlist, gidx, gtile);
    // a block outside the partial last group maps as the generic kernel maps it (all blocks under the generic mapping)
    if (!even || nsp8 < 0 || nlist % 8 == 0 || gidx < full)
      CHECK(live == glive && (!live || (idx == gidx && tile == gtile)), "nlist %d ntiles %d even %d bid %d: (%d, %d, %d) generic (%d, %d, %d)",
            nlist, ntiles, even, bid, live, idx, tile, glive, gidx, gtile);
    if (!live) {
      ++d.dead;
      continue;
    }
    CHECK(idx >= 0 && idx < nlist && tile >= 0 && tile < ntiles, "nlist %d ntiles %d even %d bid %d: span %d tile %d", nlist, ntiles, even, bid,
          idx, tile);
    if (idx < 0 || idx >= nlist || tile < 0 || tile >= ntiles) continue;
    // the partial last group's blocks stay in that group
    if (gidx >= full) CHECK(idx >= full, "nlist %d ntiles %d even %d bid %d: span %d left the last group", nlist, ntiles, even, bid, idx);
    ++seen[(size_t)idx * ntiles + tile];
    ++d.live[bid & 7];
  }
  for (int i = 0; i < nlist * ntiles; ++i)
    CHECK(seen[i] == 1, "nlist %d ntiles %d even %d: span %d tile %d owned by %d blocks", nlist, ntiles, even, i / ntiles, i % ntiles, seen[i]);
  CHECK(d.dead == grid - nlist * ntiles, "nlist %d ntiles %d even %d: %d dead blocks of %d, want %d", nlist, ntiles, even, d.dead, grid,
        grid - nlist * ntiles);
  return d;
}

} // namespace

int main() {
  const int nlists[] = {1, 7, 8, 9, 15, 16, 17, 23, 118}, tiles[] = {1, 2, 3, 5, 32};
  for (int nlist : nlists)
    for (int ntiles : tiles) {
      const Deal e = enumerate(nlist, ntiles, true);
      // (fewer than 8 spans: bid & 7 is no XCD-to-span relation the mapping controls — the grid is not padded — but the
      // round-robin deal of nlist * ntiles consecutive live blocks is even as well)
      CHECK(e.spread() <= 1, "nlist %d ntiles %d: live blocks per XCD %d %d %d %d %d %d %d %d", nlist, ntiles, e.live[0], e.live[1], e.live[2],
            e.live[3], e.live[4], e.live[5], e.live[6], e.live[7]);
      const Deal g = enumerate(nlist, ntiles, false);
      if (nlist == 118 && ntiles == 32) {
        std::printf("118 spans x 32 tiles: even deal %d..%d live blocks per XCD, generic mapping %d..%d\n", *std::min_element(e.live, e.live + 8),
                    *std::max_element(e.live, e.live + 8), *std::min_element(g.live, g.live + 8), *std::max_element(g.live, g.live + 8));
        CHECK(*std::max_element(g.live, g.live + 8) == 480 && *std::min_element(g.live, g.live + 8) == 448 && g.spread() > 1,
              "the generic mapping is expected to be uneven here");
        CHECK(*std::max_element(e.live, e.live + 8) == 472 && *std::min_element(e.live, e.live + 8) == 472, "an even deal is 472 each");
      }
    }
  if (failures) std::printf("%d conditions failed\n", failures);
  return failures ? 1 : 0;
}
