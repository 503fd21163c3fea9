// grouped_image_check.h — what the kernels of every grouped table entry rely on in a launch list (fcpgp::LaunchList,
// recom_amd/csrc/fcp_grouped_plan.h), checked in ONE place for the sanitizer programs (tables_rows_plan_san.cc,
// tables_digest_plan_san.cc, grouped_plan_san.cc): the launches lie back to back; a launch holds 1 to 65537 records; its
// first-block table starts at 0, ascends strictly and ends at the grid, which is `blocks`; nothing is left over; the image fits
// the workspace behind the 16 bytes that align it.  The includer defines EXPECT first and keeps its own checks:
// on_launch(launch) in front of a launch's records; blocks_of(launch, rec, first) -> the record's blocks, `first` its first block.
#pragma once
#include <cstddef>
#include <cstdint>

template <class List, class OnLaunch, class BlocksOf>
void check_launch_list(const List &L, int64_t image_bytes, int64_t workspace_bytes, int set, OnLaunch on_launch, BlocksOf blocks_of) {
  EXPECT(16 + image_bytes <= workspace_bytes, "set %d: the image outgrows the workspace", set);
  size_t rec = 0, pre = 0;
  for (const auto &l : L.launches) {
    EXPECT(l.first_rec == rec && l.prefix_off == pre, "set %d: launches are not back to back", set);
    EXPECT(l.n_recs >= 1 && l.n_recs <= 65537u, "set %d: %u records in a launch", set, l.n_recs);
    on_launch(l);
    uint32_t first = 0;
    for (uint32_t j = 0; j < l.n_recs; ++j) {
      EXPECT(L.prefix[pre + j] == first, "set %d: prefix[%u] = %u, want %u", set, j, L.prefix[pre + j], first);
      const uint32_t blocks = blocks_of(l, L.recs[rec + j], first);
      EXPECT(blocks >= 1, "set %d: record %u of a launch without a block", set, j);
      first += blocks;
    }
    EXPECT(L.prefix[pre + l.n_recs] == first && l.blocks == first, "set %d: grid %u, records sum to %u", set, l.blocks, first);
    rec += l.n_recs;
    pre += l.n_recs + 1;
  }
  EXPECT(rec == L.recs.size() && pre == L.prefix.size(), "set %d: records left over", set);
}
