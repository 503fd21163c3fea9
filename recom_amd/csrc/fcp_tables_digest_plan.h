// fcp_tables_digest_plan.h — the host-only level of the grouped table digest (fcp_tables_digest, fcp_tables_digest.hip): the
// argument checks, the class rule, the deal of blocks and the launch list with its descriptor image, decided before any GPU call
// (fcp_tables_digest_plan.cc).  No GPU header: the unit is ordinary C++ and is linked, and tested under sanitizers, without the
// HIP runtime — with fcp_table_digest_host.cc beside it, whose checks of one table it takes (fcpd::check_digest /
// check_digest_rows).  fcp_table_digest.hip takes G, A and the lone grid from here, so the single-table entries and the grouped
// one class a table by one rule.
//
// Class rule, NOT folded: an entry with rows belongs to (A, G, by-id), the template parameters of the digest kernels, 4 * 7 * 2 =
// 56 classes; a call enqueues one launch per class PRESENT, in ascending class order, an upload in front and a fold behind —
// at most 58 launches whatever n_tables is, and 3 for a model of one format, one dim and one mode.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fcp_grouped_plan.h" // what the grouped entries share: constants, refusals, class sort, launch list

namespace fcpg {

using fcpgp::kBlockThreads;
using fcpgp::kMaxTables;
constexpr int kLoneBlocks = 2048;     // the most blocks of one table: 8 blocks of 256 threads on each of 256 CUs
constexpr int64_t kDealBlocks = 8192;  // the blocks of one call sum to at most kDealBlocks + n_tables
constexpr int kClasses = 4 * 7 * 2;    // A 8, 4, 2, 1 x G 1 .. 64 x by-id
constexpr int kMaxLaunches = kClasses + 2;
constexpr int kPartialBytes = 32;      // sizeof(DigestPartial), fcp_table_digest_bodies.h (asserted there where both are seen)

// G, the lanes that share a row: the largest power of two that is not above the row's words, at most 64 — a row of 9 words
// (q8, dim 64) takes 8 lanes and two words in its first lane, not 16 lanes of which 7 idle
inline int group_of_words(int64_t nw) {
  int g = 1;
  while (2 * g <= nw && g < 64) g <<= 1;
  return g;
}
// A, what is known of every row's address: the largest power of two up to 8 that divides the base and the row bytes (a q8
// table of dim % 8 == 0 at an allocation's start takes the aligned loads)
inline int align_of(const void *base, int64_t rb) {
  const uintptr_t bits = (uintptr_t)base | (uintptr_t)rb | 8u;
  return (int)(bits & (~bits + 1));
}
// the grid a table of `count` rows (by id: ids) takes alone
inline int64_t lone_blocks(int64_t count, int g) {
  const int64_t rows_per_block = kBlockThreads / g;
  return std::min<int64_t>(kLoneBlocks, (count + rows_per_block - 1) / rows_per_block);
}

// One entry with rows as the kernels see it.  64 bytes, a multiple of 16 (the upload kernel moves 16-byte words; the kernels
// read a record as four of them).
struct Rec {
  const char *base;       // the first row; by id: the table's base
  const int64_t *ids;     // null: the rows lie back to back from `base`
  uint64_t count;         // rows; by id: ids
  uint64_t table_rows;    // by id only
  uint64_t salt, row0, row_step;
  int32_t rb;             // bytes of a row
  uint32_t blocks;        // the entry's share of the launch's grid: the stride of its walk
};
static_assert(sizeof(Rec) == 64, "the descriptor image's records are 64 bytes");

// Where the fold finds entry k's partial records: `n` of them from record `first` of the partial area (n == 0: zeros).
struct Run {
  uint32_t first, n;
};
static_assert(sizeof(Run) == 8, "one run per entry, 8 bytes");

// One kernel launch (fcpgp::LaunchList): entries of ONE class.  Block b writes partial record partial_first + b.
struct Launch {
  int32_t align, group, by_id;
  uint32_t first_rec, n_recs, prefix_off, blocks, partial_first;
};

// The image: the records, the prefixes, the runs (each a 16-byte multiple)
struct LaunchList : fcpgp::LaunchList<Rec, Launch> {
  std::vector<Run> runs; // one per entry of the call, in entry order
  size_t runs_bytes() const { return (runs.size() * sizeof(Run) + 15) / 16 * 16; }
  void write_image(char *buf) const { // all three sections, their padding zeroed
    fcpgp::LaunchList<Rec, Launch>::write_image(buf);
    const size_t used = runs.size() * sizeof(Run);
    if (used) std::memcpy(buf + recs_bytes() + prefix_bytes(), runs.data(), used);
    std::memset(buf + recs_bytes() + prefix_bytes() + used, 0, runs_bytes() - used);
  }
  size_t image_bytes() const { return recs_bytes() + prefix_bytes() + runs_bytes(); }
};

// Every refusal that needs no device, in the header's order: n_tables, `entries`, the entries in ascending order (the matching
// single-table entry's checks behind "fcp_tables_digest: entry k: ", then `reserved`, then `n` without `row_ids`).
int check_entries(const fcp_table_digest_entry_t *entries, int32_t n_tables, std::string *why);
// ... then `out`, then `workspace`
int check_call(const fcp_table_digest_entry_t *entries, int32_t n_tables, const void *out, const void *workspace, std::string *why);

// The deal: blocks[k] for every entry that passed check_entries — 0 without rows, else at least 1 and at most the lone grid;
// exactly the lone grid while those sum to kDealBlocks or less, else max(1, floor(lone * kDealBlocks / sum)).  A pure
// function of the entries.
void deal_blocks(const fcp_table_digest_entry_t *entries, int32_t n_tables, std::vector<uint32_t> *blocks);

// The launch list of entries that passed check_entries: classes in ascending (by-id, A 8 4 2 1, G 1 .. 64) order, entries inside
// a class in ascending order; the partial records of the launches back to back, so an entry's run is its blocks.
void build_launches(const fcp_table_digest_entry_t *entries, int32_t n_tables, LaunchList *out);

// -1 outside [0, kMaxTables]; else a multiple of 16, increasing with n_tables: 16 bytes to bring the image to a 16-byte
// boundary, the largest image of n_tables entries, then kDealBlocks + n_tables partial records at partials_offset
int64_t partials_offset(int32_t n_tables); // from the 16-byte boundary
int64_t workspace_bytes(int32_t n_tables);

} // namespace fcpg
