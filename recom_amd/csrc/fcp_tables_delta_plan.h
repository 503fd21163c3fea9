// fcp_tables_delta_plan.h — the host-only level of the grouped delta distinct (fcp_tables_delta_distinct,
// fcp_tables_delta.hip): the argument checks, the class rule, the deal of blocks, the workspace layout and the launch list with
// its descriptor image, decided before any GPU call (fcp_tables_delta_plan.cc).  No GPU header: the unit is ordinary C++ and is
// linked, and tested under sanitizers, without the HIP runtime.  fcp_table_delta.hip takes its argument checks and cells_for
// from here, so the single-table entry and the grouped one refuse by one text and size a hash table by one rule.
//
// Launches: one upload, ONE clear, ONE insert, ONE classify, ONE fold, then one compact launch per class PRESENT — ids only, or
// the (V, G) with_compact_shape chooses for the entry's rows, 1 + 3 * 7 = 22 classes: at most 27 launches whatever n_tables is.
//
// The workspace, from its first 16-byte boundary, a function of the n values alone:
//   image      room for the largest image of n_tables entries: 128-byte records (one per entry with ids, sorted by class), the
//              compact launches' first-block tables, the insert launch's and the classify launch's, one 16-byte run per entry;
//   partials   per entry with ids, in entry order: min(1024, ceil(n / 1024)) + 1 records of 32 bytes — its blocks' (a grid never
//              has more: a chunk is at least 4 tiles and the lone grid at most 1024 blocks) and its totals;
//   cells      per entry with ids, in entry order, back to back: cells_for(n) cells of 8 bytes, so ONE clear covers them all;
//   flags      per entry with ids, in entry order: n bytes rounded up to 8.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fcp_grouped_plan.h" // what the grouped entries share: constants, refusals, class sort, launch list

namespace fcptd {

using fcpgp::kBlockThreads;
using fcpgp::kMaxTables;
// the single-table unit's geometry (fcp_table_delta.hip and fcp_tables_delta.hip assert these against their kernels' constants)
constexpr int kTile = 256;              // positions of one step of a classify / compact block
constexpr int kLoneBlocks = 1024;       // the most blocks of one entry's classify / compact grid
constexpr int kMinChunkTiles = 4;       // a block's chunk is at least this many tiles
constexpr int kInsertTile = 1024;       // positions of one step of an insert block
constexpr int kInsertMaxBlocks = 65535; // of one entry; longer deltas: the stride loop
constexpr int64_t kMinCells = 64;
constexpr int64_t kDealBlocks = 8192;   // the classify / compact blocks of one call sum to at most kDealBlocks + n_tables
constexpr int kCompactClasses = 1 + 3 * 7; // ids only, then V 4, 2, 1 x G 1 .. 64
constexpr int kFixedLaunches = 5;       // upload, clear, insert, classify, fold
constexpr int kMaxLaunches = kFixedLaunches + kCompactClasses;
constexpr int kPartialBytes = 32;       // sizeof(DeltaPartial), fcp_delta_table.h (asserted where both are seen)

// cells of the hash table of n ids: a power of two, at least 2 n and kMinCells
inline int64_t cells_for(int64_t n) {
  int64_t cells = kMinCells;
  while (cells < 2 * n) cells <<= 1;
  return cells;
}

// The classify / compact grid of n positions dealt at most max_blocks: select_grid of fcp_select_compact.h with the unit's
// smallest chunk — whole tiles, at least kMinChunkTiles of them, no empty block.
struct Grid { int64_t chunk; uint32_t nblocks; };
inline Grid grid_of(int64_t n, int64_t max_blocks) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t chunk = std::max<int64_t>(kMinChunkTiles, (tiles + max_blocks - 1) / max_blocks) * kTile;
  return Grid{chunk, (uint32_t)((n + chunk - 1) / chunk)};
}
// partial records an entry of n > 0 ids owns, whatever its share of blocks is: non-decreasing in n
inline int64_t partial_recs(int64_t n) { return std::min<int64_t>(kLoneBlocks, (n + kMinChunkTiles * kTile - 1) / (kMinChunkTiles * kTile)) + 1; }

// One entry with ids as the kernels see it.  128 bytes, a multiple of 16 (the upload kernel moves 16-byte words; the kernels
// read a record as eight of them).
struct Rec {
  uint32_t *cells;        // the entry's own hash table: 2^(64 - shift) cells {row, pos1}
  const void *ids;
  const float *rows;      // null: ids only
  uint8_t *flags;         // the entry's flag bytes
  void *partials;         // the entry's records: nblocks of its blocks, then its totals
  int64_t *ids_out, *pos_out; // pos_out may be null
  float *rows_out;
  uint64_t table_rows;
  int64_t n, chunk;       // chunk: positions of one classify / compact block
  int32_t shift, is64, dim;
  uint32_t nblocks;       // the entry's classify / compact grid
  uint32_t insert_blocks; // the entry's insert grid: the stride of its tile loop
  uint32_t pad[5];        // 0
};
static_assert(sizeof(Rec) == 128, "the descriptor image's records are 128 bytes");

// What the fold's wave of entry k finds: nblocks records from record `first` of the partial area, the totals record behind
// them; n for the report.  nblocks == 0 (n == 0): zeros into the report and nothing else.
struct Run {
  uint32_t first, nblocks;
  int64_t n;
};
static_assert(sizeof(Run) == 16, "one run per entry, 16 bytes");

// One compact launch (fcpgp::LaunchList): entries of ONE class; vec == 0: ids only.
struct Launch {
  int32_t vec, group;
  uint32_t first_rec, n_recs, prefix_off, blocks;
};

// The image: the records (sorted by class, so a compact launch's are a run of them and the insert and classify launches take
// them all), the compact launches' prefixes, the insert launch's, the classify launch's, the runs (each a 16-byte multiple).
struct LaunchList : fcpgp::LaunchList<Rec, Launch> {
  typedef fcpgp::LaunchList<Rec, Launch> Base;
  std::vector<uint32_t> insert_prefix, classify_prefix; // recs.size() + 1 values each: first blocks, then the grid
  std::vector<Run> runs;                                // one per entry of the call, in entry order
  std::vector<uint32_t> blocks;                         // every entry's classify / compact grid (0 without ids)
  uint64_t total_cells = 0;                             // of all entries: what the clear launch covers
  static size_t pad16(size_t bytes) { return (bytes + 15) / 16 * 16; }
  uint32_t insert_grid() const { return insert_prefix.empty() ? 0 : insert_prefix.back(); }
  uint32_t classify_grid() const { return classify_prefix.empty() ? 0 : classify_prefix.back(); }
  size_t insert_off() const { return recs_bytes() + prefix_bytes(); }
  size_t classify_off() const { return insert_off() + pad16(insert_prefix.size() * 4); }
  size_t runs_off() const { return classify_off() + pad16(classify_prefix.size() * 4); }
  size_t image_bytes() const { return runs_off() + pad16(runs.size() * sizeof(Run)); }
  void write_image(char *buf) const; // every section, its padding zeroed
  // launches of the call: 0 without entries, 1 when no entry has ids (the fold alone: zeros into the reports)
  int32_t n_launches() const { return runs.empty() ? 0 : recs.empty() ? 1 : kFixedLaunches + (int32_t)launches.size(); }
};

// The checks of fcp_table_delta_distinct in its stated order; `w` goes in front of the message, which names the argument
// between backquotes.  FCP_OK, or FCP_ERR_INVALID_ARGUMENT with *why.
int check_delta_args(const std::string &w, const void *row_ids, int32_t id_bytes, const float *rows, int32_t dim, int64_t n, int64_t table_rows,
                     const void *ids_out, const void *rows_out, const void *pos_out, const void *report, const void *workspace, std::string *why);

// Every refusal of the grouped entry that needs no device, in the header's order: n_tables, `entries`, the entries in ascending
// order (check_delta_args behind "<who>: entry k: ", `report` and `workspace` being the call's), the call's ids summed ...
int check_entries(const char *who, const fcp_table_delta_entry_t *entries, int32_t n_tables, std::string *why);
// ... then `reports`, then `workspace`
int check_call(const fcp_table_delta_entry_t *entries, int32_t n_tables, const void *reports, const void *workspace, std::string *why);

// The deal: every entry's classify / compact grid — 0 without ids, else grid_of(n, share): share the lone grid's blocks while
// those sum to kDealBlocks or less, else max(1, floor(lone * kDealBlocks / sum)).  A pure function of the n values.
void deal_grids(const fcp_table_delta_entry_t *entries, int32_t n_tables, std::vector<Grid> *grids);

// Where the workspace's sections lie, from its first 16-byte boundary (the header comment)
int64_t image_room(int32_t n_tables);
struct Layout { int64_t partials_off, cells_off, flags_off, end; };
Layout layout_of(const fcp_table_delta_entry_t *entries, int32_t n_tables);

// The launch list of entries that passed check_entries.  image: the workspace's first 16-byte boundary (0: the records' device
// pointers into the workspace mean nothing, as for fcp_tables_delta_launches).  Compact classes in ascending (ids only, V 4 2 1,
// G 1 .. 64) order, entries inside a class in ascending order.
void build_launches(const fcp_table_delta_entry_t *entries, int32_t n_tables, uintptr_t image, LaunchList *out);

// -1 for an invalid argument (n_tables outside [0, kMaxTables], a null n with n_tables > 0, an n[k] that is negative or beyond
// the row limit, or a sum beyond it); else a multiple of 16: 16 bytes to reach the boundary, then the layout's end
int64_t workspace_bytes(const int64_t *n, int32_t n_tables);

} // namespace fcptd
