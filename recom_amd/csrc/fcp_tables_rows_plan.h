// fcp_tables_rows_plan.h — the host-only level of the grouped rows-by-id entries (fcp_tables_update_rows /
// fcp_tables_read_rows, fcp_tables_rows.hip): the argument checks, the class rule and the launch list with its descriptor image,
// decided before any GPU call (fcp_tables_rows_plan.cc).  No GPU header: the unit is ordinary C++ and is linked, and tested
// under sanitizers, without the HIP runtime — as fcp_plan_desc.cc is.  fcp_table_rows.hip takes its argument checks from here
// too, so the single-table entries and the grouped ones refuse by one text.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "fcp_grouped_plan.h" // what the grouped entries share: constants, refusals, class sort, launch list

namespace fcpr {

using fcpgp::kBlockThreads;
using fcpgp::kMaxTables;
constexpr int64_t kMaxLaunchThreads = 1ll << 30; // per launch, as the single-table hosts chunk (fcp_table_walk.h)
constexpr int64_t kMaxLaunchBlocks = kMaxLaunchThreads / kBlockThreads;
// One call names at most 2^40 elements — 4 TiB of float32 rows, beyond any device.  The bound is what makes the workspace a
// function of n_tables alone: a PIECE (below) that does not end its entry holds more than 2^29 elements, so a call has at
// most 2^11 of them, and its launches, two consecutive ones of a class together above 2^30 threads of at most two elements
// each, at most 24 + 2^12.
constexpr int64_t kMaxCallElems = 1ll << 40;
constexpr int64_t kExtraRecs = 1 << 11;
constexpr int64_t kMaxLaunches = 24 + (1 << 12) + 8;

// One PIECE of an entry as the kernels see it: the whole entry, or — an entry of more than 2^30 threads — a run of its rows
// cut where the single-table host cuts its launches, with `ids` and `rows` at the run's first row.  64 bytes, a multiple of 16
// (the upload kernel moves 16-byte words; the kernels read a record as four of them).
struct Rec {
  void *table;              // the table's base
  const int64_t *ids;       // the piece's first id
  float *rows;              // the piece's first float32 row: source of an update, destination of a read
  int64_t *skipped;         // the entry's counter, or null
  uint64_t table_rows;
  uint32_t n;               // q8 update: rows of the piece; streaming kernels: its slots, rows * spr
  uint32_t spr;             // slots per row, dim / V
  int32_t dim, kind;
  uint64_t pad;             // 0
};
static_assert(sizeof(Rec) == 64, "the descriptor image's records are 64 bytes");

// One kernel launch (fcpgp::LaunchList): pieces of ONE class — (vec, group) for a q8 update, (vec, 0) for every other update
// and for every read.  n_recs <= kMaxTables + 1.  The image: the records, then the prefixes.
struct Launch {
  int32_t vec, group;
  uint32_t first_rec, n_recs, prefix_off, blocks;
};
using LaunchList = fcpgp::LaunchList<Rec, Launch>;

// The checks of fcp_table_update_rows / fcp_table_read_rows up to `skipped`, in their stated order; `w` goes in front of the
// message, which names the argument between backquotes.  FCP_OK, or FCP_ERR_INVALID_ARGUMENT with *why.
int check_row_args(const std::string &w, const void *table, int32_t kind, int64_t table_rows, int32_t dim, const void *row_ids,
                   const void *rows, int64_t n, std::string *why);

// Every refusal of the grouped entries that needs no device, in the header's order: n_tables, `entries`, the entries in
// ascending order (check_row_args behind "<who>: entry k: ", then `reserved`), the call's element bound, `workspace`, `skipped`.
int check_entries(const char *who, const fcp_table_rows_t *entries, int32_t n_tables, std::string *why); // (up to the element bound)
int check_call(const char *who, const fcp_table_rows_t *entries, int32_t n_tables, const void *skipped, const void *workspace,
               std::string *why);

// The launch list of entries that passed check_call.  update: q8 entries are classed by (V, G) and `skipped` (device int64
// [n_tables] or null) gives entry k the counter skipped + k; else every entry is classed by V alone.  Entries with n == 0 take
// no part.  Classes come in a fixed order (streaming V 4, 2, 1, then q8 by V and G), entries inside a class in ascending order.
void build_launches(const fcp_table_rows_t *entries, int32_t n_tables, bool update, int64_t *skipped, LaunchList *out);

// -1 outside [0, kMaxTables]; else a multiple of 16, increasing with n_tables: 16 bytes to bring the image to a 16-byte
// boundary, n_tables + kExtraRecs records, and as many prefix values plus one per launch
int64_t workspace_bytes(int32_t n_tables);

} // namespace fcpr
