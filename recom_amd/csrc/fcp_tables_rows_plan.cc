// fcp_tables_rows_plan.cc — the host-only level of the grouped rows-by-id entries: see fcp_tables_rows_plan.h.  Ordinary C++:
// nothing here touches a device or dereferences a device pointer.
#include "fcp_tables_rows_plan.h"

#include <algorithm>

namespace fcpr {

using fcpgp::refuse;

namespace {

// classes in launch order: streaming V 4, 2, 1 (group 0), then q8 V 4, 2, 1 by G 1, 2, ..., 64
constexpr int kClasses = 3 + 3 * 7;
int vec_index(int vec) { return vec == 4 ? 0 : vec == 2 ? 1 : 2; }
int class_of(int vec, int group) { return group == 0 ? vec_index(vec) : 3 + vec_index(vec) * 7 + fcpgp::log2_of(group); }

// rows of one piece: where the single-table hosts cut their launches
int64_t rows_per_piece(int group, int64_t spr) {
  return group ? kMaxLaunchThreads / group : std::max<int64_t>(1, kMaxLaunchThreads / spr); // (one row of 2^31 - 1 elements: 2^31 threads)
}

} // namespace

int check_row_args(const std::string &w, const void *table, int32_t kind, int64_t table_rows, int32_t dim, const void *row_ids,
                   const void *rows, int64_t n, std::string *why) {
  if (n < 0) return refuse(why, w + "`n` is negative");
  if (const std::string limit = fcpf::row_limit_refusal("n", n, table_rows); !limit.empty()) return refuse(why, w + limit);
  if (dim <= 0) return refuse(why, w + "`dim` must be positive");
  if (!fcpf::known_tab_kind(kind)) return refuse(why, w + "`kind` is no FCP_TAB_* value");
  if (n > 0 && !table) return refuse(why, w + "`table` is null");
  if (n > 0 && !row_ids) return refuse(why, w + "`row_ids` is null");
  if (n > 0 && !rows) return refuse(why, w + "`rows` is null");
  const int vec = fcpf::vec_of(dim);
  if ((uintptr_t)table % fcpf::base_alignment(kind, vec))
    return refuse(why, w + fcpf::not_aligned("table", fcpf::base_alignment(kind, vec), std::string(" (a ") + fcpf::kind_name(kind) + " table of this dim)"));
  if ((uintptr_t)rows % (4 * vec)) return refuse(why, w + fcpf::not_aligned("rows", 4 * vec, " (float32 rows of this dim)"));
  if ((uintptr_t)row_ids % 8) return refuse(why, w + fcpf::not_aligned("row_ids", 8));
  return FCP_OK;
}

int check_entries(const char *who, const fcp_table_rows_t *entries, int32_t n_tables, std::string *why) {
  const std::string w = std::string(who) + ": ";
  int64_t elems = 0;
  const int rc = fcpgp::check_entries(w, entries, n_tables, why, [&](int32_t k, std::string *what) {
    const fcp_table_rows_t &e = entries[k];
    const int rc = check_row_args(std::string(), e.table, e.kind, e.table_rows, e.dim, e.row_ids, e.rows, e.n, what);
    if (rc) return rc;
    if (e.reserved[0] || e.reserved[1]) return refuse(what, "`reserved` must be 0");
    elems = std::min(kMaxCallElems + 1, elems + std::min(kMaxCallElems + 1, e.n * (int64_t)e.dim)); // (n < 2^32, dim < 2^31: no overflow)
    return (int)FCP_OK;
  });
  if (rc) return rc;
  if (elems > kMaxCallElems) return refuse(why, w + "`entries` name more than 2^40 elements together (4 TiB of float32 rows)");
  return FCP_OK;
}

int check_call(const char *who, const fcp_table_rows_t *entries, int32_t n_tables, const void *skipped, const void *workspace,
               std::string *why) {
  int rc = check_entries(who, entries, n_tables, why);
  if (rc) return rc;
  const std::string w = std::string(who) + ": ";
  if ((rc = fcpgp::check_workspace(w, n_tables, workspace, why))) return rc;
  if ((uintptr_t)skipped % 8) return refuse(why, w + fcpf::not_aligned("skipped", 8));
  return FCP_OK;
}

void build_launches(const fcp_table_rows_t *entries, int32_t n_tables, bool update, int64_t *skipped, LaunchList *out) {
  out->clear(kMaxLaunchBlocks);
  auto group_of = [&](const fcp_table_rows_t &e, int vec) { return update && e.kind == FCP_TAB_Q8 ? fcpf::group_of(e.dim, vec) : 0; };
  const fcpgp::ClassSort sorted = fcpgp::sort_by_class(n_tables, kClasses, [&](int32_t k) {
    const fcp_table_rows_t &e = entries[k];
    const int vec = fcpf::vec_of(e.dim);
    return e.n <= 0 ? -1 : class_of(vec, group_of(e, vec));
  });
  out->recs.reserve(sorted.members.size() + 8);
  out->prefix.reserve(sorted.members.size() + kClasses + 8);
  for (int c = 0; c < kClasses; ++c) {
    for (int32_t m = sorted.first[c]; m < sorted.first[c + 1]; ++m) {
      const int32_t k = sorted.members[m];
      const fcp_table_rows_t &e = entries[k];
      const int vec = fcpf::vec_of(e.dim);
      const int group = group_of(e, vec);
      if (m == sorted.first[c]) out->open(Launch{vec, group, 0, 0, 0, 0});
      const int64_t spr = e.dim / vec;
      const int64_t per_piece = rows_per_piece(group, spr);
      for (int64_t r0 = 0; r0 < e.n; r0 += per_piece) {
        const int64_t rows = std::min(e.n - r0, per_piece);
        const int64_t threads = group ? rows * group : rows * spr;
        const int64_t blocks = (threads + kBlockThreads - 1) / kBlockThreads;
        Rec r;
        r.table = e.table;
        r.ids = e.row_ids + r0;
        r.rows = e.rows + r0 * e.dim;
        r.skipped = update && skipped ? skipped + k : nullptr;
        r.table_rows = (uint64_t)e.table_rows;
        r.n = (uint32_t)(group ? rows : threads);
        r.spr = (uint32_t)spr;
        r.dim = e.dim;
        r.kind = e.kind;
        r.pad = 0;
        out->add(r, (uint32_t)blocks); // (a piece alone: at most 2^23 blocks; else the launch's sum stays within 2^22)
      }
    }
    out->close();
  }
}

int64_t workspace_bytes(int32_t n_tables) {
  if (n_tables < 0 || n_tables > kMaxTables) return -1;
  const int64_t recs = n_tables + kExtraRecs;
  return 16 + recs * (int64_t)sizeof(Rec) + ((recs + kMaxLaunches) * (int64_t)sizeof(uint32_t) + 15) / 16 * 16;
}

} // namespace fcpr

extern "C" int64_t fcp_tables_rows_workspace_bytes(int32_t n_tables) { return fcpr::workspace_bytes(n_tables); }
