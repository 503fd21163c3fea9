// fcp_tables_rows_plan.cc — the host-only level of the grouped rows-by-id entries: see fcp_tables_rows_plan.h.  Ordinary C++:
// nothing here touches a device or dereferences a device pointer.
#include "fcp_tables_rows_plan.h"

#include <algorithm>

namespace fcpr {

namespace {

int refuse(std::string *why, const std::string &msg) {
  if (why) *why = msg;
  return FCP_ERR_INVALID_ARGUMENT;
}

// classes in launch order: streaming V 4, 2, 1 (group 0), then q8 V 4, 2, 1 by G 1, 2, ..., 64
constexpr int kClasses = 3 + 3 * 7;
int vec_index(int vec) { return vec == 4 ? 0 : vec == 2 ? 1 : 2; }
int class_of(int vec, int group) {
  if (group == 0) return vec_index(vec);
  int g = 0;
  while ((1 << g) < group) ++g;
  return 3 + vec_index(vec) * 7 + g;
}

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
  if (n_tables < 0 || n_tables > kMaxTables) return refuse(why, w + "`n_tables` must lie in [0, 65536]");
  if (n_tables > 0 && !entries) return refuse(why, w + "`entries` is null");
  int64_t elems = 0;
  for (int32_t k = 0; k < n_tables; ++k) {
    const fcp_table_rows_t &e = entries[k];
    auto we = [&]() { return w + "entry " + std::to_string(k) + ": "; }; // (made for a refusal only: a model has thousands of entries)
    std::string what;
    const int rc = check_row_args(std::string(), e.table, e.kind, e.table_rows, e.dim, e.row_ids, e.rows, e.n, &what);
    if (rc) return refuse(why, we() + what);
    if (e.reserved[0] || e.reserved[1]) return refuse(why, we() + "`reserved` must be 0");
    elems = std::min(kMaxCallElems + 1, elems + std::min(kMaxCallElems + 1, e.n * (int64_t)e.dim)); // (n < 2^32, dim < 2^31: no overflow)
  }
  if (elems > kMaxCallElems) return refuse(why, w + "`entries` name more than 2^40 elements together (4 TiB of float32 rows)");
  return FCP_OK;
}

int check_call(const char *who, const fcp_table_rows_t *entries, int32_t n_tables, const void *skipped, const void *workspace,
               std::string *why) {
  const int rc = check_entries(who, entries, n_tables, why);
  if (rc) return rc;
  const std::string w = std::string(who) + ": ";
  if (n_tables > 0 && !workspace) return refuse(why, w + "`workspace` is null");
  if ((uintptr_t)workspace % 8) return refuse(why, w + fcpf::not_aligned("workspace", 8));
  if ((uintptr_t)skipped % 8) return refuse(why, w + fcpf::not_aligned("skipped", 8));
  return FCP_OK;
}

void build_launches(const fcp_table_rows_t *entries, int32_t n_tables, bool update, int64_t *skipped, LaunchList *out) {
  out->recs.clear();
  out->prefix.clear();
  out->launches.clear();
  // the classes present, and the entries of each in ascending order: a counting sort of the entries with rows by class
  int32_t first[kClasses + 1] = {};
  std::vector<int8_t> cls((size_t)std::max(n_tables, 0), -1);
  for (int32_t k = 0; k < n_tables; ++k) {
    const fcp_table_rows_t &e = entries[k];
    if (e.n <= 0) continue;
    const int vec = fcpf::vec_of(e.dim);
    const int group = update && e.kind == FCP_TAB_Q8 ? fcpf::group_of(e.dim, vec) : 0;
    cls[k] = (int8_t)class_of(vec, group);
    ++first[cls[k] + 1];
  }
  for (int c = 0; c < kClasses; ++c) first[c + 1] += first[c];
  std::vector<int32_t> members((size_t)first[kClasses]);
  {
    int32_t at[kClasses];
    std::copy(first, first + kClasses, at);
    for (int32_t k = 0; k < n_tables; ++k)
      if (cls[k] >= 0) members[at[cls[k]]++] = k;
  }
  out->recs.reserve(members.size() + 8);
  out->prefix.reserve(members.size() + kClasses + 8);
  for (int c = 0; c < kClasses; ++c) {
    if (first[c] == first[c + 1]) continue;
    Launch cur = {};
    bool open = false;
    auto close = [&]() {
      if (!open) return;
      out->prefix.push_back(cur.blocks);
      out->launches.push_back(cur);
      open = false;
    };
    for (int32_t m = first[c]; m < first[c + 1]; ++m) {
      const int32_t k = members[m];
      const fcp_table_rows_t &e = entries[k];
      const int vec = fcpf::vec_of(e.dim);
      const int group = c < 3 ? 0 : fcpf::group_of(e.dim, vec);
      const int64_t spr = e.dim / vec;
      const int64_t per_piece = rows_per_piece(group, spr);
      for (int64_t r0 = 0; r0 < e.n; r0 += per_piece) {
        const int64_t rows = std::min(e.n - r0, per_piece);
        const int64_t threads = group ? rows * group : rows * spr;
        const int64_t blocks = (threads + kBlockThreads - 1) / kBlockThreads;
        if (open && (int64_t)cur.blocks + blocks > kMaxLaunchBlocks) close();
        if (!open) {
          cur.vec = vec;
          cur.group = group;
          cur.first_rec = (uint32_t)out->recs.size();
          cur.n_recs = 0;
          cur.prefix_off = (uint32_t)out->prefix.size();
          cur.blocks = 0;
          open = true;
        }
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
        out->recs.push_back(r);
        out->prefix.push_back(cur.blocks);
        cur.blocks += (uint32_t)blocks; // (a piece alone: at most 2^23 blocks; else the sum stays within 2^22)
        ++cur.n_recs;
      }
    }
    close();
  }
}

int64_t workspace_bytes(int32_t n_tables) {
  if (n_tables < 0 || n_tables > kMaxTables) return -1;
  const int64_t recs = n_tables + kExtraRecs;
  return 16 + recs * (int64_t)sizeof(Rec) + ((recs + kMaxLaunches) * (int64_t)sizeof(uint32_t) + 15) / 16 * 16;
}

} // namespace fcpr

extern "C" int64_t fcp_tables_rows_workspace_bytes(int32_t n_tables) { return fcpr::workspace_bytes(n_tables); }
