// fcp_tables_delta_plan.cc — the host-only level of the grouped delta distinct: see fcp_tables_delta_plan.h.  Ordinary C++:
// nothing here touches a device or dereferences a device pointer.
#include "fcp_tables_delta_plan.h"

namespace fcptd {

using fcpgp::refuse;

namespace {

const char kWho[] = "fcp_tables_delta_distinct";

// a pointer the single-table checks take for `report` and `workspace`: those two are the CALL's here and are checked behind the entries
const void *const kPresent = reinterpret_cast<const void *>(uintptr_t(64));

// compact classes in launch order: ids only, then V 4, 2, 1 by G 1, 2, ..., 64
int class_of(const fcp_table_delta_entry_t &e) {
  if (!e.rows) return 0;
  const int vec = fcpf::vec_of(e.dim);
  return 1 + (vec == 4 ? 0 : vec == 2 ? 1 : 2) * 7 + fcpgp::log2_of(fcpf::group_of(e.dim, vec));
}

// the sections of the workspace behind the image, from the n values: n_of(k) is entry k's
template <class F> Layout layout_from(int32_t n_tables, F n_of) {
  int64_t recs = 0, cells = 0, flags = 0;
  for (int32_t k = 0; k < n_tables; ++k) {
    const int64_t n = n_of(k);
    if (n <= 0) continue;
    recs += partial_recs(n);
    cells += cells_for(n);
    flags += (n + 7) / 8 * 8;
  }
  Layout l;
  l.partials_off = image_room(n_tables);
  l.cells_off = l.partials_off + recs * kPartialBytes;
  l.flags_off = l.cells_off + cells * 8;
  l.end = (l.flags_off + flags + 15) / 16 * 16;
  return l;
}

} // namespace

int check_delta_args(const std::string &w, const void *row_ids, int32_t id_bytes, const float *rows, int32_t dim, int64_t n, int64_t table_rows,
                     const void *ids_out, const void *rows_out, const void *pos_out, const void *report, const void *workspace, std::string *why) {
  if (n < 0) return refuse(why, w + "`n` is negative");
  if (const std::string limit = fcpf::row_limit_refusal("n", n, table_rows); !limit.empty()) return refuse(why, w + limit);
  if (id_bytes != 4 && id_bytes != 8) return refuse(why, w + "`id_bytes` is 4 (int32 ids) or 8 (int64 ids)");
  if (rows && dim <= 0) return refuse(why, w + "`dim` must be positive");
  if (rows_out && !rows) return refuse(why, w + "`rows_out` without `rows`: ids only takes both null");
  if (rows && !rows_out) return refuse(why, w + "`rows_out` is null and `rows` is not");
  if (!report) return refuse(why, w + "`report` is null");
  if (!workspace) return refuse(why, w + "`workspace` is null");
  if (n > 0 && !row_ids) return refuse(why, w + "`row_ids` is null");
  if (n > 0 && !ids_out) return refuse(why, w + "`ids_out` is null");
  const int vec = rows ? fcpf::vec_of(dim) : 1;
  if ((uintptr_t)row_ids % (uintptr_t)id_bytes) return refuse(why, w + fcpf::not_aligned("row_ids", id_bytes));
  if ((uintptr_t)rows % (4 * vec)) return refuse(why, w + fcpf::not_aligned("rows", 4 * vec, " (float32 rows of this dim)"));
  if ((uintptr_t)ids_out % 8) return refuse(why, w + fcpf::not_aligned("ids_out", 8));
  if ((uintptr_t)rows_out % (4 * vec)) return refuse(why, w + fcpf::not_aligned("rows_out", 4 * vec, " (float32 rows of this dim)"));
  if ((uintptr_t)pos_out % 8) return refuse(why, w + fcpf::not_aligned("pos_out", 8));
  if ((uintptr_t)report % 8) return refuse(why, w + fcpf::not_aligned("report", 8));
  if ((uintptr_t)workspace % 8) return refuse(why, w + fcpf::not_aligned("workspace", 8));
  return FCP_OK;
}

int check_entries(const char *who, const fcp_table_delta_entry_t *entries, int32_t n_tables, std::string *why) {
  const std::string w = std::string(who) + ": ";
  int64_t ids = 0;
  const int rc = fcpgp::check_entries(w, entries, n_tables, why, [&](int32_t k, std::string *what) {
    const fcp_table_delta_entry_t &e = entries[k];
    const int rc = check_delta_args(std::string(), e.row_ids, e.id_bytes, e.rows, e.dim, e.n, e.table_rows, e.ids_out, e.rows_out, e.pos_out,
                                    kPresent, kPresent, what);
    if (rc) return rc;
    ids = std::min(fcpf::kRowLimit, ids + e.n); // (each n is below the limit: no overflow)
    return (int)FCP_OK;
  });
  if (rc) return rc;
  if (ids >= fcpf::kRowLimit) return refuse(why, w + "`entries` name 2^32 - 3 ids or more together");
  return FCP_OK;
}

int check_call(const fcp_table_delta_entry_t *entries, int32_t n_tables, const void *reports, const void *workspace, std::string *why) {
  const int rc = check_entries(kWho, entries, n_tables, why);
  if (rc) return rc;
  const std::string w = std::string(kWho) + ": ";
  if (n_tables > 0 && !reports) return refuse(why, w + "`reports` is null");
  if ((uintptr_t)reports % 8) return refuse(why, w + fcpf::not_aligned("reports", 8));
  return fcpgp::check_workspace(w, n_tables, workspace, why);
}

void deal_grids(const fcp_table_delta_entry_t *entries, int32_t n_tables, std::vector<Grid> *grids) {
  grids->assign((size_t)std::max(n_tables, 0), Grid{0, 0});
  int64_t sum = 0;
  for (int32_t k = 0; k < n_tables; ++k) {
    if (entries[k].n <= 0) continue;
    (*grids)[k] = grid_of(entries[k].n, kLoneBlocks);
    sum += (*grids)[k].nblocks;
  }
  if (sum <= kDealBlocks) return;
  for (int32_t k = 0; k < n_tables; ++k)
    if (const int64_t lone = (*grids)[k].nblocks) // (lone <= 1024: the product stays below 2^24)
      (*grids)[k] = grid_of(entries[k].n, std::max<int64_t>(1, lone * kDealBlocks / sum));
}

int64_t image_room(int32_t n_tables) {
  const int64_t n = n_tables;
  return n * (int64_t)sizeof(Rec) + (int64_t)LaunchList::pad16((size_t)(n + kCompactClasses) * 4) + 2 * (int64_t)LaunchList::pad16((size_t)(n + 1) * 4) +
         n * (int64_t)sizeof(Run);
}

Layout layout_of(const fcp_table_delta_entry_t *entries, int32_t n_tables) {
  return layout_from(n_tables, [&](int32_t k) { return entries[k].n; });
}

void LaunchList::write_image(char *buf) const {
  Base::write_image(buf);
  auto section = [&](size_t off, const void *src, size_t used) {
    if (used) std::memcpy(buf + off, src, used);
    std::memset(buf + off + used, 0, pad16(used) - used);
  };
  section(insert_off(), insert_prefix.data(), insert_prefix.size() * 4);
  section(classify_off(), classify_prefix.data(), classify_prefix.size() * 4);
  section(runs_off(), runs.data(), runs.size() * sizeof(Run));
}

void build_launches(const fcp_table_delta_entry_t *entries, int32_t n_tables, uintptr_t image, LaunchList *out) {
  out->clear();
  out->insert_prefix.clear();
  out->classify_prefix.clear();
  out->runs.assign((size_t)std::max(n_tables, 0), Run{0, 0, 0});
  out->blocks.assign((size_t)std::max(n_tables, 0), 0);
  out->total_cells = 0;
  std::vector<Grid> grids;
  deal_grids(entries, n_tables, &grids);
  // every entry's sections, in entry order: a function of the n values alone
  const Layout lay = layout_of(entries, n_tables);
  struct Place { int64_t first_partial, cells_off, flags_off; };
  std::vector<Place> place((size_t)std::max(n_tables, 0), Place{0, 0, 0});
  {
    int64_t recs = 0, cells = 0, flags = 0;
    for (int32_t k = 0; k < n_tables; ++k) {
      const int64_t n = entries[k].n;
      if (n <= 0) continue;
      place[k] = Place{recs, lay.cells_off + cells * 8, lay.flags_off + flags};
      out->runs[k] = Run{(uint32_t)recs, grids[k].nblocks, n};
      out->blocks[k] = grids[k].nblocks;
      recs += partial_recs(n);
      cells += cells_for(n);
      flags += (n + 7) / 8 * 8;
    }
    out->total_cells = (uint64_t)cells;
  }
  const fcpgp::ClassSort sorted = fcpgp::sort_by_class(n_tables, kCompactClasses, [&](int32_t k) { return entries[k].n <= 0 ? -1 : class_of(entries[k]); });
  out->recs.reserve(sorted.members.size());
  out->prefix.reserve(sorted.members.size() + kCompactClasses);
  out->insert_prefix.reserve(sorted.members.size() + 1);
  out->classify_prefix.reserve(sorted.members.size() + 1);
  uint32_t insert_grid = 0, classify_grid = 0;
  for (int c = 0; c < kCompactClasses; ++c) {
    if (sorted.first[c] == sorted.first[c + 1]) continue;
    const int v = c == 0 ? 0 : 4 >> ((c - 1) / 7);
    out->open(Launch{v, c == 0 ? 1 : 1 << ((c - 1) % 7), 0, 0, 0, 0});
    for (int32_t m = sorted.first[c]; m < sorted.first[c + 1]; ++m) {
      const int32_t k = sorted.members[m];
      const fcp_table_delta_entry_t &e = entries[k];
      const int64_t cells = cells_for(e.n);
      Rec r;
      r.cells = reinterpret_cast<uint32_t *>(image + (uintptr_t)place[k].cells_off);
      r.ids = e.row_ids;
      r.rows = e.rows;
      r.flags = reinterpret_cast<uint8_t *>(image + (uintptr_t)place[k].flags_off);
      r.partials = reinterpret_cast<void *>(image + (uintptr_t)(lay.partials_off + place[k].first_partial * kPartialBytes));
      r.ids_out = e.ids_out;
      r.pos_out = e.pos_out;
      r.rows_out = e.rows_out;
      r.table_rows = (uint64_t)e.table_rows;
      r.n = e.n;
      r.chunk = grids[k].chunk;
      r.shift = 64 - __builtin_ctzll((unsigned long long)cells);
      r.is64 = e.id_bytes == 8;
      r.dim = e.rows ? e.dim : 0;
      r.nblocks = grids[k].nblocks;
      r.insert_blocks = (uint32_t)std::min<int64_t>((e.n + kInsertTile - 1) / kInsertTile, kInsertMaxBlocks);
      std::fill(r.pad, r.pad + 5, 0u);
      out->insert_prefix.push_back(insert_grid);
      out->classify_prefix.push_back(classify_grid);
      insert_grid += r.insert_blocks;   // (a call: below 2^22 + n_tables, its ids staying below 2^32)
      classify_grid += r.nblocks;       // (a call: at most kDealBlocks + n_tables)
      out->add(r, r.nblocks);
    }
    out->close();
  }
  if (!out->recs.empty()) {
    out->insert_prefix.push_back(insert_grid);
    out->classify_prefix.push_back(classify_grid);
  }
}

int64_t workspace_bytes(const int64_t *n, int32_t n_tables) {
  if (n_tables < 0 || n_tables > kMaxTables || (n_tables > 0 && !n)) return -1;
  int64_t ids = 0;
  for (int32_t k = 0; k < n_tables; ++k) {
    if (n[k] < 0 || n[k] >= fcpf::kRowLimit) return -1;
    ids = std::min(fcpf::kRowLimit, ids + n[k]);
  }
  if (ids >= fcpf::kRowLimit) return -1;
  return 16 + layout_from(n_tables, [&](int32_t k) { return n[k]; }).end;
}

} // namespace fcptd

extern "C" int64_t fcp_tables_delta_workspace_bytes(const int64_t *n, int32_t n_tables) { return fcptd::workspace_bytes(n, n_tables); }
