// fcp_tables_digest_plan.cc — the host-only level of the grouped table digest: see fcp_tables_digest_plan.h.  Ordinary C++:
// nothing here touches a device or dereferences a device pointer.
#include "fcp_tables_digest_plan.h"

#include "fcp_table_digest.h"

namespace fcpg {

using fcpgp::log2_of;
using fcpgp::refuse;

namespace {

const char kWho[] = "fcp_tables_digest: ";

// what the entry sums over: rows back to back, or ids
int64_t count_of(const fcp_table_digest_entry_t &e) { return e.row_ids ? e.n : e.rows; }

// classes in launch order: back to back before by id, A 8, 4, 2, 1, G 1, 2, ..., 64
int class_of(int align, int group, bool by_id) { return ((by_id ? 4 : 0) + (3 - log2_of(align))) * 7 + log2_of(group); }

// a pointer the single-table checks take for `out` and `workspace`: those two are the CALL's here and are checked behind the entries
const void *const kPresent = reinterpret_cast<const void *>(uintptr_t(64));

} // namespace

int check_entries(const fcp_table_digest_entry_t *entries, int32_t n_tables, std::string *why) {
  return fcpgp::check_entries(kWho, entries, n_tables, why, [&](int32_t k, std::string *what) {
    const fcp_table_digest_entry_t &e = entries[k];
    const int rc = e.row_ids ? fcpd::check_digest_rows(std::string(), e.table, e.kind, e.rows, e.dim, e.row0, e.row_step, e.row_ids, e.n, kPresent, kPresent, what)
                             : fcpd::check_digest(std::string(), e.table, e.kind, e.rows, e.dim, e.row0, e.row_step, kPresent, kPresent, what);
    if (rc) return rc;
    if (e.reserved) return refuse(what, "`reserved` must be 0");
    if (!e.row_ids && e.n != 0) return refuse(what, "`n` must be 0 where `row_ids` is null");
    return (int)FCP_OK;
  });
}

int check_call(const fcp_table_digest_entry_t *entries, int32_t n_tables, const void *out, const void *workspace, std::string *why) {
  const int rc = check_entries(entries, n_tables, why);
  if (rc) return rc;
  const std::string w = kWho;
  if (n_tables > 0 && !out) return refuse(why, w + "`out` is null");
  if ((uintptr_t)out % 8) return refuse(why, w + fcpf::not_aligned("out", 8));
  return fcpgp::check_workspace(w, n_tables, workspace, why);
}

void deal_blocks(const fcp_table_digest_entry_t *entries, int32_t n_tables, std::vector<uint32_t> *blocks) {
  blocks->assign((size_t)std::max(n_tables, 0), 0);
  int64_t sum = 0;
  for (int32_t k = 0; k < n_tables; ++k) {
    const fcp_table_digest_entry_t &e = entries[k];
    const int64_t count = count_of(e);
    if (count <= 0) continue;
    const int g = group_of_words((fcpf::row_bytes(e.kind, e.dim) + 7) / 8);
    (*blocks)[k] = (uint32_t)lone_blocks(count, g);
    sum += (*blocks)[k];
  }
  if (sum <= kDealBlocks) return;
  for (uint32_t &b : *blocks)
    if (b) b = (uint32_t)std::max<int64_t>(1, (int64_t)b * kDealBlocks / sum); // (b <= 2048: the product stays below 2^24)
}

void build_launches(const fcp_table_digest_entry_t *entries, int32_t n_tables, LaunchList *out) {
  out->clear();
  out->runs.assign((size_t)std::max(n_tables, 0), Run{0, 0});
  std::vector<uint32_t> blocks;
  deal_blocks(entries, n_tables, &blocks);
  const fcpgp::ClassSort sorted = fcpgp::sort_by_class(n_tables, kClasses, [&](int32_t k) {
    const fcp_table_digest_entry_t &e = entries[k];
    const int64_t rb = fcpf::row_bytes(e.kind, e.dim);
    return blocks[k] ? class_of(align_of(e.table, rb), group_of_words((rb + 7) / 8), e.row_ids != nullptr) : -1;
  });
  out->recs.reserve(sorted.members.size());
  out->prefix.reserve(sorted.members.size() + kClasses);
  uint32_t partial = 0; // partial records handed out so far
  for (int c = 0; c < kClasses; ++c) {
    if (sorted.first[c] == sorted.first[c + 1]) continue;
    out->open(Launch{8 >> (c / 7 % 4), 1 << (c % 7), c / 28, 0, 0, 0, 0, partial});
    for (int32_t m = sorted.first[c]; m < sorted.first[c + 1]; ++m) {
      const int32_t k = sorted.members[m];
      const fcp_table_digest_entry_t &e = entries[k];
      Rec r;
      r.base = static_cast<const char *>(e.table);
      r.ids = e.row_ids;
      r.count = (uint64_t)count_of(e);
      r.table_rows = e.row_ids ? (uint64_t)e.rows : 0;
      r.salt = fcpd::salt_of(e.kind, e.dim);
      r.row0 = (uint64_t)e.row0;
      r.row_step = (uint64_t)e.row_step;
      r.rb = (int32_t)fcpf::row_bytes(e.kind, e.dim); // (below 2^31: the argument checks)
      r.blocks = blocks[k];
      out->runs[k] = Run{partial + out->open_blocks(), blocks[k]};
      out->add(r, blocks[k]); // (a call: at most kDealBlocks + n_tables)
    }
    partial += out->open_blocks();
    out->close();
  }
}

int64_t partials_offset(int32_t n_tables) {
  const int64_t n = n_tables;
  return n * (int64_t)sizeof(Rec) + ((n + kClasses) * (int64_t)sizeof(uint32_t) + 15) / 16 * 16 + (n * (int64_t)sizeof(Run) + 15) / 16 * 16;
}

int64_t workspace_bytes(int32_t n_tables) {
  if (n_tables < 0 || n_tables > kMaxTables) return -1;
  return 16 + partials_offset(n_tables) + (kDealBlocks + n_tables) * (int64_t)kPartialBytes;
}

} // namespace fcpg

extern "C" int64_t fcp_tables_digest_workspace_bytes(int32_t n_tables) { return fcpg::workspace_bytes(n_tables); }
