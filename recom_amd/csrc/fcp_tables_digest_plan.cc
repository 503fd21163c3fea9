// fcp_tables_digest_plan.cc — the host-only level of the grouped table digest: see fcp_tables_digest_plan.h.  Ordinary C++:
// nothing here touches a device or dereferences a device pointer.
#include "fcp_tables_digest_plan.h"

#include "fcp_table_digest.h"

namespace fcpg {

namespace {

const char kWho[] = "fcp_tables_digest: ";

int refuse(std::string *why, const std::string &msg) {
  if (why) *why = msg;
  return FCP_ERR_INVALID_ARGUMENT;
}

// what the entry sums over: rows back to back, or ids
int64_t count_of(const fcp_table_digest_entry_t &e) { return e.row_ids ? e.n : e.rows; }

int log2_of(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
// classes in launch order: back to back before by id, A 8, 4, 2, 1, G 1, 2, ..., 64
int class_of(int align, int group, bool by_id) { return ((by_id ? 4 : 0) + (3 - log2_of(align))) * 7 + log2_of(group); }

// a pointer the single-table checks take for `out` and `workspace`: those two are the CALL's here and are checked behind the entries
const void *const kPresent = reinterpret_cast<const void *>(uintptr_t(64));

} // namespace

int check_entries(const fcp_table_digest_entry_t *entries, int32_t n_tables, std::string *why) {
  const std::string w = kWho;
  if (n_tables < 0 || n_tables > kMaxTables) return refuse(why, w + "`n_tables` must lie in [0, 65536]");
  if (n_tables > 0 && !entries) return refuse(why, w + "`entries` is null");
  for (int32_t k = 0; k < n_tables; ++k) {
    const fcp_table_digest_entry_t &e = entries[k];
    auto we = [&]() { return w + "entry " + std::to_string(k) + ": "; }; // (made for a refusal only: a model has thousands of entries)
    std::string what;
    const int rc = e.row_ids ? fcpd::check_digest_rows(std::string(), e.table, e.kind, e.rows, e.dim, e.row0, e.row_step, e.row_ids, e.n, kPresent, kPresent, &what)
                             : fcpd::check_digest(std::string(), e.table, e.kind, e.rows, e.dim, e.row0, e.row_step, kPresent, kPresent, &what);
    if (rc) return refuse(why, we() + what);
    if (e.reserved) return refuse(why, we() + "`reserved` must be 0");
    if (!e.row_ids && e.n != 0) return refuse(why, we() + "`n` must be 0 where `row_ids` is null");
  }
  return FCP_OK;
}

int check_call(const fcp_table_digest_entry_t *entries, int32_t n_tables, const void *out, const void *workspace, std::string *why) {
  const int rc = check_entries(entries, n_tables, why);
  if (rc) return rc;
  const std::string w = kWho;
  if (n_tables > 0 && !out) return refuse(why, w + "`out` is null");
  if ((uintptr_t)out % 8) return refuse(why, w + fcpf::not_aligned("out", 8));
  if (n_tables > 0 && !workspace) return refuse(why, w + "`workspace` is null");
  if ((uintptr_t)workspace % 8) return refuse(why, w + fcpf::not_aligned("workspace", 8));
  return FCP_OK;
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
  out->recs.clear();
  out->prefix.clear();
  out->launches.clear();
  out->runs.assign((size_t)std::max(n_tables, 0), Run{0, 0});
  std::vector<uint32_t> blocks;
  deal_blocks(entries, n_tables, &blocks);
  // the classes present, and the entries of each in ascending order: a counting sort of the entries with rows by class
  int32_t first[kClasses + 1] = {};
  std::vector<int8_t> cls((size_t)std::max(n_tables, 0), -1);
  for (int32_t k = 0; k < n_tables; ++k) {
    if (!blocks[k]) continue;
    const fcp_table_digest_entry_t &e = entries[k];
    const int64_t rb = fcpf::row_bytes(e.kind, e.dim);
    cls[k] = (int8_t)class_of(align_of(e.table, rb), group_of_words((rb + 7) / 8), e.row_ids != nullptr);
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
  out->recs.reserve(members.size());
  out->prefix.reserve(members.size() + kClasses);
  uint32_t partial = 0; // partial records handed out so far
  for (int c = 0; c < kClasses; ++c) {
    if (first[c] == first[c + 1]) continue;
    Launch l = {};
    l.by_id = c / 28;
    l.align = 8 >> (c / 7 % 4);
    l.group = 1 << (c % 7);
    l.first_rec = (uint32_t)out->recs.size();
    l.prefix_off = (uint32_t)out->prefix.size();
    l.partial_first = partial;
    for (int32_t m = first[c]; m < first[c + 1]; ++m) {
      const int32_t k = members[m];
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
      out->recs.push_back(r);
      out->prefix.push_back(l.blocks);
      out->runs[k] = Run{partial + l.blocks, blocks[k]};
      l.blocks += blocks[k]; // (a call: at most kDealBlocks + n_tables)
      ++l.n_recs;
    }
    out->prefix.push_back(l.blocks);
    partial += l.blocks;
    out->launches.push_back(l);
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
