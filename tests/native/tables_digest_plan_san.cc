// tables_digest_plan_san.cc — the host-only level of the grouped table digest (recom_amd/csrc/fcp_tables_digest_plan.cc, with
// the host half of the single-table digest whose checks it takes, fcp_table_digest_host.cc) on its own, for a build with
// -fsanitize=address,undefined: the units need no GPU runtime and no other unit of the library.
//   tables_digest_plan_san SEED SETS
// Drives the launch-list builder over SETS random entry lists — every kind, dims of every G, every alignment the kind allows,
// both modes, empty entries, entries beyond the fixed grid (their pointers are numbers: nothing is dereferenced) — and checks,
// per list, what the kernels rely on: the launch list's own promises (grouped_image_check.h: first-block tables from 0, strictly
// ascending, ending at the grid); a launch holds entries of ONE class, in ascending order; the records say what the entries say; the launches' partial records lie
// back to back, every entry's run is exactly its blocks inside its launch's, no two runs meet, and all of them lie inside the
// partial area of the workspace of n_tables; the image ends in front of that area.  Then the deal's promises and the
// refusals, in order.  Prints `<n> sets` and `<n> failures`.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "fcp_table_digest.h"
#include "fcp_tables_digest_plan.h"

static int failures = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      ++failures;                    \
      std::printf("%s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);      \
      std::printf("\n");             \
    }                                \
  } while (0)
#include "grouped_image_check.h" // check_launch_list: what both grouped entries' kernels rely on (needs EXPECT)

static const uintptr_t A = uintptr_t(1) << 40; // aligned for everything

static fcp_table_digest_entry_t entry(int kind, int dim, int64_t count, bool by_id, uintptr_t off, int k) {
  fcp_table_digest_entry_t e = {};
  e.table = reinterpret_cast<const void *>(A + (uintptr_t)k * 4096 + off);
  e.row_ids = by_id ? reinterpret_cast<const int64_t *>((uintptr_t(1) << 50) + ((uintptr_t)k << 36)) : nullptr;
  e.rows = by_id ? 1 + count / 2 : count; // (by id: table_rows, smaller than the ids)
  e.n = by_id ? count : 0;
  e.row0 = k;
  e.row_step = 1 + k % 3;
  e.kind = kind;
  e.dim = dim;
  return e;
}

static int64_t count_of(const fcp_table_digest_entry_t &e) { return e.row_ids ? e.n : e.rows; }

static void check_set(const std::vector<fcp_table_digest_entry_t> &es, int set) {
  const int32_t n_tables = (int32_t)es.size();
  std::string why;
  const int rc = fcpg::check_call(es.data(), n_tables, reinterpret_cast<void *>(4 * A), reinterpret_cast<void *>(5 * A), &why);
  EXPECT(rc == FCP_OK && why.empty(), "set %d: refused: %s", set, why.c_str());
  if (rc) return;
  fcpg::LaunchList L;
  fcpg::build_launches(es.data(), n_tables, &L);
  std::vector<uint32_t> blocks;
  fcpg::deal_blocks(es.data(), n_tables, &blocks);
  // the deal
  int64_t sum = 0, lone_sum = 0;
  for (int k = 0; k < n_tables; ++k) {
    const int64_t count = count_of(es[k]);
    const int64_t lone = count > 0 ? fcpg::lone_blocks(count, fcpg::group_of_words((fcpf::row_bytes(es[k].kind, es[k].dim) + 7) / 8)) : 0;
    EXPECT((blocks[k] >= 1) == (count > 0) && blocks[k] <= lone, "set %d: entry %d: %u blocks, alone %" PRId64, set, k, blocks[k], lone);
    sum += blocks[k];
    lone_sum += lone;
  }
  EXPECT(sum <= fcpg::kDealBlocks + n_tables, "set %d: %" PRId64 " blocks", set, sum);
  if (lone_sum <= fcpg::kDealBlocks) EXPECT(sum == lone_sum, "set %d: lone grids that fit were scaled", set);
  // the image and the workspace
  const int64_t partials_off = fcpg::partials_offset(n_tables);
  EXPECT((int64_t)L.image_bytes() <= partials_off && partials_off % 16 == 0, "set %d: the image reaches the partial records", set);
  EXPECT(16 + partials_off + (fcpg::kDealBlocks + n_tables) * (int64_t)fcpg::kPartialBytes == fcpg::workspace_bytes(n_tables), "set %d: workspace", set);
  EXPECT((int)L.launches.size() <= fcpg::kClasses && (int64_t)L.runs.size() == n_tables, "set %d: %zu launches", set, L.launches.size());
  std::vector<int> seen((size_t)n_tables, 0);
  uint32_t partial = 0, next_partial = 0; // the launch's first partial record, the next launch's
  int last_class = -1, last_k = -1;
  check_launch_list(
      L, (int64_t)L.image_bytes(), fcpg::workspace_bytes(n_tables), set,
      [&](const fcpg::Launch &l) {
        partial = next_partial;
        next_partial += l.blocks;
        last_k = -1;
        EXPECT(l.partial_first == partial, "set %d: partial records are not back to back", set);
        EXPECT(l.n_recs <= (uint32_t)fcpg::kMaxTables, "set %d: %u entries in a launch", set, l.n_recs);
        const int cls = (l.by_id * 4 + (l.align == 8 ? 0 : l.align == 4 ? 1 : l.align == 2 ? 2 : 3)) * 128 + l.group;
        EXPECT(cls > last_class, "set %d: classes out of order", set);
        last_class = cls;
      },
      [&](const fcpg::Launch &l, const fcpg::Rec &r, uint32_t first) {
        // which entry: the one whose run starts here
        int k = -1;
        for (int c = last_k + 1; c < n_tables && k < 0; ++c)
          if (L.runs[c].n && L.runs[c].first == partial + first) k = c;
        EXPECT(k >= 0, "set %d: a record without an entry", set);
        if (k < 0) return r.blocks;
        last_k = k;
        ++seen[k];
        const fcp_table_digest_entry_t &e = es[k];
        const int64_t rb = fcpf::row_bytes(e.kind, e.dim);
        EXPECT(l.align == fcpg::align_of(e.table, rb) && l.group == fcpg::group_of_words((rb + 7) / 8) && (l.by_id != 0) == (e.row_ids != nullptr),
               "set %d: entry %d in a launch of class (%d, %d, %d)", set, k, l.align, l.group, l.by_id);
        EXPECT((uintptr_t)e.table % l.align == 0 && rb % l.align == 0, "set %d: entry %d: loads of %d bytes", set, k, l.align);
        EXPECT(r.base == e.table && r.ids == e.row_ids && r.count == (uint64_t)count_of(e) && r.table_rows == (e.row_ids ? (uint64_t)e.rows : 0) &&
                   r.salt == fcpd::salt_of(e.kind, e.dim) && r.row0 == (uint64_t)e.row0 && r.row_step == (uint64_t)e.row_step && r.rb == rb &&
                   r.blocks == blocks[k] && L.runs[k].n == blocks[k],
               "set %d: entry %d: record", set, k);
        return r.blocks;
      });
  partial = next_partial;
  EXPECT((int64_t)partial == sum && (int64_t)partial <= fcpg::kDealBlocks + n_tables, "set %d: %u partial records", set, partial);
  // runs: disjoint, inside the area
  std::vector<std::pair<uint32_t, uint32_t>> runs;
  for (int k = 0; k < n_tables; ++k) {
    EXPECT(seen[k] == (count_of(es[k]) > 0 ? 1 : 0), "set %d: entry %d has %d records", set, k, seen[k]);
    if (L.runs[k].n) runs.push_back({L.runs[k].first, L.runs[k].n});
    else EXPECT(blocks[k] == 0, "set %d: entry %d: rows without a run", set, k);
  }
  std::sort(runs.begin(), runs.end());
  uint32_t end = 0;
  for (const auto &r : runs) {
    EXPECT(r.first >= end, "set %d: runs meet at %u", set, r.first);
    end = r.first + r.second;
  }
  EXPECT(end <= partial, "set %d: a run leaves the partial records", set);
  // the image as the upload moves it: the three sections, the padding of the last two zeros, not a byte behind it
  std::vector<unsigned char> image(L.image_bytes() + 1, 0x5a), want(L.image_bytes() + 1, 0);
  want.back() = 0x5a;
  if (!L.recs.empty()) std::memcpy(want.data(), L.recs.data(), L.recs_bytes());
  if (!L.prefix.empty()) std::memcpy(want.data() + L.recs_bytes(), L.prefix.data(), L.prefix.size() * 4);
  if (!L.runs.empty()) std::memcpy(want.data() + L.recs_bytes() + L.prefix_bytes(), L.runs.data(), L.runs.size() * sizeof(fcpg::Run));
  L.write_image(reinterpret_cast<char *>(image.data()));
  EXPECT(image == want, "set %d: the image's bytes", set);
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: tables_digest_plan_san SEED SETS\n");
    return 2;
  }
  std::mt19937_64 rng(std::strtoull(argv[1], nullptr, 10));
  const int sets = std::atoi(argv[2]);
  const int dims[] = {1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 31, 32, 33, 64, 68, 128, 129, 252, 256, 260, 300, 1000, 1001, 514};
  const int64_t counts[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 5000, 100000, 600000, (1ll << 31), (1ll << 32) - 4};
  for (int s = 0; s < sets; ++s) {
    const int shape = s % 4; // 0: a few entries; 1: many small; 2: one large among small; 3: several large
    const int n_tables = shape == 1 ? 1 + (int)(rng() % 3000) : (int)(rng() % 40);
    std::vector<fcp_table_digest_entry_t> es;
    for (int k = 0; k < n_tables; ++k) {
      const int kind = (int)(rng() % 4), dim = dims[rng() % (sizeof(dims) / sizeof(dims[0]))];
      int64_t count = (int64_t)(rng() % 5 == 0 ? 0 : 1 + rng() % 600);
      if ((shape == 2 && k == n_tables / 2) || (shape == 3 && rng() % 2 == 0) || shape == 0) count = counts[rng() % (sizeof(counts) / sizeof(counts[0]))];
      const uintptr_t unit = (uintptr_t)fcpd::row_alignment(kind, dim);
      es.push_back(entry(kind, dim, count, rng() % 2 == 0, unit * (rng() % 16), k));
    }
    check_set(es, s);
  }
  // the most entries, each beyond the fixed grid: one block each
  {
    std::vector<fcp_table_digest_entry_t> es;
    for (int k = 0; k < fcpg::kMaxTables; ++k) es.push_back(entry(k % 4, dims[k % 24], 1 << 22, k % 3 == 0, 0, k));
    check_set(es, -1);
    std::vector<uint32_t> blocks;
    fcpg::deal_blocks(es.data(), (int32_t)es.size(), &blocks);
    EXPECT(*std::max_element(blocks.begin(), blocks.end()) == 1, "65536 large entries: more than one block each");
  }
  // a single entry takes the lone grid
  for (int64_t count : counts) {
    std::vector<fcp_table_digest_entry_t> es = {entry(1, 16, count, false, 0, 0)};
    std::vector<uint32_t> blocks;
    fcpg::deal_blocks(es.data(), 1, &blocks);
    EXPECT(blocks[0] == (uint32_t)(count ? fcpg::lone_blocks(count, 4) : 0), "one entry of %" PRId64 " rows: %u blocks", count, blocks[0]);
    check_set(es, -2);
  }

  // the refusals, in order
  std::string why;
  void *O = reinterpret_cast<void *>(4 * A), *W = reinterpret_cast<void *>(5 * A);
  std::vector<fcp_table_digest_entry_t> es = {entry(3, 64, 5, false, 0, 0), entry(1, 62, 0, true, 0, 1), entry(0, 61, 9, true, 0, 2)};
  auto refused = [&](const char *word, const void *out, const void *ws, int32_t n = 3) {
    why.clear();
    const int rc = fcpg::check_call(es.data(), n, out, ws, &why);
    EXPECT(rc == FCP_ERR_INVALID_ARGUMENT && why.find(word) != std::string::npos && why.rfind("fcp_tables_digest: ", 0) == 0, "want %s, got %d: %s", word, rc,
           why.c_str());
  };
  refused("`n_tables`", O, W, -1);
  refused("`n_tables`", O, W, 65537);
  why.clear();
  EXPECT(fcpg::check_call(nullptr, 2, O, W, &why) == FCP_ERR_INVALID_ARGUMENT && why.find("`entries`") != std::string::npos, "null entries: %s", why.c_str());
  EXPECT(fcpg::check_call(nullptr, 0, nullptr, nullptr, &why) == FCP_OK, "no entries refused");
  es[2].dim = 0;
  es[1].n = -1;
  refused("entry 1: `n`", nullptr, nullptr); // the first bad entry wins, and wins over out and the workspace
  es[1].n = 0;
  refused("entry 2: `dim`", nullptr, nullptr);
  es[2].dim = 61;
  es[2].reserved = 1;
  es[2].table = reinterpret_cast<const void *>(A + 2); // a misaligned table comes before reserved
  refused("entry 2: `table`", nullptr, nullptr);
  es[2].table = reinterpret_cast<const void *>(A);
  refused("entry 2: `reserved`", nullptr, nullptr);
  es[2].reserved = 0;
  es[0].n = 4; // ids without row_ids
  refused("entry 0: `n`", nullptr, nullptr);
  es[0].n = 0;
  es[0].rows = es[2].n = es[2].rows = (1ll << 32) - 4; // the last values below the limits
  why.clear();
  EXPECT(fcpg::check_call(es.data(), 3, O, W, &why) == FCP_OK, "%s", why.c_str());
  es[0].rows = 5;
  refused("`out`", nullptr, nullptr);
  refused("`out`", reinterpret_cast<void *>(4 * A + 4), nullptr);
  refused("`workspace`", O, nullptr);
  refused("`workspace`", O, reinterpret_cast<void *>(5 * A + 4));
  EXPECT(fcpg::workspace_bytes(-1) == -1 && fcpg::workspace_bytes(65537) == -1 && fcpg::workspace_bytes(0) > 0, "workspace range");
  for (int n = 0; n < 65536; n += 257)
    EXPECT(fcpg::workspace_bytes(n) % 8 == 0 && fcpg::workspace_bytes(n) <= fcpg::workspace_bytes(n + 1), "workspace at %d", n);

  std::printf("%d sets\n%d failures\n", sets, failures);
  return failures ? 1 : 0;
}
