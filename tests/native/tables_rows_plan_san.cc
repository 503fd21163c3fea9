// tables_rows_plan_san.cc — the host-only level of the grouped rows-by-id entries (recom_amd/csrc/fcp_tables_rows_plan.cc) on
// its own, for a build with -fsanitize=address,undefined: the unit needs no GPU runtime and no other unit of the library.
//   tables_rows_plan_san SEED SETS
// Drives the launch-list builder over SETS random entry sets — every kind, dims of every V and G, empty entries, entries of
// more than 2^30 threads (their pointers are numbers: nothing is dereferenced) — and checks, per set, what the kernels rely on:
// the launch list's own promises (grouped_image_check.h: first-block tables from 0, strictly ascending, ending at the grid; at
// most 65537 pieces in a launch); the grid is the sum of its pieces' blocks and stays within 2^22 unless the launch is one
// piece; a launch holds pieces of ONE class; the pieces of
// an entry tile its rows exactly, in order, with ids / rows / skipped pointing where the single-table host would point; the
// image fits the workspace of n_tables.  Then the refusals, in order.  Prints `<n> sets` and `<n> failures`.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "fcp_tables_rows_plan.h"

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

// (the ids of entry k lie 2^36 bytes behind those of entry k - 1: no two entries' id ranges meet, whatever n is)
static fcp_table_rows_t entry(int kind, int dim, int64_t n, int64_t table_rows, int k) {
  fcp_table_rows_t e = {};
  e.table = reinterpret_cast<void *>(A + (uintptr_t)k * 4096);
  e.row_ids = reinterpret_cast<const int64_t *>((uintptr_t(1) << 50) + ((uintptr_t)k << 36));
  e.rows = reinterpret_cast<float *>((uintptr_t(1) << 52) + (uintptr_t)k * 4096);
  e.table_rows = table_rows;
  e.n = n;
  e.kind = kind;
  e.dim = dim;
  return e;
}

static void check_set(const std::vector<fcp_table_rows_t> &es, bool update, int set) {
  const int32_t n_tables = (int32_t)es.size();
  std::string why;
  int64_t *skipped = update ? reinterpret_cast<int64_t *>(4 * A) : nullptr;
  const int rc = fcpr::check_call("who", es.data(), n_tables, skipped, reinterpret_cast<void *>(5 * A), &why);
  EXPECT(rc == FCP_OK && why.empty(), "set %d: refused: %s", set, why.c_str());
  if (rc) return;
  fcpr::LaunchList L;
  fcpr::build_launches(es.data(), n_tables, update, skipped, &L);
  EXPECT((int64_t)L.recs.size() <= n_tables + fcpr::kExtraRecs && (int64_t)L.launches.size() <= fcpr::kMaxLaunches, "set %d: bounds", set);
  std::map<const void *, int64_t> next_row; // by ids base of the entry -> rows seen so far
  std::map<uintptr_t, int> by_ids;
  for (int k = 0; k < n_tables; ++k) by_ids[(uintptr_t)es[k].row_ids] = k;
  check_launch_list(
      L, (int64_t)(L.recs_bytes() + L.prefix_bytes()), fcpr::workspace_bytes(n_tables), set,
      [&](const fcpr::Launch &l) { EXPECT(l.blocks <= fcpr::kMaxLaunchBlocks || l.n_recs == 1, "set %d: a launch of %u blocks and %u pieces", set, l.blocks, l.n_recs); },
      [&](const fcpr::Launch &l, const fcpr::Rec &r, uint32_t) {
        // which entry: the one whose ids the piece points into
        auto it = by_ids.upper_bound((uintptr_t)r.ids);
        --it;
        const fcp_table_rows_t &e = es[it->second];
        const int vec = fcpf::vec_of(e.dim);
        const int group = update && e.kind == FCP_TAB_Q8 ? fcpf::group_of(e.dim, vec) : 0;
        EXPECT(l.vec == vec && l.group == group, "set %d: entry %d in a launch of class (%d, %d)", set, it->second, l.vec, l.group);
        const int64_t spr = e.dim / vec, r0 = r.ids - e.row_ids;
        const int64_t rows = group ? (int64_t)r.n : (int64_t)r.n / spr;
        const int64_t threads = group ? rows * group : (int64_t)r.n;
        EXPECT(rows >= 1 && (group || (int64_t)r.n == rows * spr), "set %d: a piece of %u units", set, r.n);
        EXPECT(r0 == next_row[e.row_ids] && r.rows == e.rows + r0 * e.dim, "set %d: entry %d: piece at row %" PRId64, set, it->second, r0);
        EXPECT(threads <= fcpr::kMaxLaunchThreads || rows == 1, "set %d: a piece of %" PRId64 " threads", set, threads);
        next_row[e.row_ids] = r0 + rows;
        EXPECT(r.table == e.table && r.table_rows == (uint64_t)e.table_rows && r.dim == e.dim && r.kind == e.kind && r.spr == (uint32_t)spr && r.pad == 0,
               "set %d: entry %d: record", set, it->second);
        EXPECT(r.skipped == (skipped ? skipped + it->second : nullptr), "set %d: entry %d: skipped", set, it->second);
        return (uint32_t)((threads + fcpr::kBlockThreads - 1) / fcpr::kBlockThreads);
      });
  for (int k = 0; k < n_tables; ++k)
    EXPECT(next_row[es[k].row_ids] == std::max<int64_t>(es[k].n, 0), "set %d: entry %d: %" PRId64 " of %" PRId64 " rows", set, k, next_row[es[k].row_ids], es[k].n);
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: tables_rows_plan_san SEED SETS\n");
    return 2;
  }
  std::mt19937_64 rng(std::strtoull(argv[1], nullptr, 10));
  const int sets = std::atoi(argv[2]);
  const int dims[] = {1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 31, 32, 33, 64, 68, 128, 252, 256, 260, 1000, 1001, 1028, 514, 257};
  for (int s = 0; s < sets; ++s) {
    const int shape = s % 4; // 0: a few entries; 1: many small; 2: one above 2^30 threads among small; 3: several large
    const int n_tables = shape == 1 ? 1 + (int)(rng() % 3000) : (int)(rng() % 40);
    std::vector<fcp_table_rows_t> es;
    int64_t elems = 0; // the large entries stay within half the call's element bound together
    for (int k = 0; k < n_tables; ++k) {
      const int kind = (int)(rng() % 4), dim = dims[rng() % (sizeof(dims) / sizeof(dims[0]))];
      int64_t n = (int64_t)(rng() % 5 == 0 ? 0 : 1 + rng() % 600);
      if ((shape == 2 && k == n_tables / 2) || (shape == 3 && rng() % 4 == 0)) {
        const int64_t big = std::min<int64_t>((int64_t)((1ull << 26) + rng() % (1ull << 31)) / (shape == 3 ? 8 : 1), (1ll << 39) / dim);
        if (elems + big * dim <= (1ll << 39)) n = big, elems += big * dim;
      }
      es.push_back(entry(kind, dim, n, 1 + (int64_t)(rng() % (1ull << 31)), k));
    }
    check_set(es, true, s);
    check_set(es, false, s);
  }
  // the same 1000 entries once, ten times: the launches of a class do not grow
  {
    std::vector<fcp_table_rows_t> es;
    for (int rep = 0; rep < 10; ++rep)
      for (int k = 0; k < 100; ++k) es.push_back(entry(k % 4, dims[k % 24], 1 + k, 5000, rep * 100 + k));
    fcpr::LaunchList one, ten;
    fcpr::build_launches(es.data(), 100, true, nullptr, &one);
    fcpr::build_launches(es.data(), 1000, true, nullptr, &ten);
    EXPECT(one.launches.size() == ten.launches.size() && ten.launches.size() <= 24, "launches grew with the entries");
    check_set(es, true, -1);
  }
  // one row of 2^31 - 1 elements: one piece of 2^31 - 1 slots, alone in its launch
  {
    std::vector<fcp_table_rows_t> es = {entry(0, 16, 5, 100, 0), entry(0, INT32_MAX, 2, 100, 1), entry(1, 16, 7, 100, 2)};
    check_set(es, true, -2);
    fcpr::LaunchList L;
    fcpr::build_launches(es.data(), 3, true, nullptr, &L);
    EXPECT(L.launches.size() == 3, "%zu launches", L.launches.size()); // V 4: one; V 1: one per row
  }

  // the refusals, in order
  std::string why;
  void *W = reinterpret_cast<void *>(5 * A);
  std::vector<fcp_table_rows_t> es = {entry(3, 64, 5, 100, 0), entry(1, 62, 0, 100, 1), entry(0, 61, 9, 100, 2)};
  auto refused = [&](const char *word, const void *skipped, const void *ws, int32_t n = 3) {
    why.clear();
    const int rc = fcpr::check_call("who", es.data(), n, skipped, ws, &why);
    EXPECT(rc == FCP_ERR_INVALID_ARGUMENT && why.find(word) != std::string::npos && why.rfind("who: ", 0) == 0, "want %s, got %d: %s", word, rc, why.c_str());
  };
  refused("`n_tables`", nullptr, W, -1);
  refused("`n_tables`", nullptr, W, 65537);
  why.clear();
  EXPECT(fcpr::check_call("who", nullptr, 2, nullptr, W, &why) == FCP_ERR_INVALID_ARGUMENT && why.find("`entries`") != std::string::npos, "null entries: %s", why.c_str());
  EXPECT(fcpr::check_call("who", nullptr, 0, nullptr, nullptr, &why) == FCP_OK, "no entries refused");
  es[2].dim = 0;
  es[1].n = -1;
  refused("entry 1: `n`", nullptr, nullptr); // the first bad entry wins, and wins over the workspace
  es[1].n = 0;
  refused("entry 2: `dim`", nullptr, nullptr);
  es[2].dim = 61;
  es[2].reserved[1] = 1;
  es[2].rows = reinterpret_cast<float *>(3 * A + 2); // misaligned rows come before reserved
  refused("entry 2: `rows`", nullptr, nullptr);
  es[2].rows = reinterpret_cast<float *>(3 * A);
  refused("entry 2: `reserved`", nullptr, nullptr);
  es[2].reserved[1] = 0;
  es[0].n = es[2].n = (1ll << 32) - 4; // 2^32 rows of dim 64 and of dim 61: below 2^40 elements
  why.clear();
  EXPECT(fcpr::check_call("who", es.data(), 3, nullptr, W, &why) == FCP_OK, "%s", why.c_str());
  es[0].dim = 256;
  refused("`entries`", nullptr, nullptr); // 2^40 elements and more
  es[0].dim = 64;
  es[0].n = es[2].n = 5;
  refused("`workspace`", reinterpret_cast<void *>(4 * A + 4), nullptr);
  refused("`workspace`", reinterpret_cast<void *>(4 * A + 4), reinterpret_cast<void *>(5 * A + 4));
  refused("`skipped`", reinterpret_cast<void *>(4 * A + 4), W);
  EXPECT(fcpr::workspace_bytes(-1) == -1 && fcpr::workspace_bytes(65537) == -1 && fcpr::workspace_bytes(0) > 0, "workspace range");
  for (int n = 0; n < 65536; n += 257)
    EXPECT(fcpr::workspace_bytes(n) % 8 == 0 && fcpr::workspace_bytes(n) <= fcpr::workspace_bytes(n + 1), "workspace at %d", n);

  std::printf("%d sets\n%d failures\n", sets, failures);
  return failures ? 1 : 0;
}
