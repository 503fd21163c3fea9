// tables_delta_plan_san.cc — the host-only level of the grouped delta distinct (recom_amd/csrc/fcp_tables_delta_plan.cc) on its
// own, for a build with -fsanitize=address,undefined: the unit needs no GPU runtime and no other unit of the library.
//   tables_delta_plan_san SEED SETS
// Drives the launch-list builder over SETS random entry sets — ids only and rows of every V and G, int32 and int64 ids, empty
// entries, a few large ones, sets whose lone grids sum past the deal's cap (pointers are numbers: nothing is dereferenced) — and
// checks, per set, what the kernels rely on: the compact launches' own promises (grouped_image_check.h); a launch holds entries
// of ONE class; the insert and the classify launch's first-block tables start at 0, ascend strictly and end at their grids; a
// record's grid covers its n with no idle block, within its run of partial records; every entry's partial records, cells and
// flags lie inside the workspace fcp_tables_delta_workspace_bytes states and meet no other entry's; the cells lie back to back;
// the image fits its room; the deal's bound.  Then the workspace formula and the refusals, in order.  Prints `<n> sets` and
// `<n> failures`.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "fcp_tables_delta_plan.h"

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
#include "grouped_image_check.h" // check_launch_list: what every grouped entry's kernels rely on (needs EXPECT)

static const uintptr_t A = uintptr_t(1) << 40; // aligned for everything
static const uintptr_t IMAGE = uintptr_t(1) << 44;

// (the ids of entry k lie 2^36 bytes behind those of entry k - 1: a record's ids tell its entry)
static fcp_table_delta_entry_t entry(int dim, int64_t n, int64_t table_rows, int id_bytes, bool pos, int k) {
  fcp_table_delta_entry_t e = {};
  e.row_ids = reinterpret_cast<const void *>((uintptr_t(1) << 50) + ((uintptr_t)k << 36));
  e.rows = dim ? reinterpret_cast<const float *>((uintptr_t(1) << 52) + (uintptr_t)k * 4096) : nullptr;
  e.ids_out = reinterpret_cast<int64_t *>((uintptr_t(1) << 54) + ((uintptr_t)k << 36));
  e.rows_out = dim ? reinterpret_cast<float *>((uintptr_t(1) << 56) + (uintptr_t)k * 4096) : nullptr;
  e.pos_out = pos ? reinterpret_cast<int64_t *>((uintptr_t(1) << 58) + ((uintptr_t)k << 36)) : nullptr;
  e.table_rows = table_rows;
  e.n = n;
  e.id_bytes = id_bytes;
  e.dim = dim;
  return e;
}

static void check_prefix(const std::vector<uint32_t> &prefix, const std::vector<uint32_t> &blocks, const char *what, int set) {
  EXPECT(prefix.size() == (blocks.empty() ? 0 : blocks.size() + 1), "set %d: %s: %zu values for %zu records", set, what, prefix.size(), blocks.size());
  if (prefix.size() != blocks.size() + 1) return;
  uint32_t first = 0;
  for (size_t j = 0; j < blocks.size(); ++j) {
    EXPECT(prefix[j] == first && blocks[j] >= 1, "set %d: %s[%zu] = %u, want %u (%u blocks)", set, what, j, prefix[j], first, blocks[j]);
    first += blocks[j];
  }
  EXPECT(prefix.back() == first, "set %d: %s ends at %u, records sum to %u", set, what, prefix.back(), first);
}

static void check_set(const std::vector<fcp_table_delta_entry_t> &es, int set) {
  const int32_t n_tables = (int32_t)es.size();
  std::string why;
  const int rc = fcptd::check_call(es.data(), n_tables, reinterpret_cast<void *>(4 * A), reinterpret_cast<void *>(5 * A), &why);
  EXPECT(rc == FCP_OK && why.empty(), "set %d: refused: %s", set, why.c_str());
  if (rc) return;
  std::vector<int64_t> ns;
  int64_t lone_sum = 0;
  for (const auto &e : es) {
    ns.push_back(e.n);
    if (e.n > 0) lone_sum += fcptd::grid_of(e.n, fcptd::kLoneBlocks).nblocks;
  }
  const int64_t ws = fcptd::workspace_bytes(ns.data(), n_tables);
  EXPECT(ws > 0 && ws % 8 == 0, "set %d: workspace %" PRId64, set, ws);
  fcptd::LaunchList L;
  fcptd::build_launches(es.data(), n_tables, IMAGE, &L);
  const fcptd::Layout lay = fcptd::layout_of(es.data(), n_tables);
  EXPECT(16 + lay.end == ws && (int64_t)L.image_bytes() <= fcptd::image_room(n_tables) && fcptd::image_room(n_tables) == lay.partials_off,
         "set %d: image %zu, room %" PRId64, set, L.image_bytes(), fcptd::image_room(n_tables));
  EXPECT(lay.partials_off <= lay.cells_off && lay.cells_off <= lay.flags_off && lay.flags_off <= lay.end && lay.cells_off % 8 == 0, "set %d: layout", set);
  EXPECT((int)L.launches.size() <= fcptd::kCompactClasses && L.n_launches() <= fcptd::kMaxLaunches, "set %d: %zu compact launches", set, L.launches.size());
  EXPECT((int32_t)L.runs.size() == n_tables && (int32_t)L.blocks.size() == n_tables, "set %d: runs", set);

  std::map<uintptr_t, int> by_ids;
  for (int k = 0; k < n_tables; ++k) by_ids[(uintptr_t)es[k].row_ids] = k;
  std::vector<int> seen((size_t)n_tables, 0);
  std::vector<uint32_t> insert_blocks, classify_blocks;
  struct Span { uintptr_t lo, hi; };
  std::vector<Span> partials, cells, flags;
  check_launch_list(
      L, (int64_t)L.image_bytes(), ws, set, [&](const fcptd::Launch &) {},
      [&](const fcptd::Launch &l, const fcptd::Rec &r, uint32_t) {
        auto it = by_ids.find((uintptr_t)r.ids);
        EXPECT(it != by_ids.end(), "set %d: a record of no entry", set);
        if (it == by_ids.end()) return 1u;
        const int k = it->second;
        const fcp_table_delta_entry_t &e = es[k];
        ++seen[k];
        const int vec = e.rows ? fcpf::vec_of(e.dim) : 0, group = e.rows ? fcpf::group_of(e.dim, vec) : 1;
        EXPECT(l.vec == vec && l.group == group, "set %d: entry %d (dim %d) in a launch of class (%d, %d)", set, k, e.dim, l.vec, l.group);
        EXPECT(r.rows == e.rows && r.ids_out == e.ids_out && r.pos_out == e.pos_out && r.rows_out == e.rows_out && r.n == e.n && e.n > 0 &&
                   r.table_rows == (uint64_t)e.table_rows && r.is64 == (e.id_bytes == 8) && r.dim == (e.rows ? e.dim : 0),
               "set %d: entry %d: record", set, k);
        for (uint32_t p : r.pad) EXPECT(p == 0, "set %d: entry %d: pad", set, k);
        // the grid: whole tiles, at least the smallest chunk, every block with positions, inside the entry's run of records
        EXPECT(r.chunk % fcptd::kTile == 0 && r.chunk >= fcptd::kMinChunkTiles * fcptd::kTile && r.nblocks >= 1 &&
                   (int64_t)(r.nblocks - 1) * r.chunk < e.n && (int64_t)r.nblocks * r.chunk >= e.n,
               "set %d: entry %d: %u blocks of %" PRId64 " for %" PRId64 " ids", set, k, r.nblocks, r.chunk, e.n);
        const fcptd::Grid lone = fcptd::grid_of(e.n, fcptd::kLoneBlocks);
        EXPECT(r.nblocks <= lone.nblocks && (int64_t)r.nblocks + 1 <= fcptd::partial_recs(e.n), "set %d: entry %d: %u blocks, lone %u", set, k, r.nblocks, lone.nblocks);
        if (lone_sum <= fcptd::kDealBlocks) EXPECT(r.nblocks == lone.nblocks && r.chunk == lone.chunk, "set %d: entry %d: not its lone grid", set, k);
        EXPECT(L.blocks[k] == r.nblocks && L.runs[k].nblocks == r.nblocks && L.runs[k].n == e.n, "set %d: entry %d: run", set, k);
        const int64_t tiles = (e.n + fcptd::kInsertTile - 1) / fcptd::kInsertTile;
        EXPECT(r.insert_blocks == (uint32_t)std::min<int64_t>(tiles, fcptd::kInsertMaxBlocks), "set %d: entry %d: %u insert blocks", set, k, r.insert_blocks);
        // the hash table: a power of two, at least 2 n; the sections inside the workspace
        const int64_t n_cells = int64_t(1) << (64 - r.shift);
        EXPECT(n_cells == fcptd::cells_for(e.n) && n_cells >= 2 * e.n && n_cells >= fcptd::kMinCells, "set %d: entry %d: %" PRId64 " cells", set, k, n_cells);
        const uintptr_t p0 = (uintptr_t)r.partials, c0 = (uintptr_t)r.cells, f0 = (uintptr_t)r.flags;
        EXPECT(p0 == IMAGE + (uintptr_t)lay.partials_off + (uintptr_t)L.runs[k].first * 32, "set %d: entry %d: the run and the record disagree", set, k);
        partials.push_back(Span{p0, p0 + (uintptr_t)fcptd::partial_recs(e.n) * 32});
        cells.push_back(Span{c0, c0 + (uintptr_t)n_cells * 8});
        flags.push_back(Span{f0, f0 + (uintptr_t)e.n});
        EXPECT(p0 % 8 == 0 && c0 % 8 == 0 && p0 >= IMAGE + (uintptr_t)lay.partials_off && partials.back().hi <= IMAGE + (uintptr_t)lay.cells_off &&
                   c0 >= IMAGE + (uintptr_t)lay.cells_off && cells.back().hi <= IMAGE + (uintptr_t)lay.flags_off && f0 >= IMAGE + (uintptr_t)lay.flags_off &&
                   flags.back().hi <= IMAGE + (uintptr_t)lay.end,
               "set %d: entry %d: a section outside its area", set, k);
        insert_blocks.push_back(r.insert_blocks);
        classify_blocks.push_back(r.nblocks);
        return r.nblocks;
      });
  for (int k = 0; k < n_tables; ++k) {
    EXPECT(seen[k] == (es[k].n > 0 ? 1 : 0), "set %d: entry %d: %d records", set, k, seen[k]);
    if (es[k].n <= 0) EXPECT(L.blocks[k] == 0 && L.runs[k].nblocks == 0, "set %d: entry %d: an empty entry with blocks", set, k);
  }
  check_prefix(L.insert_prefix, insert_blocks, "insert prefix", set);
  check_prefix(L.classify_prefix, classify_blocks, "classify prefix", set);
  int64_t grid = 0;
  for (uint32_t b : classify_blocks) grid += b;
  EXPECT(grid <= fcptd::kDealBlocks + n_tables && grid == (int64_t)L.classify_grid(), "set %d: %" PRId64 " classify blocks", set, grid);
  // no two entries' sections meet; the cells lie back to back from the area's start
  auto disjoint = [&](std::vector<Span> &v, const char *what, bool back_to_back, uintptr_t start) {
    std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    for (size_t i = 0; i + 1 < v.size(); ++i)
      EXPECT(back_to_back ? v[i].hi == v[i + 1].lo : v[i].hi <= v[i + 1].lo, "set %d: %s of two entries %s", set, what, back_to_back ? "are not back to back" : "meet");
    if (back_to_back && !v.empty()) EXPECT(v[0].lo == start, "set %d: %s do not start their area", set, what);
  };
  disjoint(partials, "partial records", false, 0);
  disjoint(cells, "cells", true, IMAGE + (uintptr_t)lay.cells_off);
  disjoint(flags, "flags", false, 0);
  uint64_t total = 0;
  for (const Span &s : cells) total += (s.hi - s.lo) / 8;
  EXPECT(total == L.total_cells, "set %d: the clear covers %" PRIu64 " cells of %" PRIu64, set, (uint64_t)L.total_cells, total);
  // the image round trip: sections where the offsets say, padding zeroed
  if (L.image_bytes() > 0 && L.image_bytes() < (size_t(1) << 24)) {
    std::vector<char> buf(L.image_bytes(), (char)0xAB);
    L.write_image(buf.data());
    EXPECT(L.recs.empty() || !std::memcmp(buf.data(), L.recs.data(), L.recs_bytes()), "set %d: records of the image", set);
    EXPECT(L.insert_prefix.empty() || !std::memcmp(buf.data() + L.insert_off(), L.insert_prefix.data(), L.insert_prefix.size() * 4), "set %d: insert prefix of the image", set);
    EXPECT(L.classify_prefix.empty() || !std::memcmp(buf.data() + L.classify_off(), L.classify_prefix.data(), L.classify_prefix.size() * 4), "set %d: classify prefix of the image", set);
    EXPECT(L.runs.empty() || !std::memcmp(buf.data() + L.runs_off(), L.runs.data(), L.runs.size() * sizeof(fcptd::Run)), "set %d: runs of the image", set);
    EXPECT(std::find(buf.begin(), buf.end(), (char)0xAB) == buf.end() || !L.recs.empty(), "set %d: bytes of the image left unwritten", set);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: tables_delta_plan_san SEED SETS\n");
    return 2;
  }
  std::mt19937_64 rng(std::strtoull(argv[1], nullptr, 10));
  const int sets = std::atoi(argv[2]);
  const int dims[] = {0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 31, 32, 33, 62, 64, 68, 128, 252, 256, 260, 300, 1000, 1001, 514, 257};
  const int64_t sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 100000};
  for (int s = 0; s < sets; ++s) {
    const int shape = s % 4; // 0: a few entries; 1: many small; 2: one large among small; 3: lone grids that sum past the cap
    const int n_tables = shape == 1 ? 1 + (int)(rng() % 3000) : shape == 3 ? 20 + (int)(rng() % 60) : (int)(rng() % 40);
    std::vector<fcp_table_delta_entry_t> es;
    for (int k = 0; k < n_tables; ++k) {
      const int dim = dims[rng() % (sizeof(dims) / sizeof(dims[0]))];
      int64_t n = rng() % 5 == 0 ? 0 : sizes[rng() % (sizeof(sizes) / sizeof(sizes[0]))];
      if (shape == 2 && k == n_tables / 2) n = (int64_t)((1ull << 20) + rng() % (1ull << 31));
      if (shape == 3 && rng() % 2) n = (int64_t)(200000 + rng() % 4000000);
      es.push_back(entry(dim, n, 1 + (int64_t)(rng() % (1ull << 31)), rng() % 2 ? 4 : 8, rng() % 3 == 0, k));
    }
    check_set(es, s);
  }
  // the same 100 entries once, ten times: the launches do not grow
  {
    std::vector<fcp_table_delta_entry_t> es;
    for (int rep = 0; rep < 10; ++rep)
      for (int k = 0; k < 100; ++k) es.push_back(entry(dims[k % 28], 1 + k, 5000, k % 2 ? 4 : 8, k % 3 == 0, rep * 100 + k));
    fcptd::LaunchList one, ten;
    fcptd::build_launches(es.data(), 100, 0, &one);
    fcptd::build_launches(es.data(), 1000, 0, &ten);
    EXPECT(one.n_launches() == ten.n_launches() && ten.n_launches() <= fcptd::kMaxLaunches, "launches grew with the entries");
    check_set(es, -1);
    fcptd::LaunchList none;
    fcptd::build_launches(es.data(), 0, 0, &none);
    EXPECT(none.n_launches() == 0, "launches without entries");
    for (auto &e : es) e.n = 0;
    fcptd::build_launches(es.data(), 1000, 0, &none);
    EXPECT(none.n_launches() == 1 && none.recs.empty() && none.total_cells == 0, "launches without ids");
    check_set(es, -2);
  }
  // the last n_tables, every entry of one id; one entry at the row limit's edge
  {
    std::vector<fcp_table_delta_entry_t> es;
    for (int k = 0; k < 65536; ++k) es.push_back(entry(k % 3 ? 0 : 16, 1, 7, 8, false, k));
    check_set(es, -3);
    es.assign(1, entry(64, fcpf::kRowLimit - 1, 1000, 4, true, 0));
    check_set(es, -4);
  }

  // the workspace formula: -1 cases, a multiple of 8, monotone in each n[k], within the header's bound
  {
    std::vector<int64_t> ns = {5, 0, 1024, 100000};
    EXPECT(fcptd::workspace_bytes(ns.data(), -1) == -1 && fcptd::workspace_bytes(ns.data(), 65537) == -1 && fcptd::workspace_bytes(nullptr, 1) == -1, "workspace range");
    EXPECT(fcptd::workspace_bytes(nullptr, 0) > 0, "workspace of no entries");
    ns[1] = -1;
    EXPECT(fcptd::workspace_bytes(ns.data(), 4) == -1, "a negative n");
    ns[1] = fcpf::kRowLimit;
    EXPECT(fcptd::workspace_bytes(ns.data(), 4) == -1, "an n at the limit");
    ns[1] = fcpf::kRowLimit - 1 - (5 + 1024 + 100000);
    EXPECT(fcptd::workspace_bytes(ns.data(), 4) > 0, "a sum below the limit");
    ++ns[1];
    EXPECT(fcptd::workspace_bytes(ns.data(), 4) == -1, "a sum at the limit");
    for (int t = 0; t < 2000; ++t) {
      const int nt = 1 + (int)(rng() % 50);
      std::vector<int64_t> v;
      int64_t sum = 0;
      for (int k = 0; k < nt; ++k) v.push_back(rng() % 4 == 0 ? 0 : (int64_t)(rng() % (rng() % 2 ? 5000 : 3000000))), sum += v.back();
      const int64_t w = fcptd::workspace_bytes(v.data(), nt);
      EXPECT(w > 0 && w % 8 == 0 && w <= 40 * sum + 1024 * (int64_t)nt + 1024, "workspace %" PRId64 " of %d entries, %" PRId64 " ids", w, nt, sum);
      const int k = (int)(rng() % nt);
      v[k] += 1 + (int64_t)(rng() % 3000);
      EXPECT(fcptd::workspace_bytes(v.data(), nt) >= w, "workspace decreases in n[%d]", k);
    }
  }

  // the refusals, in order
  std::string why;
  void *W = reinterpret_cast<void *>(5 * A), *R = reinterpret_cast<void *>(4 * A);
  std::vector<fcp_table_delta_entry_t> es = {entry(64, 5, 100, 8, true, 0), entry(0, 0, 100, 4, false, 1), entry(61, 9, 100, 4, false, 2)};
  auto refused = [&](const char *word, const void *reports, const void *ws, int32_t n = 3) {
    why.clear();
    const int rc = fcptd::check_call(es.data(), n, reports, ws, &why);
    EXPECT(rc == FCP_ERR_INVALID_ARGUMENT && why.find(word) != std::string::npos && why.rfind("fcp_tables_delta_distinct: ", 0) == 0, "want %s, got %d: %s", word, rc, why.c_str());
  };
  refused("`n_tables`", R, W, -1);
  refused("`n_tables`", R, W, 65537);
  why.clear();
  EXPECT(fcptd::check_call(nullptr, 2, R, W, &why) == FCP_ERR_INVALID_ARGUMENT && why.find("`entries`") != std::string::npos, "null entries: %s", why.c_str());
  EXPECT(fcptd::check_call(nullptr, 0, nullptr, nullptr, &why) == FCP_OK, "no entries refused");
  EXPECT(fcptd::check_call(es.data(), 3, R, W, &why) == FCP_OK, "%s", why.c_str());
  es[2].id_bytes = 2;
  es[1].n = -1;
  refused("entry 1: `n` is negative", nullptr, nullptr); // the first bad entry wins, and wins over reports and workspace
  es[1].n = 0;
  refused("entry 2: `id_bytes` is 4 (int32 ids) or 8 (int64 ids)", nullptr, nullptr);
  es[2].id_bytes = 4;
  es[2].rows_out = nullptr;
  refused("entry 2: `rows_out` is null and `rows` is not", nullptr, nullptr);
  es[2].rows_out = reinterpret_cast<float *>(3 * A + 2);
  refused("entry 2: `rows_out` is not 4-byte aligned (float32 rows of this dim)", nullptr, nullptr);
  es[2].rows_out = reinterpret_cast<float *>(3 * A);
  es[0].n = es[2].n = (fcpf::kRowLimit - 1) / 2; // together one below the limit
  why.clear();
  EXPECT(fcptd::check_call(es.data(), 3, R, W, &why) == FCP_OK, "%s", why.c_str());
  es[1].n = 1;
  es[1].row_ids = es[0].row_ids, es[1].ids_out = es[0].ids_out;
  refused("`entries` name 2^32 - 3 ids or more together", nullptr, nullptr);
  es[0].n = es[2].n = 5;
  refused("`reports` is null", nullptr, nullptr);
  refused("`reports` is not 8-byte aligned", reinterpret_cast<void *>(4 * A + 4), nullptr);
  refused("`workspace` is null", R, nullptr);
  refused("`workspace` is not 8-byte aligned", R, reinterpret_cast<void *>(5 * A + 4));

  std::printf("%d sets\n%d failures\n", sets, failures);
  return failures ? 1 : 0;
}
