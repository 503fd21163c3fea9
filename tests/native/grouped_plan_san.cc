// grouped_plan_san.cc — what the host-only levels of the grouped table entries share (recom_amd/csrc/fcp_grouped_plan.h) on its
// own, for a build with -fsanitize=address,undefined: a header, no unit of the library, no GPU runtime.
//   grouped_plan_san SEED SETS
// Over SETS random inputs: the class sort against std::stable_sort (empty classes, entries of class -1, every entry -1, no
// entries); the launch-list builder with and without a block cap over random block counts — the list's own promises
// (grouped_image_check.h), no launch past the cap unless it is one record, a launch closed only where the next record would
// have passed the cap, every launch of its class, the launches' records the input in its order.  Then log2_of and the shared
// refusals, in order, by their whole text.  Prints `<n> sets` and `<n> failures`.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "fcp_grouped_plan.h"

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
#include "grouped_image_check.h"

struct Rec {
  uint64_t id, blocks;
};
struct Launch {
  int32_t cls;
  uint32_t first_rec, n_recs, prefix_off, blocks;
};
using List = fcpgp::LaunchList<Rec, Launch>;

static void check_sort(const std::vector<int> &cls, int n_classes, int set) {
  const int32_t n = (int32_t)cls.size();
  const fcpgp::ClassSort s = fcpgp::sort_by_class(n, n_classes, [&](int32_t k) { return cls[k]; });
  std::vector<int32_t> want;
  for (int32_t k = 0; k < n; ++k)
    if (cls[k] >= 0) want.push_back(k);
  std::stable_sort(want.begin(), want.end(), [&](int32_t a, int32_t b) { return cls[a] < cls[b]; });
  EXPECT(s.members == want, "set %d: the members are not the stable sort", set);
  EXPECT(s.first[0] == 0 && s.first[n_classes] == (int32_t)want.size(), "set %d: first[] spans %d .. %d", set, s.first[0], s.first[n_classes]);
  for (int c = 0; c < n_classes; ++c) {
    EXPECT(s.first[c] <= s.first[c + 1], "set %d: class %d ends in front of its start", set, c);
    for (int32_t m = s.first[c]; m < s.first[c + 1] && m < (int32_t)want.size(); ++m) EXPECT(cls[s.members[m]] == c, "set %d: member %d in class %d", set, m, c);
  }
}

// records (class, blocks) in the order given, a launch opened per run of one class
static void check_builder(const std::vector<std::pair<int, uint32_t>> &in, int64_t cap, int set) {
  List L;
  L.recs.push_back(Rec{99, 99}); // clear() forgets an earlier call
  L.clear(cap);
  for (size_t i = 0; i < in.size(); ++i) {
    if (i == 0 || in[i].first != in[i - 1].first) {
      L.close();
      L.open(Launch{in[i].first, 7, 7, 7, 7});
    }
    L.add(Rec{(uint64_t)i, in[i].second}, in[i].second);
    EXPECT(L.open_blocks() == L.prefix.back() + in[i].second, "set %d: the open launch has %u blocks behind record %zu", set, L.open_blocks(), i);
  }
  L.close();
  L.close(); // closing twice leaves nothing
  uint64_t next = 0;
  int runs = 0;
  for (size_t i = 0; i < in.size(); ++i) runs += i == 0 || in[i].first != in[i - 1].first;
  if (!cap) EXPECT((int)L.launches.size() == runs, "set %d: %zu launches of %d classes without a cap", set, L.launches.size(), runs);
  EXPECT(L.recs_bytes() == L.recs.size() * sizeof(Rec) && L.prefix_bytes() % 16 == 0 && L.prefix_bytes() >= L.prefix.size() * 4 && L.prefix_bytes() < L.prefix.size() * 4 + 16,
         "set %d: section bytes", set);
  const Launch *prev = nullptr;
  check_launch_list(
      L, (int64_t)(L.recs_bytes() + L.prefix_bytes()), (int64_t)(16 + L.recs_bytes() + L.prefix_bytes()), set,
      [&](const Launch &l) {
        EXPECT(!cap || l.blocks <= cap || l.n_recs == 1, "set %d: a launch of %u blocks and %u records past the cap", set, l.blocks, l.n_recs);
        EXPECT(l.cls == in[next].first, "set %d: a launch of class %d at a record of class %d", set, l.cls, in[next].first);
        // a launch that continues its class: the record it starts with did not fit the one in front
        if (prev && next > 0 && in[next - 1].first == in[next].first)
          EXPECT(cap && (int64_t)prev->blocks + in[next].second > cap, "set %d: a launch closed at %u blocks in front of a record of %u", set, prev->blocks, in[next].second);
        prev = &l;
      },
      [&](const Launch &l, const Rec &r, uint32_t) {
        EXPECT(r.id == next && next < in.size() && in[next].first == l.cls && r.blocks == in[next].second, "set %d: record %llu at place %llu", set,
               (unsigned long long)r.id, (unsigned long long)next);
        ++next;
        return (uint32_t)r.blocks;
      });
  EXPECT(next == in.size(), "set %d: %llu of %zu records", set, (unsigned long long)next, in.size());
  // the image: records, then prefixes, zeros up to the 16-byte multiple and not a byte more
  std::vector<char> image(L.recs_bytes() + L.prefix_bytes() + 1, 0x5a);
  L.write_image(image.data());
  EXPECT(L.recs.empty() || std::memcmp(image.data(), L.recs.data(), L.recs_bytes()) == 0, "set %d: the image's records", set);
  EXPECT(L.prefix.empty() || std::memcmp(image.data() + L.recs_bytes(), L.prefix.data(), L.prefix.size() * 4) == 0, "set %d: the image's prefixes", set);
  for (size_t b = L.recs_bytes() + L.prefix.size() * 4; b + 1 < image.size(); ++b) EXPECT(image[b] == 0, "set %d: byte %zu of the padding is not 0", set, b);
  EXPECT(image.back() == 0x5a, "set %d: a byte written behind the image", set);
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: grouped_plan_san SEED SETS\n");
    return 2;
  }
  std::mt19937_64 rng(std::strtoull(argv[1], nullptr, 10));
  const int sets = std::atoi(argv[2]);
  for (int s = 0; s < sets; ++s) {
    // the sort: 1 to 64 classes, of which some stay empty; a share of the entries takes no part
    const int n_classes = 1 + (int)(rng() % fcpgp::kMaxClasses), used = 1 + (int)(rng() % n_classes);
    const int n = s % 7 == 0 ? 0 : (int)(rng() % (s % 5 == 0 ? 5000 : 60));
    const int out_of = s % 3 == 0 ? 1 : 2 + (int)(rng() % 5); // 1: every entry is -1
    std::vector<int> cls((size_t)n);
    for (int &c : cls) c = rng() % out_of == 0 ? -1 : (int)(rng() % used) * (n_classes / used);
    check_sort(cls, n_classes, s);
    // the builder: the sorted members as runs of one class, blocks small, near the cap and above it
    const fcpgp::ClassSort sorted = fcpgp::sort_by_class(n, n_classes, [&](int32_t k) { return cls[k]; });
    const int64_t cap = 1000;
    std::vector<std::pair<int, uint32_t>> in;
    for (int32_t k : sorted.members) {
      const uint32_t pick = (uint32_t)(rng() % 10);
      in.push_back({cls[k], pick == 0 ? (uint32_t)(cap - 1 + rng() % 3) : pick == 1 ? (uint32_t)(cap + 1 + rng() % 5000) : 1 + (uint32_t)(rng() % 400)});
    }
    check_builder(in, 0, s);
    check_builder(in, cap, s);
  }
  check_sort({}, 1, -1);
  check_sort(std::vector<int>(100, -1), fcpgp::kMaxClasses, -2);
  check_sort(std::vector<int>(100, fcpgp::kMaxClasses - 1), fcpgp::kMaxClasses, -3);
  check_builder({}, 1000, -4);
  check_builder({{3, 1000}, {3, 1}, {3, 999}, {3, 1}, {3, 1}, {5, 4000}, {5, 4000}, {6, 1}}, 1000, -5); // 3: 1000 | 1 999 | 1 1; 5: alone twice

  static_assert(fcpgp::log2_of(1) == 0 && fcpgp::log2_of(2) == 1 && fcpgp::log2_of(64) == 6, "log2_of at compile time");
  volatile int one = 1, two = 2, sixty_four = 64;
  EXPECT(fcpgp::log2_of(one) == 0 && fcpgp::log2_of(two) == 1 && fcpgp::log2_of(sixty_four) == 6, "log2_of");
  EXPECT(fcpgp::kMaxLaunchRecs == 65537 && fcpgp::log2_of(fcpgp::kMaxLaunchRecs) == 17, "the search depth of a launch's records");

  // the shared refusals, in order, by their whole text
  std::string why;
  int asked = 0;
  int bad_entry = -1;
  auto entry = [&](int32_t k, std::string *what) {
    ++asked;
    return k >= bad_entry && bad_entry >= 0 ? fcpgp::refuse(what, "`dim` must be positive") : (int)FCP_OK;
  };
  const char some[8] = {};
  auto refused = [&](const char *want, const void *entries, int32_t n) {
    why.clear();
    const int rc = fcpgp::check_entries("who: ", entries, n, &why, entry);
    EXPECT(rc == FCP_ERR_INVALID_ARGUMENT && why == want, "want %s, got %d: %s", want, rc, why.c_str());
  };
  refused("who: `n_tables` must lie in [0, 65536]", some, -1);
  refused("who: `n_tables` must lie in [0, 65536]", some, 65537);
  refused("who: `entries` is null", nullptr, 1);
  EXPECT(asked == 0, "an entry was looked at behind a refusal of the call");
  bad_entry = 2;
  refused("who: entry 2: `dim` must be positive", some, 5); // the first bad entry wins, and ends the loop
  EXPECT(asked == 3, "%d entries looked at", asked);
  bad_entry = -1;
  EXPECT(fcpgp::check_entries("who: ", nullptr, 0, &why, entry) == FCP_OK && fcpgp::check_entries("who: ", some, 65536, nullptr, entry) == FCP_OK, "good entries refused");
  EXPECT(fcpgp::refuse(nullptr, "no place for the text") == FCP_ERR_INVALID_ARGUMENT, "refuse without a string");
  why.clear();
  EXPECT(fcpgp::check_workspace("who: ", 3, nullptr, &why) == FCP_ERR_INVALID_ARGUMENT && why == "who: `workspace` is null", "%s", why.c_str());
  EXPECT(fcpgp::check_workspace("who: ", 3, reinterpret_cast<const void *>(uintptr_t(4100)), &why) == FCP_ERR_INVALID_ARGUMENT &&
             why == "who: " + fcpf::not_aligned("workspace", 8) && why == "who: `workspace` is not 8-byte aligned",
         "%s", why.c_str());
  why.clear();
  EXPECT(fcpgp::check_workspace("who: ", 0, nullptr, &why) == FCP_OK && fcpgp::check_workspace("who: ", 3, reinterpret_cast<const void *>(uintptr_t(4096)), &why) == FCP_OK &&
             why.empty(),
         "a good workspace refused: %s", why.c_str());
  EXPECT(fcpgp::check_workspace("who: ", 0, reinterpret_cast<const void *>(uintptr_t(4100)), &why) == FCP_ERR_INVALID_ARGUMENT, "a misaligned workspace of no entries");

  std::printf("%d sets\n%d failures\n", sets, failures);
  return failures ? 1 : 0;
}
