// fcp_grouped_plan.h — what the host-only levels of the grouped table entries share (fcp_tables_rows_plan.h,
// fcp_tables_digest_plan.h), written ONCE as fcp_find_piece.h is for their kernels: the constants, the refusals every grouped
// entry makes by one text, the sort of a call's entries into classes and the launch list with its descriptor image.  No GPU
// header and no unit of its own: ordinary C++, linked and tested under sanitizers without the HIP runtime
// (tests/native/grouped_plan_san.cc).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fcp_hip.h"
#include "fcp_formats.h"

namespace fcpgp {

constexpr int32_t kMaxTables = 65536;            // n_tables lies in [0, kMaxTables]
constexpr int kBlockThreads = 256;               // FCP_BLOCK_THREADS (the .hip units assert it)
constexpr int32_t kMaxLaunchRecs = kMaxTables + 1; // the most records of one launch (fcp_grouped_front.h: find_piece reaches them)
constexpr int kMaxClasses = 64;

// the index of a power of two (for any v >= 1: the least l with v <= 2^l)
constexpr int log2_of(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

inline int refuse(std::string *why, const std::string &msg) {
  if (why) *why = msg;
  return FCP_ERR_INVALID_ARGUMENT;
}

// The refusals in front of every grouped entry's own, `w` = "<who>: " in front of the message: n_tables, `entries`, then the
// entries in ascending order — check_entry(k, &what) returns a status and, with one that is not FCP_OK, what goes behind
// "<who>: entry k: " (made for a refusal only: a model has thousands of entries).
template <class F> int check_entries(const std::string &w, const void *entries, int32_t n_tables, std::string *why, F check_entry) {
  if (n_tables < 0 || n_tables > kMaxTables) return refuse(why, w + "`n_tables` must lie in [0, 65536]");
  if (n_tables > 0 && !entries) return refuse(why, w + "`entries` is null");
  for (int32_t k = 0; k < n_tables; ++k) {
    std::string what;
    if (check_entry(k, &what)) return refuse(why, w + "entry " + std::to_string(k) + ": " + what);
  }
  return FCP_OK;
}
// ... and behind them, of the call's workspace
inline int check_workspace(const std::string &w, int32_t n_tables, const void *workspace, std::string *why) {
  if (n_tables > 0 && !workspace) return refuse(why, w + "`workspace` is null");
  if ((uintptr_t)workspace % 8) return refuse(why, w + fcpf::not_aligned("workspace", 8));
  return FCP_OK;
}

// The classes present and the entries of each in ascending order: a counting sort, stable inside a class.  class_of_entry(k)
// is in [0, n_classes), n_classes <= kMaxClasses, or -1: the entry takes no part.  Class c holds members[first[c] .. first[c + 1]).
struct ClassSort {
  int32_t first[kMaxClasses + 1] = {};
  std::vector<int32_t> members;
};
template <class F> ClassSort sort_by_class(int32_t n_tables, int n_classes, F class_of_entry) {
  ClassSort s;
  std::vector<int8_t> cls((size_t)std::max(n_tables, 0), -1);
  for (int32_t k = 0; k < n_tables; ++k)
    if ((cls[k] = (int8_t)class_of_entry(k)) >= 0) ++s.first[cls[k] + 1];
  for (int c = 0; c < kMaxClasses; ++c) s.first[c + 1] += s.first[c];
  s.members.resize((size_t)s.first[n_classes]);
  int32_t at[kMaxClasses];
  std::copy(s.first, s.first + kMaxClasses, at);
  for (int32_t k = 0; k < n_tables; ++k)
    if (cls[k] >= 0) s.members[at[cls[k]]++] = k;
  return s;
}

// The launch list of one call and its descriptor image.  Rec: a record of the image, a multiple of 16 bytes (the upload kernel
// moves 16-byte words).  Launch: one kernel launch, the records recs[first_rec .. first_rec + n_recs) of ONE class and
// prefix[prefix_off .. prefix_off + n_recs] — the first block of each record in the launch's grid, ascending from 0, and the
// grid itself, `blocks`, as the last value; what else a Launch holds (its class) is the header open() is given.
template <class Rec, class Launch> struct LaunchList {
  std::vector<Rec> recs;        // grouped by launch
  std::vector<uint32_t> prefix; // n_recs + 1 values per launch
  std::vector<Launch> launches;
  // bytes of the image's sections (each a 16-byte multiple)
  size_t recs_bytes() const { return recs.size() * sizeof(Rec); }
  size_t prefix_bytes() const { return (prefix.size() * sizeof(uint32_t) + 15) / 16 * 16; }
  // both sections into `buf`: the records, the prefixes, zeros up to the prefixes' 16-byte multiple
  void write_image(char *buf) const {
    const size_t used = prefix.size() * sizeof(uint32_t);
    if (!recs.empty()) std::memcpy(buf, recs.data(), recs_bytes());
    if (used) std::memcpy(buf + recs_bytes(), prefix.data(), used);
    std::memset(buf + recs_bytes() + used, 0, prefix_bytes() - used);
  }

  // block_cap > 0: an add() that would take the open launch's grid past it closes the launch and opens the next of its class
  void clear(int64_t block_cap = 0) {
    recs.clear();
    prefix.clear();
    launches.clear();
    cap = block_cap;
    is_open = false;
  }
  void open(const Launch &header) {
    cur = header;
    cur.first_rec = (uint32_t)recs.size();
    cur.prefix_off = (uint32_t)prefix.size();
    cur.n_recs = cur.blocks = 0;
    is_open = true;
  }
  uint32_t open_blocks() const { return cur.blocks; } // the first block of the record add() is given next
  void add(const Rec &r, uint32_t blocks) {
    if (cap && cur.n_recs && (int64_t)cur.blocks + blocks > cap) {
      close();
      open(Launch(cur));
    }
    recs.push_back(r);
    prefix.push_back(cur.blocks);
    cur.blocks += blocks;
    ++cur.n_recs;
  }
  void close() { // (a launch without records leaves nothing)
    if (is_open && cur.n_recs) {
      prefix.push_back(cur.blocks);
      launches.push_back(cur);
    }
    is_open = false;
  }

private:
  Launch cur = {};
  int64_t cap = 0;
  bool is_open = false;
};

} // namespace fcpgp
