// fcp_formats.h — the storage formats of tables (FCP_TAB_*) and outputs (FCP_OUT_*): ONE table of their facts and the small
// functions every host-side unit derives the rest from.  Plain C++, no GPU header.  A new format is one row here and one
// refusal subject in fcp_plan_desc.cc.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/fcp_hip.h"

namespace fcpf {

struct Format {
  const char *name;   // in a plan file
  uint32_t flag;      // the plan-wide bit of fcp_plan_desc_t::flags, 0 for float32
  int elem, row_tail; // bytes of one element; bytes behind the elements of a row (q8: float32 scale, float32 bias)
};
constexpr int kTabKinds = 4, kOutKinds = 3;
constexpr Format kTab[kTabKinds] = {{"f32", 0, 4, 0}, {"bf16", FCP_FLAG_TABLES_BF16, 2, 0}, {"f16", FCP_FLAG_TABLES_F16, 2, 0}, {"q8", FCP_FLAG_TABLES_Q8, 1, 8}};
constexpr Format kOut[kOutKinds] = {{"f32", 0, 4, 0}, {"bf16", FCP_FLAG_OUT_BF16, 2, 0}, {"f16", FCP_FLAG_OUT_F16, 2, 0}};
static_assert(FCP_TAB_F32 == 0 && FCP_TAB_BF16 == 1 && FCP_TAB_F16 == 2 && FCP_TAB_Q8 == 3 && FCP_OUT_F32 == 0 && FCP_OUT_BF16 == 1 && FCP_OUT_F16 == 2,
              "kTab is indexed by FCP_TAB_*, kOut by FCP_OUT_*");
constexpr int64_t kRowLimit = (1ll << 32) - 3; // a plan's row limit: the rows of a table, and of one call of a table entry, stay below it
constexpr uint32_t kTabFlags = FCP_FLAG_TABLES_BF16 | FCP_FLAG_TABLES_F16 | FCP_FLAG_TABLES_Q8, kOutFlags = FCP_FLAG_OUT_BF16 | FCP_FLAG_OUT_F16;

inline bool known_tab_kind(int kind) { return kind >= 0 && kind < kTabKinds; } // (FCP_TAB_MIXED is no row format)
// bytes of one row of `dim` elements; rows lie back to back in every format
inline int64_t row_bytes(int kind, int dim) { return (int64_t)dim * kTab[kind].elem + kTab[kind].row_tail; }
// the base alignment a plan asks of a table of `kind` whose rows are read `vec` elements at a time (q8: its tail's floats)
inline int base_alignment(int kind, int vec) { return kTab[kind].row_tail ? 4 : kTab[kind].elem * vec; }
// How the table kernels walk a float32 row (fcp_table_walk.h): V elements per lane and access, G lanes per row of a q8 row.
// V: the largest of 4 | 2 | 1 that divides dim
inline int vec_of(int32_t dim) { return dim % 4 == 0 ? 4 : dim % 2 == 0 ? 2 : 1; }
// G, the lanes that share a row: 1 for dims <= 4, else the power of two that holds the row's dim / V slots, at most 64
inline int group_of(int dim, int vec) {
  int g = 1;
  if (dim > 4)
    while (g < dim / vec && g < 64) g <<= 1;
  return g;
}
// a kind in a refusal's text
inline const char *kind_name(int32_t k) { return k == FCP_TAB_F32 ? "float32" : k == FCP_TAB_BF16 ? "bf16" : k == FCP_TAB_F16 ? "fp16" : "q8"; }

// Refusals the table entries share, to go behind the entry's "name: " (the host tests assert the sentences).
// `name` lies at an address that is no multiple of align; what: " (...)" or nothing
inline std::string not_aligned(const char *name, int align, const std::string &what = std::string()) {
  return std::string("`") + name + "` is not " + std::to_string(align) + "-byte aligned" + what;
}
// a call's count `name` (n: ids or rows) and the table's rows against kRowLimit; empty when both pass
inline std::string row_limit_refusal(const char *name, int64_t n, int64_t table_rows) {
  if (n >= kRowLimit) return std::string("`") + name + "` must stay below 2^32 - 3";
  if (table_rows < 1 || table_rows >= kRowLimit) return "`table_rows` must lie in [1, 2^32 - 3), a plan's row limit";
  return std::string();
}

// the kind the plan-wide flag bits name: float32 without a bit, -1 for two bits at once
inline int kind_of_flags(const Format *t, int n, uint32_t bits) {
  for (int k = 0; k < n; ++k)
    if (bits == t[k].flag) return k;
  return -1;
}
inline int tab_kind_of_flags(uint32_t flags) { return kind_of_flags(kTab, kTabKinds, flags & kTabFlags); }
inline int out_kind_of_flags(uint32_t flags) { return kind_of_flags(kOut, kOutKinds, flags & kOutFlags); }
// plan-file name -> kind, -1 for a name that is none
inline int kind_of_name(const Format *t, int n, const char *name) {
  for (int k = 0; k < n; ++k)
    if (!std::strcmp(name, t[k].name)) return k;
  return -1;
}
inline int tab_kind_of_name(const char *name) { return kind_of_name(kTab, kTabKinds, name); }
inline int out_kind_of_name(const char *name) { return kind_of_name(kOut, kOutKinds, name); }

} // namespace fcpf
