// fcp_plan_desc.h — the descriptor level of the library (fcp_plan_desc.cc): what a plan IS, decided before any GPU call.
// No GPU header: the unit is ordinary C++ and can be linked, and tested under sanitizers, without the HIP runtime.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fcp_hip.h"
#include "fcp_formats.h"
#include "fcp_internal.h"

namespace fcph {

// sets fcp_last_error for this thread and returns `code`
int fail(int code, const std::string &msg);

// What check_desc learns from a descriptor that passed: everything format-dependent that plan creation needs.
struct PlanFacts {
  uint32_t flags = 0;           // the descriptor's flags, canonical: FCP_FLAG_TABLES_PER_INPUT resolved away
  int out_kind = FCP_OUT_F32;   // FCP_OUT_*
  int tab_kind = FCP_TAB_F32;   // FCP_TAB_*; FCP_TAB_MIXED when the tables really differ
  std::vector<int8_t> col_kind; // tables that really differ: FCP_TAB_* per plan column (FCP_TAB_F32 without a table); else empty
  FcpVariant variant = FCP_VAR_F32;
};

// The one descriptor entry point of plan creation: validates `d` (and `ext`, when given), turns per-input table formats
// whose tables all share one kind into the plan-wide plan of that kind, and refuses by name what the kernels of the plan's
// format do not serve — for device and host-only plans alike.
int check_desc(const fcp_plan_desc_t *d, const fcp_column_ext_t *ext, PlanFacts *facts);

} // namespace fcph
