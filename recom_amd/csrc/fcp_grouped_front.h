// fcp_grouped_front.h — the two halves of the grouped table entries' front seen together: the device's search
// (fcp_find_piece.h) and the host's launch list (fcp_grouped_plan.h).  What one relies on of the other is asserted here, once,
// for every unit that launches over a fcpgp::LaunchList (fcp_tables_rows.hip, fcp_tables_digest.hip).
#pragma once
#include "fcp_find_piece.h"
#include "fcp_grouped_plan.h"

static_assert(fcpgp::kMaxLaunchRecs <= (1 << kSearchSteps), "find_piece's steps reach every record of a launch");
