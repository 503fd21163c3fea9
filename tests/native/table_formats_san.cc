// table_formats_san.cc — fcp_table_formats_choose (recom_amd/csrc/fcp_plan_desc.cc) on its own, for a build with
// -fsanitize=address,undefined: linked with that one unit and nothing else, no GPU runtime.
//
//   table_formats_san CASES
//
// CASES: the chooser's instances of tests/table_audit_cases.py as text (write_instances there).  Per case one line on stdout:
// `status bytes error kinds...` (error as a C99 hex float; after a status other than FCP_OK: `status bytes`), which the test
// compares with what the library answers through ctypes.  Checked here as well: an FCP_OK answer lies within the budget, its
// bytes and error are those of its kinds, and a second call answers the same.  Exit status 0 and no sanitizer report are the pass.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "fcp_plan_desc.h"

// (the unit's plan-file entry refers to plan creation, which needs the GPU runtime; nothing here reaches it)
extern "C" int fcp_plan_create_ex(const fcp_plan_desc_t *, const fcp_column_ext_t *, fcp_plan_t **) { return FCP_ERR_UNSUPPORTED; }

static double hex_double(std::ifstream &in) {
  std::string s;
  in >> s;
  return std::strtod(s.c_str(), nullptr);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  int failures = 0, n = 0, has_weights = 0;
  unsigned allowed = 0;
  long long budget = 0;
  while (in >> n >> allowed >> has_weights >> budget) {
    std::vector<fcp_table_audit_t> audits(n);
    std::vector<int64_t> rows(n);
    std::vector<int32_t> dims(n);
    std::vector<double> weights(n);
    for (int t = 0; t < n; ++t) {
      long long r = 0, nonfinite = 0;
      in >> r >> dims[t] >> nonfinite;
      fcp_table_audit_t a = {};
      a.rows = rows[t] = r;
      a.rows_nonfinite = nonfinite;
      a.first_nonfinite_row = nonfinite ? 0 : -1;
      a.sum_sq = hex_double(in);
      a.kind[0].first_bad_row = -1;
      for (int k = 1; k < 4; ++k) {
        long long bad = 0;
        in >> bad;
        a.kind[k].rows_bad = bad;
        a.kind[k].first_bad_row = bad ? 0 : -1;
        a.kind[k].sum_sq_err = hex_double(in);
      }
      weights[t] = hex_double(in);
      audits[t] = a;
    }
    std::vector<int32_t> kinds(n, -1), again(n, -1);
    int64_t bytes = -1, bytes2 = -1;
    double error = -1.0, error2 = -1.0;
    const double *w = has_weights ? weights.data() : nullptr;
    const int status = fcp_table_formats_choose(audits.data(), rows.data(), dims.data(), n, budget, allowed, w, kinds.data(), &bytes, &error);
    const int status2 = fcp_table_formats_choose(audits.data(), rows.data(), dims.data(), n, budget, allowed, w, again.data(), &bytes2, &error2);
    if (status != status2 || bytes != bytes2 || (status == FCP_OK && (kinds != again || error != error2))) ++failures;
    if (status != FCP_OK) {
      if (status != FCP_ERR_UNSUPPORTED || bytes <= budget) ++failures;
      std::printf("%d %lld\n", status, (long long)bytes);
      continue;
    }
    int64_t sum = 0;
    for (int t = 0; t < n; ++t) {
      if (kinds[t] < 0 || kinds[t] > 3) {
        ++failures;
        continue;
      }
      sum += rows[t] * fcpf::row_bytes(kinds[t], dims[t]);
    }
    if (sum != bytes || bytes > budget) ++failures;
    std::printf("%d %lld %a", status, (long long)bytes, error);
    for (int t = 0; t < n; ++t) std::printf(" %d", kinds[t]);
    std::printf("\n");
  }
  // the argument checks, null pointers included
  int32_t kind = 0;
  int64_t one = 1;
  int32_t dim = 4;
  fcp_table_audit_t a = {};
  if (fcp_table_formats_choose(nullptr, nullptr, nullptr, 0, 0, 15, nullptr, nullptr, nullptr, nullptr) != FCP_OK) ++failures;
  if (fcp_table_formats_choose(nullptr, &one, &dim, 1, 100, 15, nullptr, &kind, nullptr, nullptr) != FCP_ERR_INVALID_ARGUMENT) ++failures;
  if (fcp_table_formats_choose(&a, &one, &dim, -1, 100, 15, nullptr, &kind, nullptr, nullptr) != FCP_ERR_INVALID_ARGUMENT) ++failures;
  if (fcp_table_formats_choose(&a, &one, &dim, 1, -1, 15, nullptr, &kind, nullptr, nullptr) != FCP_ERR_INVALID_ARGUMENT) ++failures;
  if (fcp_table_formats_choose(&a, &one, &dim, 1, 100, 15, nullptr, &kind, nullptr, nullptr) != FCP_OK || kind != FCP_TAB_F32) ++failures;
  if (failures) std::fprintf(stderr, "%d failures\n", failures);
  return failures ? 1 : 0;
}
