// plan_desc_san.cc — the descriptor unit of the library (recom_amd/csrc/fcp_plan_desc.cc) on its own, for a build with
// -fsanitize=address,undefined: linked with that one unit and nothing else, no GPU runtime.
//
//   plan_desc_san CASES PLAN...
//
// CASES: the refusal matrix of tests/plan_refusal_cases.py as text (write_cases there); per case check_desc must answer
// the recorded status and message.  Every PLAN (a column-plan file) must load with FCP_OK, and every proper prefix of it,
// written to PLAN.prefix, with FCP_OK or FCP_ERR_INVALID_ARGUMENT and nothing else: the parser reads untrusted text.
// Exit status 0 and no sanitizer report are the pass.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "fcp_plan_desc.h"

// Plan creation proper needs the GPU runtime; here its descriptor entry point stands in for it: what a loaded file is handed
// to is what fcp_plan_create_ex does with a descriptor first.
extern "C" int fcp_plan_create_ex(const fcp_plan_desc_t *desc, const fcp_column_ext_t *ext, fcp_plan_t **) {
  fcph::PlanFacts facts;
  return fcph::check_desc(desc, ext, &facts);
}

static int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      std::fprintf(stderr, __VA_ARGS__);     \
      std::fputc('\n', stderr);              \
      ++failures;                            \
    }                                        \
  } while (0)

static void run_cases(const char *path) {
  std::ifstream in(path);
  int n_cases = 0, n_host = 0;
  in >> n_cases >> n_host;
  std::vector<int32_t> ranks(n_host), esz(n_host);
  for (int i = 0; i < n_host; ++i) in >> ranks[i] >> esz[i];
  CHECK(in.good() && n_cases > 0, "%s: bad header", path);
  for (int i = 0; i < n_cases && in.good(); ++i) {
    std::string name, message;
    long long flags = 0;
    int n_cols = 0, want = 0;
    fcp_plan_desc_t d;
    std::memset(&d, 0, sizeof(d));
    in >> name >> flags >> d.layout >> d.shard_world >> d.n_device_inputs >> d.n_symbols >> n_cols >> want;
    std::vector<fcp_column_desc_t> cols(n_cols);
    std::vector<fcp_column_ext_t> ext(n_cols);
    for (int k = 0; k < n_cols; ++k) {
      fcp_column_desc_t &c = cols[k];
      std::memset(&c, 0, sizeof(c));
      std::memset(&ext[k], 0, sizeof(ext[k]));
      long long vocab = 0;
      in >> c.form >> c.combiner >> c.dim >> c.id_source >> vocab >> c.table_input >> c.ids_input >> c.seg_input >> c.seg_kind >> c.seg_stride >>
          c.rows_source >> c.rows_arg >> c.concat_group >> c.concat_slot >> ext[k].weights_input1 >> ext[k].table_kind1;
      c.vocab = vocab;
    }
    std::getline(in, message); // the rest of the numbers' line
    std::getline(in, message);
    CHECK(!in.fail(), "%s: case %d is malformed", path, i);
    d.abi_version = FCP_ABI_VERSION;
    d.n_columns = n_cols;
    d.columns = cols.data();
    d.n_host_inputs = n_host;
    d.host_input_ranks = ranks.data();
    d.host_input_elem_sizes = esz.data();
    d.n_groups = 1;
    d.flags = (uint32_t)flags;
    fcph::PlanFacts facts;
    const int rc = fcph::check_desc(&d, ext.data(), &facts);
    CHECK(rc == want && (rc == FCP_OK || message == fcp_last_error()), "%s: status %d (%s), recorded %d (%s)", name.c_str(), rc,
          rc ? fcp_last_error() : "", want, message.c_str());
    if (rc == FCP_OK)
      CHECK(!(facts.flags & FCP_FLAG_TABLES_PER_INPUT) && facts.col_kind.size() == (facts.tab_kind == FCP_TAB_MIXED ? (size_t)n_cols : 0),
            "%s: facts are not canonical", name.c_str());
  }
}

static int load(const char *path) {
  fcp_plan_t *plan = nullptr;
  const int rc = fcp_plan_create_from_file(path, 0, FCP_FLAG_HOST_ONLY, &plan);
  int32_t n = 0, sym = 0, rows[64];
  uint8_t modes[64];
  const int rc2 = fcp_plan_file_stage_info(path, &n, modes, rows, 64, &sym);
  CHECK(rc2 == FCP_OK || rc2 == FCP_ERR_INVALID_ARGUMENT, "%s: fcp_plan_file_stage_info answers %d", path, rc2);
  return rc;
}

static void run_plan(const char *path) {
  std::ifstream in(path, std::ios::binary);
  std::stringstream buf;
  buf << in.rdbuf();
  const std::string text = buf.str();
  CHECK(!text.empty(), "%s: empty or unreadable", path);
  const int whole = load(path);
  CHECK(whole == FCP_OK, "%s: status %d (%s)", path, whole, fcp_last_error());
  const std::string prefix_path = std::string(path) + ".prefix";
  for (size_t n = 0; n < text.size(); ++n) {
    std::ofstream(prefix_path, std::ios::binary | std::ios::trunc).write(text.data(), (std::streamsize)n);
    const int rc = load(prefix_path.c_str());
    CHECK(rc == FCP_OK || rc == FCP_ERR_INVALID_ARGUMENT, "%s: the first %zu bytes answer status %d (%s)", path, n, rc, fcp_last_error());
  }
  std::remove(prefix_path.c_str());
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  run_cases(argv[1]);
  for (int i = 2; i < argc; ++i) run_plan(argv[i]);
  CHECK(load((std::string(argv[1]) + ".absent").c_str()) == FCP_ERR_INVALID_ARGUMENT, "a missing file is an invalid argument");
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
