// plan_shape_san.cc — the host half of the plan (recom_amd/csrc/fcp_plan_shape.cc) on its own, for a build with
// -fsanitize=address,undefined: linked with that unit and fcp_plan_desc.cc and nothing else, no GPU runtime.
//
//   plan_shape_san REQUESTS
//
// REQUESTS (tests/plan_shape_cases.py, write_requests): a count, then per request
//   name  plan-file  FCP_SEG_SEARCH_MAX_PAIRS-or--1  concated_bytes  n_offsets offsets...  n_shapes shapes...  n_symbols-or--1 symbols...
// Every plan file is loaded as a host-only plan and the request evaluated with evaluate_shapes; status, message and every
// field of the records, the arena layout and the launch geometry are printed, one "key values..." line each, for the test
// to compare with its restatement.  Exit status 0 and no sanitizer report are the pass.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "fcp_plan_shape.h"

struct fcp_plan : fcph::HostPlan {};

// Plan creation proper needs the GPU runtime; here it is what fcp_plan_create_ex does before it touches a device.
extern "C" int fcp_plan_create_ex(const fcp_plan_desc_t *desc, const fcp_column_ext_t *ext, fcp_plan_t **out) {
  fcph::PlanFacts facts;
  int rc = fcph::check_desc(desc, ext, &facts);
  if (rc) return rc;
  fcp_plan *p = new fcp_plan();
  rc = fcph::build_host_plan(desc, ext, facts, p);
  if (rc) {
    delete p;
    return rc;
  }
  *out = p;
  return FCP_OK;
}

static std::vector<int32_t> read_list(std::ifstream &in, bool *absent = nullptr) {
  long long n = 0;
  in >> n;
  if (absent) *absent = n < 0;
  std::vector<int32_t> v(n > 0 ? (size_t)n : 0);
  for (auto &x : v) in >> x;
  return v;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  int n_cases = 0;
  in >> n_cases;
  for (int i = 0; i < n_cases; ++i) {
    std::string name, path;
    long long max_pairs = -1, blob_bytes = -1;
    in >> name >> path >> max_pairs >> blob_bytes;
    const std::vector<int32_t> offsets = read_list(in), shapes = read_list(in);
    bool no_symbols = false;
    const std::vector<int32_t> symbols = read_list(in, &no_symbols);
    if (in.fail()) {
      std::fprintf(stderr, "request %d is malformed\n", i);
      return 2;
    }
    if (max_pairs >= 0)
      setenv("FCP_SEG_SEARCH_MAX_PAIRS", std::to_string(max_pairs).c_str(), 1);
    else
      unsetenv("FCP_SEG_SEARCH_MAX_PAIRS");
    fcp_plan_t *p = nullptr;
    int rc = fcp_plan_create_from_file(path.c_str(), 0, FCP_FLAG_HOST_ONLY, &p);
    if (rc) {
      std::fprintf(stderr, "%s: %s does not load: %d (%s)\n", name.c_str(), path.c_str(), rc, fcp_last_error());
      return 2;
    }
    if (offsets.size() != p->ranks.size() || (int)shapes.size() != p->rank_sum || (!no_symbols && (int)symbols.size() != p->desc.n_symbols)) {
      std::fprintf(stderr, "%s: the request does not fit the plan\n", name.c_str());
      return 2;
    }
    const size_t nc = p->cols.size();
    // (exact sizes, no slack: a record or a weight written out of place is the sanitizer's to find)
    std::vector<FcpColDyn> dyn(nc);
    std::vector<int64_t> wts(p->has_weights ? nc : 0);
    fcph::DynMeta m;
    rc = fcph::evaluate_shapes(*p, offsets.data(), shapes.data(), no_symbols ? nullptr : symbols.data(), blob_bytes, dyn.data(),
                               p->has_weights ? wts.data() : nullptr, &m);
    std::printf("case %s\nstatus %d\n", name.c_str(), rc);
    if (rc) {
      std::printf("message %s\n", fcp_last_error());
    } else {
      for (size_t pos = 0; pos < nc; ++pos) {
        const FcpColDyn &d = dyn[pos];
        std::printf("dyn.%zu %lld %lld %lld %d %d %d %d %d %d\n", pos, (long long)d.ids_off, (long long)d.seg_off, (long long)d.out_base,
                    d.out_stride, d.nnz, d.csr_base, d.inner, d.rows, d.seg_sym);
      }
      if (p->has_weights) {
        std::printf("wts");
        for (int64_t w : wts) std::printf(" %lld", (long long)w);
        std::printf("\n");
      }
      const int ng = p->desc.n_groups;
      std::printf("group_rows");
      for (int g = 0; g < ng; ++g) std::printf(" %d", m.group_rows[g]);
      std::printf("\ngroup_base");
      for (int g = 0; g < ng; ++g) std::printf(" %lld", (long long)m.group_base[g]);
      std::printf("\narena_bytes %lld\ncsr_arena_off %lld\nmax_seg_nnz %d\nmax_lookup_nnz %d\nseg_pairs %lld\nseg_search %d\n",
                  (long long)m.arena_bytes, (long long)m.csr_arena_off, m.max_seg_nnz, m.max_lookup_nnz, (long long)m.seg_pairs, m.seg_search ? 1 : 0);
      std::printf("csr_reg %d %d %lld\nwork_bytes %lld\n", m.csr_reg_mode, m.csr_reg_stride, (long long)m.csr_reg_base, (long long)m.work_bytes);
      for (int kind = 0; kind < 2; ++kind) {
        std::printf("geo.%d %d %d\n", kind, m.geo[kind].rows_per_wave, m.geo[kind].grid_blocks);
        for (int g = 0; g < ng; ++g) {
          const FcpGroupLaunch &G = m.geo[kind].groups[g];
          std::printf("geo.%d.%d %d %d %d %d %d %d %d\n", kind, g, G.rows, G.nslots, G.nlist, G.span_list_off, G.nsp8, G.block_begin, G.slot_map_off);
        }
      }
    }
    delete p;
  }
  std::printf("end %d\n", n_cases);
  return 0;
}
