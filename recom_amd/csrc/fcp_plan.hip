// fcp_plan.hip — the device half of the plan object (the non-codegen half of the reference's CudaEmitter): const buffers
// (CreateConstBuffers, cuda_emitter.cc:2260-2301), static column records, device resources, accessors.  The descriptor is
// checked by fcp_plan_desc.cc; the host half of the plan and the shape-dependent column records + launch geometry are
// fcp_plan_shape.cc's.  Carved out of fcp_api.hip in round 6 (see fcp_host.h); the original header comment follows.
//
// (was fcp_api.hip) — host side of libfcp_hip.so: the C ABI declared in
// include/fcp_hip.h.  Plan building (the non-codegen half of the reference's
// CudaEmitter), const buffers (CreateConstBuffers, cuda_emitter.cc:2260-2301),
// the per-request entry (ProcessFeatureColumns, :2303-2494, and its kernel
// caller :2139-2258) and the host packer of Addons>ConcatInputs
// (custom_ops/concat_inputs/concat_inputs_ops.cc:42-77).
//
// Differences from the reference's per-request host work, on purpose:
//   * no blocking stream synchronisation anywhere on the request path (the
//     reference blocks at :2246 and twice more in the ops);
//   * no per-request H2D of a pageable argument struct (:2216): the shape-
//     dependent descriptors are cached on the device keyed by the request's
//     (offsets, shapes, symbols) and re-uploaded from pinned memory only when
//     the shapes change;
//   * 64-bit byte offsets and row offsets (the reference's int arithmetic
//     overflows beyond 2^31).
#include "fcp_host.h"
#include "fcp_plain_map.h"

namespace fcph {

int hip_fail(const char *what, hipError_t e) {
  return fail((e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu || e == hipErrorInsufficientDriver)
                  ? FCP_ERR_NO_DEVICE
                  : FCP_ERR_HIP,
              std::string(what) + ": " + hipGetErrorString(e));
}

// Are the boundaries evenly spaced closely enough that floor((x - b0) * inv) + 1 names the right bucket
// for x at every boundary and just below it (the places where rounding could push the guess over)?  Then
// the kernels take the guess and verify it with two reads instead of a 7-step binary search.  The guess is
// only a starting point — a failed verification falls back to the search — so this is a speed decision.
void uniform_boundaries(const std::vector<float> &b, float *b0, float *inv, float *step_out) {
  const int n = (int)b.size();
  if (n < 2 || !(b[n - 1] > b[0])) return;
  const float lo = b[0];
  const float scale = (float)((double)(n - 1) / ((double)b[n - 1] - (double)b[0]));
  if (!(scale > 0.0f) || !std::isfinite(scale)) return;
  auto guess = [&](float x) {
    float t = (x - lo) * scale;
    t = std::fmin(std::fmax(t, -1.0f), (float)n);
    int g = (int)std::floor(t) + 1;
    return std::min(std::max(g, 0), n);
  };
  auto exact = [&](float x) { return (int)(std::upper_bound(b.begin(), b.end(), x) - b.begin()); };
  int misses = 0;
  for (int i = 0; i < n; ++i) {
    if (i && !(b[i] > b[i - 1])) return; // not strictly increasing
    const float below = std::nextafter(b[i], -INFINITY);
    misses += guess(b[i]) != exact(b[i]);
    misses += guess(below) != exact(below);
  }
  if (misses * 8 > n) return; // an occasional miss costs one fallback search; many mean the spacing is not even
  *b0 = lo;
  *inv = scale;
  // Reproducible boundaries: b[i] == fma(i, step, b0) bit for bit (one correctly rounded operation on the host
  // and on the GPU alike).  Holds for the reference's 0, 5, ..., 495 and for any integer / dyadic grid.
  const float step = b[1] - b[0];
  if (!(step > 0.0f) || !std::isfinite(step)) return;
  for (int i = 0; i < n; ++i)
    if (std::fmaf((float)i, step, lo) != b[i]) return;
  *step_out = step;
}

// Plain dense plans (fcp_dense_plain.hip): the gate, and the per-span image with everything that is known now — the
// lane -> column maps and the columns' static facts; table addresses, id-stream offsets and the id facts (all
// FCP_PLAIN_FACT_NONE here) are filled in per descriptor slot (fill_plain_image).  Called once the static records exist (their boundary constants are the image's).
void build_plain_template(fcp_plan *p) {
  p->plain_dense = false;
  // FCP_DIAG=dense_generic: a qualifying plan stays on the generic kernel (the tests' seam)
  if (fcp::diag_ll("dense_generic", 0) != 0) return;
  // FCP_DIAG=plain_even_deal=0|1: the block mapping of the plain kernel's partial last group (the A/B's seam)
  p->plain_even_deal = fcp::diag_ll("plain_even_deal", FCP_PLAIN_EVEN_DEAL_DEFAULT) != 0;
  // FCP_DIAG=store_policy=sc1: the plain kernel's launches store `sc1` whatever the rule says (store_policy_for)
  if (const char *v = fcp::diag("store_policy")) p->plain_store_sc1 = !std::strcmp(v, "sc1");
  const fcp_plan_desc_t &d = p->desc;
  if (p->out_elem != 4 || p->tab_elem != 4 || d.layout != FCP_LAYOUT_CONCAT || d.n_groups != 1 || d.shard_world > 1 || p->vec != 4 || p->wide_rows ||
      p->weighted_kernel || !p->dense_only || p->cols.empty())
    return;
  const int nc = (int)p->cols.size();
  for (int pos = 0; pos < nc; ++pos) {
    const HostColumn &hc = p->cols[p->order[pos]];
    const FcpColStatic &s = p->h_cols[pos];
    if (hc.d.form != FCP_FORM_GATHER || s.xform != 0 || hc.d.vocab < 0 || hc.d.vocab >= 0xFFFFFFFDLL) return;
    if (hc.d.id_source == FCP_IDS_F32_BUCKETIZE) {
      if (s.bnd_step == 0.0f) return; // boundaries that are read (staged in LDS or searched in L2): the generic body's
    } else if (hc.d.id_source != FCP_IDS_I32 && hc.d.id_source != FCP_IDS_I64) {
      return;
    }
  }
  const int nslots = p->group_nslots[0];
  const int nspans = (nslots + FCP_WAVE - 1) / FCP_WAVE;
  if (p->list_n[0][0] != nspans) return;
  // columns per span (concat order: a span's columns are consecutive positions)
  std::vector<int> first(nspans, nc), last(nspans, -1);
  for (int pos = 0; pos < nc; ++pos) {
    const FcpColStatic &s = p->h_cols[pos];
    const int s0 = s.out_off / 4 / FCP_WAVE, s1 = (s.out_off + s.dim - 1) / 4 / FCP_WAVE;
    for (int sp = s0; sp <= s1; ++sp) {
      first[sp] = std::min(first[sp], pos);
      last[sp] = std::max(last[sp], pos);
    }
  }
  int max_cols = 1;
  for (int sp = 0; sp < nspans; ++sp) max_cols = std::max(max_cols, last[sp] - first[sp] + 1);
  if (max_cols > FCP_WAVE) return; // (cannot happen: a column has at least one slot)
  p->plain_cols_off = FCP_PLAIN_FACTS_OFF + fcp_plain_facts_bytes(max_cols);
  p->plain_stride = (int32_t)(p->plain_cols_off + (size_t)max_cols * sizeof(FcpPlainCol));
  p->plain_spans = nspans;
  p->plain_tmpl.assign((size_t)nspans * p->plain_stride, 0);
  p->plain_entries.clear();
  for (int sp = 0; sp < nspans; ++sp) {
    char *rec = p->plain_tmpl.data() + (size_t)sp * p->plain_stride;
    FcpPlainSpan head;
    std::memset(&head, 0, sizeof(head));
    head.ncols = last[sp] - first[sp] + 1;
    head.cols_off = p->plain_cols_off;
    for (int pos = first[sp]; pos <= last[sp]; ++pos) {
      const FcpColStatic &s = p->h_cols[pos];
      FcpPlainCol c;
      std::memset(&c, 0, sizeof(c));
      c.table = nullptr;
      c.ids_off = 0;
      c.vocab = (uint32_t)s.vocab;
      c.spr = (uint32_t)(s.dim / 4);
      c.out_off = s.out_off;
      c.kind = FCP_F_IDSRC(s.flags);
      c.n_boundaries = s.n_boundaries;
      c.bnd_b0 = s.bnd_b0;
      c.bnd_inv = s.bnd_inv;
      c.bnd_step = s.bnd_step;
      const size_t at = (size_t)sp * p->plain_stride + p->plain_cols_off + (size_t)(pos - first[sp]) * sizeof(FcpPlainCol);
      std::memcpy(p->plain_tmpl.data() + at, &c, sizeof(c));
      p->plain_entries.emplace_back((uint32_t)at, pos);
      for (int q = std::max(s.out_off / 4, sp * FCP_WAVE); q < std::min((s.out_off + s.dim) / 4, (sp + 1) * FCP_WAVE); ++q)
        head.lane_col[q - sp * FCP_WAVE] = (uint8_t)(pos - first[sp]);
    }
    std::memcpy(rec, &head, sizeof(head));
  }
  p->plain_dense = true;
}

void destroy_device(fcp_plan *p) {
  if (p->host_only) return;
  for (auto &s : p->slots) {
    if (s.h_dyn) (void)hipHostFree(s.h_dyn);
    if (s.d_dyn) (void)hipFree(s.d_dyn);
    if (s.uploaded) (void)hipEventDestroy(s.uploaded);
    for (auto &e : s.done_pool) (void)hipEventDestroy(e.second);
  }
  if (p->d_slot_map) (void)hipFree(p->d_slot_map);
  if (p->d_span_list) (void)hipFree(p->d_span_list);
  if (p->d_cols) (void)hipFree(p->d_cols);
  if (p->d_xforms) (void)hipFree(p->d_xforms);
  if (p->d_segmaps) (void)hipFree(p->d_segmaps);
  if (p->d_const) (void)hipFree(p->d_const);
  if (p->d_seg_cols) (void)hipFree(p->d_seg_cols);
  if (p->d_bad) (void)hipFree(p->d_bad);
  if (p->d_zeros) (void)hipFree(p->d_zeros);
  if (p->d_traffic) (void)hipFree(p->d_traffic);
}

int init_device(fcp_plan *p) {
  DeviceGuard guard;
  int rc = guard.enter(p->desc.device);
  if (rc) return rc;
  const int nc = (int)p->cols.size();
  // slot map: slot -> position in the concat-ordered column arrays (group g's part begins at group_map_off[g])
  std::vector<uint32_t> map;
  for (int g = 0; g < p->desc.n_groups; ++g) {
    for (int pos = 0; pos < nc; ++pos) {
      const HostColumn &hc = p->cols[p->order[pos]];
      if (hc.d.concat_group != g) continue;
      for (int s = 0; s < hc.d.dim / p->vec; ++s) map.push_back((uint32_t)pos);
    }
  }
  HIP_TRY(hipMalloc(&p->d_span_list, std::max<size_t>(p->span_list.size(), 1) * sizeof(uint32_t)));
  HIP_TRY(hipMemcpy(p->d_span_list, p->span_list.data(), p->span_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&p->d_slot_map, std::max<size_t>(map.size(), 1) * sizeof(uint32_t)));
  HIP_TRY(hipMemcpy(p->d_slot_map, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  // const buffers (bucketize boundaries), each 128-byte aligned as the reference's
  // identical boundary arrays (the usual case: hundreds of bucketized features with one
  // boundary list) are stored once, so that neighbouring columns can share one LDS copy
  int64_t const_bytes = 0;
  std::vector<int> owners; // indices of columns whose array was stored
  for (size_t k = 0; k < p->cols.size(); ++k) {
    HostColumn &hc = p->cols[k];
    if (hc.boundaries.empty()) continue;
    for (int o : owners)
      if (p->cols[o].boundaries == hc.boundaries) {
        hc.const_off = p->cols[o].const_off;
        break;
      }
    if (hc.const_off < 0) {
      hc.const_off = const_bytes;
      const_bytes += align128((int64_t)hc.boundaries.size() * 4);
      owners.push_back((int)k);
    }
  }
  for (HostColumn &hc : p->cols) { // id transform intervals beyond the first (the first one travels in the record)
    if (hc.xf_lo.size() <= 1) continue;
    hc.xf_const_off = const_bytes;
    const_bytes += align128((int64_t)(hc.xf_lo.size() - 1) * 16);
  }
  if (const_bytes) {
    HIP_TRY(hipMalloc(&p->d_const, const_bytes));
    for (const HostColumn &hc : p->cols) {
      if (hc.xf_const_off < 0) continue;
      std::vector<int64_t> pairs;
      for (size_t i = 1; i < hc.xf_lo.size(); ++i) {
        pairs.push_back(hc.xf_lo[i]);
        pairs.push_back(hc.xf_hi[i]);
      }
      HIP_TRY(hipMemcpy(p->d_const + hc.xf_const_off, pairs.data(), pairs.size() * 8, hipMemcpyHostToDevice));
    }
    for (int o : owners)
      HIP_TRY(hipMemcpy(p->d_const + p->cols[o].const_off, p->cols[o].boundaries.data(),
                        p->cols[o].boundaries.size() * 4, hipMemcpyHostToDevice));
  }
  // static column records (tables are bound on the first request)
  std::vector<FcpXform> h_xforms; // filled only if some column has an id transform
  p->h_cols.resize(nc);
  for (int pos = 0; pos < nc; ++pos) {
    const HostColumn &hc = p->cols[p->order[pos]];
    FcpColStatic &s = p->h_cols[pos];
    s.table = nullptr;
    s.boundaries = hc.const_off >= 0 ? reinterpret_cast<const float *>(p->d_const + hc.const_off) : nullptr;
    s.vocab = hc.d.vocab;
    s.dim = hc.d.dim;
    s.out_off = hc.out_off;
    s.flags = FCP_F_PACK(hc.d.form, hc.d.combiner, hc.d.id_source, hc.d.seg_kind);
    if (p->tab_mixed()) s.flags |= (uint32_t)p->col_kind[p->order[pos]] << 16; // FCP_F_TABKIND: read by the mixed-table kernels only
    s.n_boundaries = (int32_t)hc.boundaries.size();
    s.seg_stride = hc.d.seg_stride < 1 ? 1 : hc.d.seg_stride;
    s.bnd_b0 = 0.0f;
    s.bnd_inv = 0.0f;
    s.bnd_step = 0.0f;
    uniform_boundaries(hc.boundaries, &s.bnd_b0, &s.bnd_inv, &s.bnd_step);
    // id transform: an empty interval set (nothing is "in") is encoded as one impossible interval
    s.bnd_off = -1;
    s.xform = 0;
    if (hc.d.xform_mode != FCP_XFORM_NONE || hc.d.hash_buckets > 0) {
      if (h_xforms.empty()) {
        FcpXform none;
        none.lo0 = 1;
        none.hi0 = 0;
        none.sub = 0;
        none.extra = nullptr;
        none.hash_buckets = 0;
        none.pad_ = 0;
        h_xforms.assign(nc, none);
      }
      FcpXform &x = h_xforms[pos];
      if (hc.d.hash_buckets > 0) {
        s.xform |= FCP_XFORM_HASH_BIT;
        x.hash_buckets = hc.d.hash_buckets;
      }
      if (hc.d.xform_mode != FCP_XFORM_NONE) {
        const uint32_t n = (uint32_t)std::max<size_t>(hc.xf_lo.size(), 1);
        s.xform |= (n << 2) | (uint32_t)hc.d.xform_mode;
        x.sub = hc.d.xform_substitute;
        if (!hc.xf_lo.empty()) {
          x.lo0 = hc.xf_lo[0];
          x.hi0 = hc.xf_hi[0];
        }
        if (hc.xf_const_off >= 0) x.extra = reinterpret_cast<const int64_t *>(p->d_const + hc.xf_const_off);
      }
    }
  }
  build_plain_template(p); // (before the descriptor slots are sized: a plain dense plan's slots carry the span image)
  HIP_TRY(hipMalloc(&p->d_cols, nc * sizeof(FcpColStatic)));
  HIP_TRY(hipMemcpy(p->d_cols, p->h_cols.data(), nc * sizeof(FcpColStatic), hipMemcpyHostToDevice));
  if (!h_xforms.empty()) {
    HIP_TRY(hipMalloc(&p->d_xforms, nc * sizeof(FcpXform)));
    HIP_TRY(hipMemcpy(p->d_xforms, h_xforms.data(), nc * sizeof(FcpXform), hipMemcpyHostToDevice));
  }
  if (p->has_seg_map) {
    std::vector<FcpSegMap> h_maps(nc);
    for (int pos = 0; pos < nc; ++pos) {
      const fcp_column_ext_t &e = p->cols[p->order[pos]].ext;
      FcpSegMap &sm = h_maps[pos];
      for (int i = 0; i < 4; ++i) sm.mul[i] = i < e.seg_map_n ? e.seg_map_mul[i] : 0;
      sm.div = e.seg_map_n > 0 ? e.seg_map_div : 1;
      sm.n = e.seg_map_n;
      sm.sym_slot = e.seg_map_n > 0 && e.seg_map_sym >= 0 ? e.seg_map_sym_slot : -1;
    }
    HIP_TRY(hipMalloc(&p->d_segmaps, nc * sizeof(FcpSegMap)));
    HIP_TRY(hipMemcpy(p->d_segmaps, h_maps.data(), nc * sizeof(FcpSegMap), hipMemcpyHostToDevice));
  }
  if (!p->seg_cols.empty()) {
    std::vector<int32_t> seg_pos;
    for (int k : p->seg_cols) seg_pos.push_back(p->pos_of[k]);
    HIP_TRY(hipMalloc(&p->d_seg_cols, seg_pos.size() * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(p->d_seg_cols, seg_pos.data(), seg_pos.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  // (8-bit row-quantised tables: a skipped id reads zero codes AND, dim - e bytes behind them, a zero scale and bias: the
  // line is as long as the plan's longest row)
  size_t zero_bytes = 256;
  for (size_t k = 0; k < p->cols.size(); ++k)
    if (fcpf::kTab[p->col_tab_kind(k)].row_tail) zero_bytes = std::max(zero_bytes, (size_t)((p->col_row_bytes(k, p->cols[k].d.dim) + 255) / 256 * 256));
  HIP_TRY(hipMalloc(&p->d_zeros, zero_bytes));
  HIP_TRY(hipMemset(p->d_zeros, 0, zero_bytes));
  if (p->desc.flags & FCP_FLAG_COUNT_BAD_IDS) {
    HIP_TRY(hipMalloc(&p->d_bad, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(p->d_bad, 0, sizeof(unsigned long long)));
  }
  {
    int large_bar = 0;
    (void)hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, p->desc.device);
    p->host_writes_dyn = large_bar != 0 && !p->env.dyn_upload_kernel; // (FCP_DYN_UPLOAD=kernel)
  }
  for (auto &s : p->slots) {
    // rounded up to 16 bytes: the upload kernel moves uint4s
    const size_t dyn_bytes = (slot_dyn_bytes(p) + 15) / 16 * 16;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s.h_dyn), dyn_bytes, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer(&s.h_dyn_dev, s.h_dyn, 0));
    if (p->host_writes_dyn) {
      if (hipExtMallocWithFlags(reinterpret_cast<void **>(&s.d_dyn), dyn_bytes, hipDeviceMallocFinegrained) != hipSuccess) {
        (void)hipGetLastError();
        p->host_writes_dyn = false; // fall back for every slot: nothing has been used yet
        for (auto &t : p->slots)
          if (t.d_dyn) {
            (void)hipFree(t.d_dyn);
            t.d_dyn = nullptr;
          }
      }
    }
  }
  for (auto &s : p->slots) {
    const size_t dyn_bytes = (slot_dyn_bytes(p) + 15) / 16 * 16;
    if (!s.d_dyn) HIP_TRY(hipMalloc(&s.d_dyn, dyn_bytes));
    HIP_TRY(hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
    s.done = nullptr; // created per stream on first use (done_event_for)
  }
  p->bound_tables.assign(p->desc.n_device_inputs, nullptr);
  {
    // the gate at plan level (the reference's check_table_size, cuda_emitter.cc:1080-1094, decides per table
    // against 256 MiB): the tables this plan reads on this device must fit the device at all
    int64_t shard_bytes = 0;
    (void)fcp_plan_table_bytes(p, &shard_bytes, nullptr);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0 && (uint64_t)shard_bytes > total_b)
      return fail(FCP_ERR_UNSUPPORTED, "this plan's tables need " + std::to_string(shard_bytes) + " bytes on a device with " +
                                           std::to_string(total_b) + ": shard them over more GPUs (fcp_placement_decide)");
  }
  return FCP_OK;
}

} // namespace fcph

// =============================== C ABI ======================================
extern "C" {

// ---- plan ---------------------------------------------------------------------
int fcp_plan_create(const fcp_plan_desc_t *desc, fcp_plan_t **out) { return fcp_plan_create_ex(desc, nullptr, out); }

int fcp_plan_create_ex(const fcp_plan_desc_t *desc, const fcp_column_ext_t *ext, fcp_plan_t **out) {
  if (!out) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan out pointer");
  *out = nullptr;
  PlanFacts facts;
  int rc = check_desc(desc, ext, &facts);
  if (rc) return rc;
  fcp_plan *p = new (std::nothrow) fcp_plan();
  if (!p) return fail(FCP_ERR_ALLOC, "out of host memory");
  rc = build_host_plan(desc, ext, facts, p); // everything decided without a device (fcp_plan_shape.h)
  if (rc == FCP_OK) {
    p->last_launch.csr_base.reset(new std::atomic<int32_t>[p->cols.size() > 0 ? p->cols.size() : 1]);
    for (size_t k = 0; k < p->cols.size(); ++k) p->last_launch.csr_base[k].store(-1, std::memory_order_relaxed);
    if (!p->host_only) rc = init_device(p);
  }
  if (rc) {
    destroy_device(p); // (frees what init_device got as far as allocating: nothing before it ran)
    delete p;
    return rc;
  }
  *out = p;
  return FCP_OK;
}

int fcp_plan_counts(const fcp_plan_t *p, int32_t *n_columns, int32_t *n_groups, int32_t *n_host_inputs,
                    int32_t *n_device_inputs, int32_t *n_symbols) {
  if (!p) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan");
  if (n_columns) *n_columns = p->desc.n_columns;
  if (n_groups) *n_groups = p->desc.n_groups;
  if (n_host_inputs) *n_host_inputs = p->desc.n_host_inputs;
  if (n_device_inputs) *n_device_inputs = p->desc.n_device_inputs;
  if (n_symbols) *n_symbols = p->desc.n_symbols;
  return FCP_OK;
}

int fcp_plan_output_columns(const fcp_plan_t *p, int32_t *n, int32_t *indices, int32_t capacity) {
  if (!p) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan");
  int32_t count = 0;
  for (int32_t k = 0; k < (int32_t)p->cols.size(); ++k) {
    if (p->cols[k].d.form == FCP_FORM_EXTERNAL) continue;
    if (indices && count < capacity) indices[count] = k;
    ++count;
  }
  if (n) *n = count;
  return FCP_OK;
}

int fcp_plan_out_dtype(const fcp_plan_t *p, int32_t *out) {
  if (!p || !out) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  *out = p->out_kind;
  return FCP_OK;
}

int fcp_plan_table_dtype(const fcp_plan_t *p, int32_t *out) {
  if (!p || !out) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  *out = p->tab_kind;
  return FCP_OK;
}

int fcp_plan_table_kinds(const fcp_plan_t *p, int32_t *kinds, int32_t capacity, int32_t *n) {
  if (!p) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan");
  std::vector<int32_t> in_kind(p->desc.n_device_inputs, -1);
  for (size_t k = 0; k < p->cols.size(); ++k) {
    const int f = p->cols[k].d.form;
    if (f == FCP_FORM_GATHER || f == FCP_FORM_SEGMENT_REDUCE || f == FCP_FORM_GATHER_SCATTER) in_kind[p->cols[k].d.table_input] = p->col_tab_kind(k);
  }
  for (int32_t t = 0; t < p->desc.n_device_inputs && t < capacity; ++t)
    if (kinds) kinds[t] = in_kind[t];
  if (n) *n = p->desc.n_device_inputs;
  return FCP_OK;
}

int fcp_plan_table_rows(const fcp_plan_t *p, int64_t *rows, int32_t capacity, int32_t *n) {
  if (!p) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan");
  std::vector<int64_t> in_rows(p->desc.n_device_inputs, -1);
  for (size_t k = 0; k < p->cols.size(); ++k) {
    const int f = p->cols[k].d.form;
    if (f != FCP_FORM_GATHER && f != FCP_FORM_SEGMENT_REDUCE && f != FCP_FORM_GATHER_SCATTER) continue;
    int64_t &r = in_rows[p->cols[k].d.table_input];
    r = std::max(r, p->cols[k].d.vocab); // (columns that share a table need not agree on vocab: the largest)
  }
  for (int32_t t = 0; t < p->desc.n_device_inputs && t < capacity; ++t)
    if (rows) rows[t] = in_rows[t];
  if (n) *n = p->desc.n_device_inputs;
  return FCP_OK;
}

int fcp_plan_table_bytes(const fcp_plan_t *p, int64_t *shard_bytes, int64_t *max_table_bytes_unsharded) {
  if (!p) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan");
  // a table input may feed several columns (shared embeddings): count each once
  std::vector<int64_t> local(p->desc.n_device_inputs, 0), whole(p->desc.n_device_inputs, 0);
  for (size_t k = 0; k < p->cols.size(); ++k) {
    const HostColumn &hc = p->cols[k];
    const int f = hc.d.form;
    if (f != FCP_FORM_GATHER && f != FCP_FORM_SEGMENT_REDUCE && f != FCP_FORM_GATHER_SCATTER) continue;
    const int64_t local_vocab =
        (hc.d.vocab - p->desc.shard_rank + p->desc.shard_world - 1) / p->desc.shard_world;
    const int64_t row_bytes = p->col_row_bytes(k, hc.d.dim); // (per-input formats: each table at its own row size)
    local[hc.d.table_input] = std::max(local[hc.d.table_input], local_vocab * row_bytes);
    whole[hc.d.table_input] = std::max(whole[hc.d.table_input], hc.d.vocab * row_bytes);
  }
  int64_t sum = 0, mx = 0;
  for (int t = 0; t < p->desc.n_device_inputs; ++t) {
    sum += local[t];
    mx = std::max(mx, whole[t]);
  }
  if (shard_bytes) *shard_bytes = sum;
  if (max_table_bytes_unsharded) *max_table_bytes_unsharded = mx;
  return FCP_OK;
}

int fcp_plan_release_captures(fcp_plan_t *p) {
  if (!p) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan");
  std::lock_guard<std::mutex> lock(p->mu);
  for (auto &s : p->slots) {
    if (!s.captured) continue;
    s.captured = false;
    s.done_valid = false; // its readers were graph replays: the next installation drains the stream / device
  }
  return FCP_OK;
}

int fcp_plan_destroy(fcp_plan_t *p) {
  if (!p) return FCP_OK;
  if (!p->host_only) {
    DeviceGuard guard;
    if (guard.enter(p->desc.device) == FCP_OK) {
      (void)hipDeviceSynchronize();
      pending_forget(p); // (the lanes belong to the device's pool and stay)
      if (p->pool && p->lane_relies.exchange(false)) p->pool->n_relying.fetch_sub(1, std::memory_order_acq_rel);
      for (hipEvent_t *ev : {&p->sup.b0, &p->sup.b1, &p->sup.w0, &p->sup.w1}) // the supervisor's timing events
        if (*ev) {
          (void)hipEventDestroy(*ev);
          *ev = nullptr;
        }
      destroy_device(p);
    }
  }
  delete p;
  return FCP_OK;
}

int fcp_plan_group_width(const fcp_plan_t *p, int32_t group, int32_t *width) {
  if (!p || !width || group < 0 || group >= p->desc.n_groups)
    return fail(FCP_ERR_INVALID_ARGUMENT, "bad group");
  *width = p->group_width[group];
  return FCP_OK;
}

int fcp_plan_column_offset(const fcp_plan_t *p, int32_t column, int32_t *offset) {
  if (!p || !offset || column < 0 || column >= (int32_t)p->cols.size())
    return fail(FCP_ERR_INVALID_ARGUMENT, "bad column");
  *offset = p->cols[column].out_off;
  return FCP_OK;
}

int fcp_plan_arena_bytes(fcp_plan_t *p, const int32_t *concated_shapes, const int32_t *symbols,
                         int64_t *bytes) {
  if (!p || !concated_shapes || !bytes) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  std::vector<FcpColDyn> dyn(p->cols.size());
  std::vector<int32_t> offsets(p->ranks.size(), 0);
  DynMeta m;
  int rc = evaluate_shapes(*p, offsets.data(), concated_shapes, symbols, -1, dyn.data(), nullptr, &m);
  if (rc) return rc;
  *bytes = m.arena_bytes;
  return FCP_OK;
}

int fcp_plan_read_bad_ids(fcp_plan_t *p, void *stream, int64_t *count) {
  if (!p || !count) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  *count = 0;
  if (p->host_only) return fail(FCP_ERR_NO_DEVICE, "host-only plan");
  if (!p->d_bad) return FCP_OK;
  DeviceGuard guard;
  int rc = guard.enter(p->desc.device);
  if (rc) return rc;
  unsigned long long v = 0;
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  if (p->pool && p->lane_count > 0) { // requests of that stream may have run on a private lane
    std::lock_guard<std::mutex> cal_lock(p->pool->cal_mu);
    for (auto &l : p->pool->lanes)
      if (l->stream) HIP_TRY(hipStreamSynchronize(l->stream));
  }
  HIP_TRY(hipMemcpy(&v, p->d_bad, sizeof(v), hipMemcpyDeviceToHost));
  *count = (int64_t)v;
  return FCP_OK;
}

int fcp_plan_last_launch(const fcp_plan_t *p, fcp_launch_info_t *out) {
  if (!p || !out) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  const fcp_plan::LastLaunch &ll = p->last_launch;
  out->kernel = ll.kernel.load(std::memory_order_relaxed);
  out->vec = p->vec;
  out->rows_per_wave = ll.rows_per_wave.load(std::memory_order_relaxed);
  out->store_policy = ll.store_policy.load(std::memory_order_relaxed);
  out->wide_rows = p->wide_rows ? 1 : 0;
  out->shard_world = p->desc.shard_world > 1 ? p->desc.shard_world : 1;
  out->dense_blocks = ll.dense_blocks.load(std::memory_order_relaxed);
  out->ragged_blocks = ll.ragged_blocks.load(std::memory_order_relaxed);
  out->segment_offsets = ll.segment_offsets.load(std::memory_order_relaxed);
  return FCP_OK;
}

int fcp_plan_last_dense_front(const fcp_plan_t *p, int32_t *front) {
  if (!p || !front) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  *front = p->last_dense_front.load(std::memory_order_relaxed);
  return FCP_OK;
}

int fcp_plan_last_csr(const fcp_plan_t *p, int64_t *csr_arena_off, int32_t *csr_base, int32_t capacity) {
  if (!p || capacity < 0 || (capacity > 0 && !csr_base)) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan / bad capacity");
  const fcp_plan::LastLaunch &ll = p->last_launch;
  if (csr_arena_off) *csr_arena_off = ll.csr_arena_off.load(std::memory_order_relaxed);
  for (int32_t k = 0; k < capacity && k < (int32_t)p->cols.size(); ++k)
    csr_base[k] = ll.csr_base ? ll.csr_base[k].load(std::memory_order_relaxed) : -1;
  return FCP_OK;
}

} // extern "C"

