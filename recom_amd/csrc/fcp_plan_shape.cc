// fcp_plan_shape.cc — the host half of a plan: what plan creation derives from a checked descriptor (build_host_plan) and
// what a request's shapes make of it (evaluate_shapes).  Ordinary C++, no GPU header (fcp_plan_shape.h).
#include "fcp_plan_shape.h"

#include <algorithm>
#include <climits>

namespace fcph {

int build_host_plan(const fcp_plan_desc_t *desc, const fcp_column_ext_t *ext, PlanFacts &facts, HostPlan *p) {
  // the format facts, assigned here and nowhere else (fcp_formats.h)
  p->out_kind = facts.out_kind;
  p->out_elem = fcpf::kOut[facts.out_kind].elem;
  p->tab_kind = facts.tab_kind;
  p->col_kind.swap(facts.col_kind);
  p->tab_elem = p->tab_mixed() ? 0 : fcpf::kTab[facts.tab_kind].elem; // (mixed: no plan-wide element size, col_row_bytes)
  p->tab_row_tail = p->tab_mixed() ? 0 : fcpf::kTab[facts.tab_kind].row_tail;
  p->variant = facts.variant;
  p->weighted_kernel = facts.variant == FCP_VAR_WEIGHTED;
  p->env = fcp::read_env(); // the library's shipping switches, read here and nowhere on the request path (fcp_env.h)
  p->desc = *desc;
  p->desc.flags = facts.flags; // (per-input table formats of one kind: the plan-wide plan of that kind)
  p->desc.columns = nullptr;
  p->desc.host_input_ranks = nullptr;
  p->desc.host_input_elem_sizes = nullptr;
  p->host_only = (facts.flags & kFlagHostOnly) != 0;
  p->ranks.assign(desc->host_input_ranks, desc->host_input_ranks + desc->n_host_inputs);
  p->elem_sizes.assign(desc->host_input_elem_sizes, desc->host_input_elem_sizes + desc->n_host_inputs);
  p->shape_off.resize(desc->n_host_inputs);
  int32_t acc = 0;
  for (int i = 0; i < desc->n_host_inputs; ++i) {
    p->shape_off[i] = acc;
    acc += p->ranks[i];
  }
  p->rank_sum = acc;
  p->cols.resize(desc->n_columns);
  int gcd4 = 4;
  for (int k = 0; k < desc->n_columns; ++k) {
    HostColumn &hc = p->cols[k];
    hc.d = desc->columns[k];
    if (hc.d.id_source == FCP_IDS_F32_BUCKETIZE && hc.d.boundaries && hc.d.n_boundaries > 0 &&
        hc.d.form != FCP_FORM_PASSTHROUGH && hc.d.form != FCP_FORM_BATCH_COL_REDUCTION && hc.d.form != FCP_FORM_EXTERNAL)
      hc.boundaries.assign(hc.d.boundaries, hc.d.boundaries + hc.d.n_boundaries);
    hc.d.boundaries = nullptr;
    if (hc.d.xform_mode != FCP_XFORM_NONE && hc.d.xform_n > 0) {
      hc.xf_lo.assign(hc.d.xform_lo, hc.d.xform_lo + hc.d.xform_n);
      hc.xf_hi.assign(hc.d.xform_hi, hc.d.xform_hi + hc.d.xform_n);
    }
    hc.d.xform_lo = hc.d.xform_hi = nullptr;
    if (ext && ext[k].seg_map_n > 0) {
      hc.ext = ext[k];
      p->has_seg_map = true;
    }
    if (ext && ext[k].weights_input1 > 0) {
      hc.weights_input = ext[k].weights_input1 - 1;
      p->has_weights = true;
    }
    if (hc.d.dim % 4) gcd4 = (hc.d.dim % 2) ? 1 : std::min(gcd4, 2);
    const int f = hc.d.form;
    if ((f == FCP_FORM_SEGMENT_REDUCE || f == FCP_FORM_GATHER_SCATTER) && hc.d.seg_kind != FCP_SEG_CSR_I32)
      p->seg_cols.push_back(k);
  }
  p->vec = gcd4;
  // any-order ScatterNd columns last: their part of the CSR scratch (the inverse maps, built with atomic max from zero)
  // is then ONE range at the tail, the only one a request has to clear
  std::stable_partition(p->seg_cols.begin(), p->seg_cols.end(), [&](int32_t k) { return p->cols[k].d.form != FCP_FORM_GATHER_SCATTER; });
  p->n_seg_plain = 0;
  for (int32_t k : p->seg_cols) p->n_seg_plain += p->cols[k].d.form != FCP_FORM_GATHER_SCATTER;
  // Segment-id columns (SparseTensor indices / row ids): unsharded plans let every block find its rows'
  // ranges with a 16-ary search (fcp_kernels.hip::seg_lower_bound) instead of running the
  // ComputeSegmentOffsets pre-pass as a second, dependent launch.  Row-sharded plans keep the
  // pre-pass: fcp_shard_finalize needs the row lengths as CSR.  FCP_SEG_PREPASS=1: tuning aid.
  p->seg_search = desc->shard_world <= 1 && !p->env.seg_prepass;
  if (p->has_seg_map) p->seg_search = false; // mapped segment ids are evaluated by the pre-pass only
  for (const HostColumn &hc : p->cols) {
    if (hc.d.seg_kind != FCP_SEG_NONE && hc.d.seg_stride > 0xffff) p->seg_search = false; // stride rides in 16 flag bits
    // ScatterNd columns take their row ids in any order (cuda_emitter.cc:296-345): nothing to search, the pre-pass
    // builds the row -> position map
    if (hc.d.form == FCP_FORM_GATHER_SCATTER && hc.d.seg_kind != FCP_SEG_CSR_I32) {
      p->has_inverse = true;
      p->seg_search = false;
    }
  }
  p->csr_by_pos = desc->layout == FCP_LAYOUT_CONCAT && desc->n_groups == 1 && !p->has_inverse && !p->seg_cols.empty() &&
                  2 * p->seg_cols.size() >= p->cols.size();
  // (a column that brings its row offsets in the blob reads them there: the kernel's regular-CSR shortcut serves every pooled /
  // scatter column of the launch from ONE matrix, so a plan that mixes the two encodings keeps the packed scratch)
  for (const HostColumn &hc : p->cols)
    if ((hc.d.form == FCP_FORM_SEGMENT_REDUCE || hc.d.form == FCP_FORM_GATHER_SCATTER) && hc.d.seg_kind == FCP_SEG_CSR_I32) p->csr_by_pos = false;
  if (fcp::diag_ll("csr_by_pos", 1) == 0) p->csr_by_pos = false; // tuning aid: FCP_DIAG=csr_by_pos=0 = packed scratch (the round-5 layout)
  // The kernels park a table row as one 32-bit number (the three largest values are their sentinels): a table — or
  // one shard of it — may hold up to 2^32 - 3 ROWS, of any width: the byte offset is formed in 64 bits where the row
  // is read.  The dense body keeps round 2's pre-scaled 32-bit slot offsets (row * dim / vec) while every table of
  // the plan stays below 2^32 - 3 slots (64 GB at vec 4), which saves it a 64-bit multiply per read.  (The
  // reference's int arithmetic stops at 2^31 elements = 8 GB, cuda_emitter.cc:270-271.)
  const bool wide_rows_forced = fcp::diag_on("wide_rows"); // test aid: the 64-bit row arithmetic on small tables
  for (int k = 0; k < desc->n_columns; ++k) {
    const fcp_column_desc_t &c = p->cols[k].d;
    if (c.form == FCP_FORM_PASSTHROUGH || c.form == FCP_FORM_BATCH_COL_REDUCTION || c.form == FCP_FORM_EXTERNAL) continue;
    const int64_t local_vocab = (c.vocab - desc->shard_rank + desc->shard_world - 1) / desc->shard_world;
    if (local_vocab >= 0xFFFFFFFDLL) return fail(FCP_ERR_UNSUPPORTED, "column " + std::to_string(k) + ": table shard exceeds 2^32 - 3 rows");
    // (8-bit row-quantised tables: a row index is scaled by the row STRIDE in slots, (dim + 8) / vec — vec divides 8)
    // (per-input formats: the table's own kind decides)
    const int row_tail = fcpf::kTab[p->col_tab_kind(k)].row_tail;
    if (local_vocab * ((c.dim + row_tail) / p->vec) >= 0xFFFFFFFDLL || wide_rows_forced) p->wide_rows = true;
  }
  // concat layout: offsets = prefix sums of dims in slot order
  // (concat_outputs_op_gpu.cu.cc:74-79)
  const int ng = desc->n_groups;
  p->group_width.assign(ng, 0);
  p->group_nslots.assign(ng, 0);
  p->group_map_off.assign(ng, 0);
  int32_t map_off = 0; // the slot map (init_device) holds one entry per slot, group after group
  for (int g = 0; g < ng; ++g) {
    std::vector<int> members;
    for (int k = 0; k < desc->n_columns; ++k)
      if (p->cols[k].d.concat_group == g) members.push_back(k);
    if (members.empty()) return fail(FCP_ERR_INVALID_ARGUMENT, "concat group without columns");
    std::sort(members.begin(), members.end(),
              [&](int a, int b) { return p->cols[a].d.concat_slot < p->cols[b].d.concat_slot; });
    int32_t off = 0;
    for (int k : members) {
      p->cols[k].out_off = off;
      off += p->cols[k].d.dim;
    }
    p->group_width[g] = off;
    p->group_nslots[g] = off / p->vec;
    p->group_map_off[g] = map_off;
    map_off += p->group_nslots[g];
    for (int k : members) p->order.push_back(k);
  }
  p->pos_of.assign(desc->n_columns, 0);
  for (int pos = 0; pos < desc->n_columns; ++pos) p->pos_of[p->order[pos]] = pos;
  p->col_facts.resize(desc->n_columns);
  p->group_rep.assign(ng, -1);
  for (int pos = 0; pos < desc->n_columns; ++pos) {
    const HostColumn &hc = p->cols[p->order[pos]];
    const fcp_column_ext_t &e = hc.ext;
    ColFacts &f = p->col_facts[pos];
    f.ids_input = hc.d.ids_input;
    f.seg_input = hc.d.seg_input;
    f.rows_arg = hc.d.rows_arg;
    f.dim = hc.d.dim;
    f.seg_stride = hc.d.seg_stride < 1 ? 1 : hc.d.seg_stride;
    f.out_off_bytes = (int64_t)hc.out_off * p->out_elem;
    f.form = (uint8_t)hc.d.form;
    f.rows_source = (uint8_t)hc.d.rows_source; // (an external slot: FCP_ROWS_FROM_GROUP, check_desc)
    f.seg_kind = (uint8_t)hc.d.seg_kind;
    f.group = (uint8_t)hc.d.concat_group; // (at most FCP_MAX_GROUPS groups)
    if (p->has_seg_map || p->has_weights) {
      p->col_rare.resize(desc->n_columns);
      ColRare &r = p->col_rare[pos];
      r.weights_input = hc.weights_input;
      r.has_map = e.seg_map_n > 0;
      r.map_sym = r.has_map ? e.seg_map_sym : -1;
      r.map_sym_min = e.seg_map_sym_slot == 4 ? 1 : 0;
      r.map_factor = r.map_sym < 0 ? 0 : (e.seg_map_sym_slot == 4 ? e.seg_map_div : e.seg_map_mul[e.seg_map_sym_slot]);
    }
    if (p->group_rep[hc.d.concat_group] < 0 && hc.d.form != FCP_FORM_EXTERNAL) p->group_rep[hc.d.concat_group] = pos;
  }
  // hybrid dispatch: classify every 64-slot span of every group
  for (int kind = 0; kind < 2; ++kind) {
    p->list_off[kind].assign(ng, -1);
    p->list_n[kind].assign(ng, 0);
  }
  p->dense_only = true;
  for (int g = 0; g < ng; ++g) {
    const int nspans = (p->group_nslots[g] + FCP_WAVE - 1) / FCP_WAVE;
    // (a plan with a weighted or sqrtn column runs ALL its spans through the weighted ragged kernel: no weighted hybrid)
    std::vector<char> ragged(nspans, p->weighted_kernel ? 1 : 0);
    for (int k = 0; k < desc->n_columns; ++k) {
      const HostColumn &hc = p->cols[k];
      if (hc.d.concat_group != g) continue;
      if (hc.d.form == FCP_FORM_GATHER || hc.d.form == FCP_FORM_PASSTHROUGH || hc.d.form == FCP_FORM_EXTERNAL) continue;
      const int s0 = hc.out_off / p->vec / FCP_WAVE, s1 = (hc.out_off + hc.d.dim - 1) / p->vec / FCP_WAVE;
      for (int sp = s0; sp <= s1 && sp < nspans; ++sp) ragged[sp] = 1;
    }
    for (int kind = 0; kind < 2; ++kind) {
      p->list_off[kind][g] = (int32_t)p->span_list.size();
      for (int sp = 0; sp < nspans; ++sp)
        if (ragged[sp] == kind) p->span_list.push_back((uint32_t)sp);
      p->list_n[kind][g] = (int32_t)p->span_list.size() - p->list_off[kind][g];
    }
    if (p->list_n[1][g] > 0) p->dense_only = false;
  }
  return FCP_OK;
}

// Are this request's row-offset arrays regular (FcpLaunch::csr_reg)?  Mode 1: the plan lays its CSR scratch out by column
// position and the pre-pass fills it (not when the blocks search the segment ids themselves: then there is no scratch to
// read).  Mode 2: EVERY column of a one-group plan brings CSR offsets in the blob and the arrays lie one constant stride
// apart in position order — what a packer that keeps the converted inputs together produces; checked per descriptor
// install (n_columns compares), never assumed.
static void find_regular_csr(const HostPlan &p, const FcpColDyn *dyn, DynMeta *m) {
  m->csr_reg_mode = 0;
  m->csr_reg_stride = 0;
  m->csr_reg_base = 0;
  if (p.desc.n_groups != 1 || p.col_facts.empty() || m->group_rows[0] <= 0) return;
  const int nc = (int)p.col_facts.size();
  if (p.csr_by_pos) {
    if (m->seg_search) return;
    m->csr_reg_mode = 1;
    m->csr_reg_stride = (int32_t)(((int64_t)m->group_rows[0] + 1 + 31) / 32 * 32);
    m->csr_reg_base = 0; // relative to the scratch (csr_arena_off)
    return;
  }
  int64_t stride = 0;
  for (int i = 0; i < nc; ++i) {
    const ColFacts &c = p.col_facts[i];
    if (c.seg_kind != FCP_SEG_CSR_I32 || (c.form != FCP_FORM_SEGMENT_REDUCE && c.form != FCP_FORM_GATHER_SCATTER)) return;
    if (i == 1) stride = dyn[1].seg_off - dyn[0].seg_off;
    if (i >= 1 && dyn[i].seg_off - dyn[i - 1].seg_off != stride) return;
  }
  if (nc == 1) stride = 4 * ((int64_t)m->group_rows[0] + 1);
  if (stride < 4 * ((int64_t)m->group_rows[0] + 1) || (stride & 3) || stride / 4 > 0x7fffffff || (dyn[0].seg_off & 3)) return;
  m->csr_reg_mode = 2;
  m->csr_reg_stride = (int32_t)(stride / 4);
  m->csr_reg_base = dyn[0].seg_off;
}

// launch geometry, one set per kernel kind
static int finish_geometry(const HostPlan &p, DynMeta *m) {
  const int ng = p.desc.n_groups;
  int32_t max_rows = 0;
  for (int g = 0; g < ng; ++g) max_rows = std::max(max_rows, m->group_rows[g]);
  for (int kind = 0; kind < 2; ++kind) {
    DynMeta::Geo &G2 = m->geo[kind];
    int rpw = 1;
    if (kind == 0) {
      // 4 rows per wave (16 per block) measured best on S2 at batch 512 and 2048: ~2 rounds of blocks
      // de-phase the read and write bursts; 8 rows lose to the tail.  Choosing fewer rows per wave for
      // narrow plans so that the grid reaches 8 blocks per CU (round 2: DLRM 896 -> 3584 blocks) made
      // them SLOWER (DLRM 5.0 -> 7.0 us, S2 at batch 128 11.0 -> 11.9 us): a block's fixed staging chain
      // costs more than the idle CUs, see profiles/HISTORY.md, round 2.
      while (rpw < 4 && max_rows >= 32 * rpw) rpw *= 2; // >= 64 rows -> 4, 32..63 -> 2, < 32 -> 1
    } // ragged kernel: one row per wave (2 interleaved rows measured slower: 33.7 vs 31.6 us)
    G2.rows_per_wave = rpw;
    int32_t blocks = 0;
    for (int g = 0; g < ng; ++g) {
      FcpGroupLaunch &G = G2.groups[g];
      G.rows = m->group_rows[g];
      G.nslots = p.group_nslots[g];
      G.nlist = p.list_n[kind][g];
      // a list that names every span in order is the identity: -1 spares the blocks a dependent load
      const int nspans_g = (p.group_nslots[g] + FCP_WAVE - 1) / FCP_WAVE;
      G.span_list_off = G.nlist == nspans_g ? -1 : p.list_off[kind][g];
      // listed spans are dealt to XCDs in groups of 8; fewer than 8 are not padded
      // (nsp8 = -nlist selects the plain mapping in the kernels)
      G.nsp8 = G.nlist >= 8 ? (G.nlist + 7) / 8 : -std::max(G.nlist, 1);
      G.block_begin = blocks;
      G.slot_map_off = p.group_map_off[g];
      G.csr_reg_stride = 0; // (fill_launch sets groups[0]'s per request)
      const int rows_per_block = FCP_WAVES_PER_BLOCK * rpw;
      const int64_t ntiles = ((int64_t)G.rows + rows_per_block - 1) / rows_per_block;
      const int64_t nb = G.nlist == 0 ? 0 : (G.nsp8 > 0 ? 8ll * G.nsp8 : (int64_t)G.nlist) * ntiles;
      if (blocks + nb > 0x7fffffff) return fail(FCP_ERR_UNSUPPORTED, "grid too large");
      blocks += (int32_t)nb;
    }
    G2.grid_blocks = blocks;
  }
  return FCP_OK;
}

// A refusal with a fixed text, out of line: a failing branch of the walk is one call, and the text is built only there.
[[gnu::cold, gnu::noinline]] static int refuse(int code, const char *msg) { return fail(code, msg); }

// A column whose segment ids go through a map: the index matrix
// holds whole rows, and the request's value of the map's symbol is in range.
[[gnu::noinline]] static int check_seg_map(const ColRare &r, bool whole_rows, const int32_t *symbols, int32_t *seg_sym) {
  if (!whole_rows) return refuse(FCP_ERR_SHAPE_MISMATCH, "index matrix shorter than the id stream");
  if (r.map_sym < 0) return FCP_OK;
  if (!symbols) return refuse(FCP_ERR_INVALID_ARGUMENT, "plan needs the symbols tensor");
  *seg_sym = symbols[r.map_sym];
  if (*seg_sym < r.map_sym_min) return refuse(FCP_ERR_SHAPE_MISMATCH, "segment-id map: symbol value out of range");
  // the pre-pass multiplies the factor by the symbol in 64 bits (load_seg_mapped): the product — and with it
  // every idx * factor for idx < 2^31 — must stay inside int64
  if (*seg_sym > 0 && r.map_factor > (INT64_MAX >> 32) / *seg_sym)
    return refuse(FCP_ERR_UNSUPPORTED, "segment-id map: factor x symbol exceeds 2^31 (the reshaped row index would overflow)");
  return FCP_OK;
}

int evaluate_shapes(const HostPlan &p, const int32_t *offsets, const int32_t *shapes, const int32_t *symbols, int64_t blob_bytes,
                    FcpColDyn *dyn, int64_t *wts, DynMeta *m) {
  const int nc = (int)p.col_facts.size();
  const int ng = p.desc.n_groups;
  const int nh = (int)p.ranks.size();
  const bool concat = p.desc.layout == FCP_LAYOUT_CONCAT;
  // element counts of all host inputs, one pass (this function is on the request path whenever shapes change: it is the
  // host's critical path when every request brings new shapes; no allocation, no string building unless it fails)
  thread_local std::vector<int64_t> numel_v;
  numel_v.resize(nh);
  int64_t *numel = numel_v.data();
  const int32_t *dims = shapes; // (the inputs' dimensions lie behind one another: shape_off is the prefix sum of ranks)
  for (int i = 0; i < nh; ++i) {
    int64_t n = 1;
    int32_t sign = 0;
    for (const int32_t *const end = dims + p.ranks[i]; dims != end; ++dims) {
      sign |= *dims;
      n *= *dims;
    }
    if (sign < 0) return refuse(FCP_ERR_SHAPE_MISMATCH, "negative dimension in concated_shapes");
    numel[i] = n;
    if (offsets[i] < 0) return refuse(FCP_ERR_SHAPE_MISMATCH, "negative blob offset (int32 overflow?)");
    if (blob_bytes >= 0 && (int64_t)offsets[i] + n * p.elem_sizes[i] > blob_bytes)
      return fail(FCP_ERR_SHAPE_MISMATCH, "host input " + std::to_string(i) + " exceeds the blob");
  }
  constexpr int64_t kNoSymbols = INT64_MIN; // rows_of: the column names a symbol and the request brings none
  auto rows_of = [&](const ColFacts &c) -> int64_t {
    if (c.rows_source == FCP_ROWS_FROM_GROUP) return m->group_rows[c.group]; // external slots
    if (c.rows_source == FCP_ROWS_FROM_IDS) return numel[c.ids_input];
    if (c.rows_source == FCP_ROWS_FROM_SYMBOL) return symbols ? (int64_t)symbols[c.rows_arg] : kNoSymbols;
    return shapes[p.shape_off[c.rows_arg]];
  };
  auto bad_rows = [](int64_t rows) {
    return rows == kNoSymbols ? refuse(FCP_ERR_INVALID_ARGUMENT, "plan needs the symbols tensor") : refuse(FCP_ERR_SHAPE_MISMATCH, "row count out of range");
  };
  // a group's rows: those of its first column in concat order that has rows of its own; every other column must agree
  // arena: outputs, then CSR scratch (one malloc_buff, cuda_emitter.cc:2151-2163)
  m->group_rows.resize(ng);
  m->group_base.resize(ng);
  int64_t cursor = 0;
  for (int g = 0; g < ng; ++g) {
    if (p.group_rep[g] < 0) return refuse(FCP_ERR_INVALID_ARGUMENT, "concat group without columns");
    const int64_t rows = rows_of(p.col_facts[p.group_rep[g]]);
    if (rows < 0 || rows > 0x7fffffff) return bad_rows(rows);
    m->group_rows[g] = (int32_t)rows;
    m->group_base[g] = cursor;
    if (concat) cursor += align128(rows * p.group_width[g] * p.out_elem);
  }
  int32_t max_seg_nnz = 0, max_lookup_nnz = 0;
  int64_t seg_pairs = 0;
  int64_t gathered = 0; // floats
  const ColFacts *const facts = p.col_facts.data();
  const int32_t *const group_rows = m->group_rows.data(), *const group_width = p.group_width.data();
  const int64_t *const group_base = m->group_base.data();
  for (int i = 0; i < nc; ++i) {
    const ColFacts &c = facts[i];
    const int64_t rows = rows_of(c);
    if (rows != group_rows[c.group]) {
      if (rows < 0 || rows > 0x7fffffff) return bad_rows(rows);
      return fail(FCP_ERR_SHAPE_MISMATCH, "columns of concat group " + std::to_string(c.group) + " disagree on the row count");
    }
    FcpColDyn &d = dyn[i];
    const bool external = c.form == FCP_FORM_EXTERNAL;
    const int64_t n_ids = external ? 0 : numel[c.ids_input];
    d.ids_off = external ? 0 : offsets[c.ids_input];
    d.seg_off = 0;
    d.out_base = group_base[c.group] + c.out_off_bytes; // (the per-column layout sets these two below)
    d.out_stride = group_width[c.group];
    d.csr_base = -1;
    d.inner = 1;
    d.rows = (int32_t)rows;
    d.seg_sym = 1;
    if (c.form == FCP_FORM_GATHER) {
      if (n_ids != rows) // (rows is below 2^31)
        return n_ids > 0x7fffffff ? refuse(FCP_ERR_UNSUPPORTED, "more than 2^31 ids in one column")
                                  : refuse(FCP_ERR_SHAPE_MISMATCH, "gather column: ids count != rows");
      d.nnz = (int32_t)n_ids;
      if (d.nnz > max_lookup_nnz) max_lookup_nnz = d.nnz;
    } else if (external) {
      d.nnz = 0;
    } else if (c.form == FCP_FORM_PASSTHROUGH) {
      if (n_ids != rows * c.dim) return refuse(FCP_ERR_SHAPE_MISMATCH, "passthrough tensor size != rows*dim");
      if (n_ids / p.vec >= 0xFFFFFFFDLL) return refuse(FCP_ERR_UNSUPPORTED, "passthrough tensor exceeds 2^32 slots");
      d.nnz = (int32_t)rows;
    } else if (c.form == FCP_FORM_BATCH_COL_REDUCTION) {
      const int32_t *s = shapes + p.shape_off[c.ids_input];
      if (s[0] != rows || s[2] != c.dim) return refuse(FCP_ERR_SHAPE_MISMATCH, "BatchColReduction shape mismatch");
      d.inner = s[1];
      d.nnz = (int32_t)rows;
    } else {
      if (n_ids > 0x7fffffff) return refuse(FCP_ERR_UNSUPPORTED, "more than 2^31 ids in one column");
      d.nnz = (int32_t)n_ids;
      if (d.nnz > max_lookup_nnz) max_lookup_nnz = d.nnz;
      d.seg_off = offsets[c.seg_input];
      const int64_t n_seg = numel[c.seg_input];
      if (c.seg_kind == FCP_SEG_CSR_I32) {
        if (n_seg != rows + 1) return refuse(FCP_ERR_SHAPE_MISMATCH, "CSR offsets must have rows+1 entries");
      } else {
        if (n_seg < n_ids * c.seg_stride - (c.seg_stride - 1) && n_ids > 0)
          return refuse(FCP_ERR_SHAPE_MISMATCH, "segment id tensor shorter than the id stream");
        if (d.nnz > max_seg_nnz) max_seg_nnz = d.nnz;
        seg_pairs += rows;
      }
    }
    if ((d.ids_off | d.seg_off) & 3) return refuse(FCP_ERR_UNSUPPORTED, "blob tensor not 4-byte aligned");
    gathered += (int64_t)d.nnz * c.dim;
  }
  // plans with segment-id maps or per-id weights: those columns' checks, the map symbols' values and the weights' blob
  // offsets (-1 = unweighted), in a short loop of their own
  for (int i = 0; i < (int)p.col_rare.size(); ++i) {
    const ColRare &r = p.col_rare[i];
    if (r.has_map) {
      const int rc = check_seg_map(r, numel[facts[i].seg_input] >= numel[facts[i].ids_input] * facts[i].seg_stride, symbols, &dyn[i].seg_sym);
      if (rc) return rc;
    }
    if (!wts) continue;
    const int32_t w = r.weights_input;
    wts[i] = w < 0 ? -1 : offsets[w];
    if (w < 0) continue;
    if (numel[w] != numel[facts[i].ids_input])
      return fail(FCP_ERR_SHAPE_MISMATCH, "column " + std::to_string(p.order[i]) + ": the weights tensor does not hold one weight per id");
    if (offsets[w] & 3) return refuse(FCP_ERR_UNSUPPORTED, "blob tensor not 4-byte aligned");
  }
  if (!concat) // one buffer per column, in PLAN column order (the reference's alignmem order), float32 only
    for (int k = 0; k < nc; ++k) {
      const int pos = p.pos_of[k];
      FcpColDyn &d = dyn[pos];
      d.out_base = cursor;
      d.out_stride = facts[pos].dim;
      cursor += align128((int64_t)d.rows * d.out_stride * 4);
    }
  m->max_seg_nnz = max_seg_nnz;
  m->max_lookup_nnz = max_lookup_nnz;
  m->seg_pairs = seg_pairs;
  // A few segment-id columns (the reference's models E / F: 10-20 multi-hot columns next to ~1000
  // one-hot ones): searching inside the blocks beats a second, dependent launch (E 15.6 -> 13.5 us).
  // Hundreds of them (RAGGED with SparseTensor indices): every row block would repeat the search on
  // the same arrays, and the one coalesced pre-pass scan wins (39.8 us vs 42.7-58.9 us).
  m->seg_search = p.seg_search && seg_pairs <= p.env.seg_search_max_pairs;
  m->csr_arena_off = cursor;
  m->work_bytes = gathered * 4 + cursor;
  int64_t csr_cursor = 0; // in int32 elements
  if (p.csr_by_pos) {
    const int64_t stride = ((int64_t)m->group_rows[0] + 1 + 31) / 32 * 32;
    for (int k : p.seg_cols) dyn[p.pos_of[k]].csr_base = (int32_t)(p.pos_of[k] * stride);
    csr_cursor = stride * nc;
    if (csr_cursor > 0x7fffffff) return refuse(FCP_ERR_UNSUPPORTED, "CSR scratch exceeds 2^31 entries");
  } else {
    for (int k : p.seg_cols) {
      FcpColDyn &d = dyn[p.pos_of[k]];
      d.csr_base = (int32_t)csr_cursor;
      csr_cursor += ((int64_t)d.rows + 1 + 31) / 32 * 32;
      if (csr_cursor > 0x7fffffff) return refuse(FCP_ERR_UNSUPPORTED, "CSR scratch exceeds 2^31 entries");
    }
  }
  m->arena_bytes = cursor + csr_cursor * 4;
  find_regular_csr(p, dyn, m);
  return finish_geometry(p, m);
}

} // namespace fcph
