// fcp_plan_desc.cc — the descriptor level of libfcp_hip.so: descriptor validation, the refusals of the storage formats, the
// plan-file parser (the one place in the library that reads untrusted text), the placement gate, the choice of table formats by
// budget (fcp_table_formats_choose), and the thread's last-error string.  Ordinary C++ without a GPU header (fcp_plan_desc.h);
// fcp_plan.hip builds the plan object from what this unit decides.
#include "fcp_plan_desc.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>

namespace fcph {
namespace {
thread_local std::string g_last_error; // private to this unit: every other unit reports through fail
}

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

namespace {

int validate_desc(const fcp_plan_desc_t *d) {
  if (!d) return fail(FCP_ERR_INVALID_ARGUMENT, "null plan descriptor");
  if (d->abi_version != FCP_ABI_VERSION) return fail(FCP_ERR_INVALID_ARGUMENT, "abi_version mismatch");
  if (d->n_columns <= 0 || !d->columns) return fail(FCP_ERR_INVALID_ARGUMENT, "plan has no columns");
  if (d->n_host_inputs < 0 || (d->n_host_inputs > 0 && (!d->host_input_ranks || !d->host_input_elem_sizes)))
    return fail(FCP_ERR_INVALID_ARGUMENT, "host input attrs missing");
  if (d->n_groups <= 0 || d->n_groups > FCP_MAX_GROUPS)
    return fail(FCP_ERR_INVALID_ARGUMENT, "n_groups must be in [1, 16]");
  if (d->layout != FCP_LAYOUT_CONCAT && d->layout != FCP_LAYOUT_PER_COLUMN)
    return fail(FCP_ERR_INVALID_ARGUMENT, "bad layout");
  if (d->shard_world < 1 || d->shard_rank < 0 || d->shard_rank >= d->shard_world)
    return fail(FCP_ERR_INVALID_ARGUMENT, "bad shard rank/world");
  for (int i = 0; i < d->n_host_inputs; ++i) {
    if (d->host_input_ranks[i] < 0 || d->host_input_ranks[i] > 8)
      return fail(FCP_ERR_INVALID_ARGUMENT, "host input rank out of range");
    if (d->host_input_elem_sizes[i] <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, "bad element size");
  }
  for (int k = 0; k < d->n_columns; ++k) {
    const fcp_column_desc_t &c = d->columns[k];
    const std::string where = "column " + std::to_string(k) + ": ";
    if (c.form < FCP_FORM_GATHER || c.form > FCP_FORM_EXTERNAL)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad form");
    if (c.dim <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, where + "dim must be positive");
    if (c.concat_group < 0 || c.concat_group >= d->n_groups)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "concat_group out of range");
    if (c.form == FCP_FORM_EXTERNAL) {
      // a slot reserved for an Addons>ConcatOutputs host input: no inputs of its own
      if (d->layout != FCP_LAYOUT_CONCAT) return fail(FCP_ERR_INVALID_ARGUMENT, where + "external slots need FCP_LAYOUT_CONCAT");
      if (c.rows_source != FCP_ROWS_FROM_GROUP) return fail(FCP_ERR_INVALID_ARGUMENT, where + "external slot takes its rows from its group");
      for (int j = 0; j < k; ++j)
        if (d->columns[j].concat_group == c.concat_group && d->columns[j].concat_slot == c.concat_slot)
          return fail(FCP_ERR_INVALID_ARGUMENT, where + "duplicate concat slot");
      continue;
    }
    if (c.rows_source == FCP_ROWS_FROM_GROUP) return fail(FCP_ERR_INVALID_ARGUMENT, where + "only external slots take their rows from the group");
    if (c.ids_input < 0 || c.ids_input >= d->n_host_inputs)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "ids_input out of range");
    const bool lookup = c.form == FCP_FORM_GATHER || c.form == FCP_FORM_SEGMENT_REDUCE ||
                        c.form == FCP_FORM_GATHER_SCATTER;
    if (lookup) {
      if (c.vocab <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, where + "vocab must be positive");
      if (c.table_input < 0 || c.table_input >= d->n_device_inputs)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "table_input out of range");
      if (c.id_source < FCP_IDS_I32 || c.id_source > FCP_IDS_F32_BUCKETIZE)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad id_source");
      if (c.id_source == FCP_IDS_F32_BUCKETIZE && (c.n_boundaries <= 0 || !c.boundaries))
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "bucketize needs boundaries");
      const int esz = d->host_input_elem_sizes[c.ids_input];
      if (esz != (c.id_source == FCP_IDS_I64 ? 8 : 4))
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "ids element size does not match id_source");
    } else if (d->host_input_elem_sizes[c.ids_input] != 4) {
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "payload must be a 4-byte type");
    }
    if (c.hash_buckets != 0) {
      if (!lookup) return fail(FCP_ERR_INVALID_ARGUMENT, where + "id transforms apply to lookup columns only");
      if (c.hash_buckets < 0) return fail(FCP_ERR_INVALID_ARGUMENT, where + "hash_buckets must be positive");
      if (c.id_source == FCP_IDS_F32_BUCKETIZE) return fail(FCP_ERR_INVALID_ARGUMENT, where + "hash_buckets applies to integer ids");
    }
    if (c.xform_mode != FCP_XFORM_NONE) {
      if (!lookup) return fail(FCP_ERR_INVALID_ARGUMENT, where + "id transforms apply to lookup columns only");
      if (c.xform_mode != FCP_XFORM_SELECT && c.xform_mode != FCP_XFORM_FILTER)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad xform_mode");
      if (c.xform_n < 0 || c.xform_n > (1 << 20) || (c.xform_n > 0 && (!c.xform_lo || !c.xform_hi)))
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad id transform intervals");
      for (int i = 0; i < c.xform_n; ++i)
        if (c.xform_lo[i] > c.xform_hi[i]) return fail(FCP_ERR_INVALID_ARGUMENT, where + "empty id transform interval");
    }
    if (c.form == FCP_FORM_SEGMENT_REDUCE || c.form == FCP_FORM_GATHER_SCATTER) {
      if (c.seg_kind < FCP_SEG_IDS_I32 || c.seg_kind > FCP_SEG_CSR_I32)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad seg_kind");
      if (c.seg_input < 0 || c.seg_input >= d->n_host_inputs)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "seg_input out of range");
      if (c.seg_stride < 1) return fail(FCP_ERR_INVALID_ARGUMENT, where + "seg_stride must be >= 1");
      if (d->host_input_elem_sizes[c.seg_input] != (c.seg_kind == FCP_SEG_IDS_I64 ? 8 : 4))
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "segment element size does not match seg_kind");
      if (c.rows_source == FCP_ROWS_FROM_IDS)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "pooled column needs an explicit row source");
    }
    if (c.form == FCP_FORM_SEGMENT_REDUCE && c.combiner != FCP_COMBINER_SUM &&
        c.combiner != FCP_COMBINER_MEAN && c.combiner != FCP_COMBINER_SQRTN)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "segment-reduce needs sum, mean or sqrtn");
    if (c.form != FCP_FORM_SEGMENT_REDUCE && c.combiner == FCP_COMBINER_SQRTN)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "the sqrtn combiner applies to pooled columns only");
    if (c.form == FCP_FORM_BATCH_COL_REDUCTION && d->host_input_ranks[c.ids_input] != 3)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "BatchColReduction input must be rank 3");
    if (c.rows_source < FCP_ROWS_FROM_IDS || c.rows_source > FCP_ROWS_FROM_INPUT_DIM0)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad rows_source");
    if (c.rows_source == FCP_ROWS_FROM_SYMBOL && (c.rows_arg < 0 || c.rows_arg >= d->n_symbols))
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "symbol index out of range");
    if (c.rows_source == FCP_ROWS_FROM_INPUT_DIM0 &&
        (c.rows_arg < 0 || c.rows_arg >= d->n_host_inputs || d->host_input_ranks[c.rows_arg] < 1))
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "rows_arg host input out of range");
    for (int j = 0; j < k; ++j)
      if (d->columns[j].concat_group == c.concat_group && d->columns[j].concat_slot == c.concat_slot)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "duplicate concat slot");
  }
  return FCP_OK;
}

int validate_ext(const fcp_plan_desc_t *d, const fcp_column_ext_t *ext) {
  for (int k = 0; k < d->n_columns; ++k) {
    const fcp_column_ext_t &e = ext[k];
    const fcp_column_desc_t &c = d->columns[k];
    const std::string where = "column " + std::to_string(k) + ": ";
    if (e.weights_input1 != 0) { // per-id weights (read before the map check below skips the record)
      if (c.form != FCP_FORM_SEGMENT_REDUCE) return fail(FCP_ERR_INVALID_ARGUMENT, where + "per-id weights apply to pooled columns only");
      if (e.weights_input1 < 0 || e.weights_input1 > d->n_host_inputs)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "weights input out of range");
      if (d->host_input_elem_sizes[e.weights_input1 - 1] != 4) return fail(FCP_ERR_INVALID_ARGUMENT, where + "per-id weights are float32");
    }
    if (e.seg_map_n == 0) continue;
    if (e.seg_map_n < 0 || e.seg_map_n > FCP_SEG_MAP_MAX) return fail(FCP_ERR_INVALID_ARGUMENT, where + "seg_map_n out of range");
    if (c.form != FCP_FORM_SEGMENT_REDUCE || (c.seg_kind != FCP_SEG_IDS_I32 && c.seg_kind != FCP_SEG_IDS_I64))
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "a segment-id map needs a pooled column with segment ids");
    if (c.seg_stride < e.seg_map_n) return fail(FCP_ERR_INVALID_ARGUMENT, where + "seg_stride is smaller than the number of mapped coordinates");
    if (e.seg_map_div < 1) return fail(FCP_ERR_INVALID_ARGUMENT, where + "seg_map_div must be >= 1");
    for (int i = 0; i < e.seg_map_n; ++i)
      if (e.seg_map_mul[i] < 0) return fail(FCP_ERR_INVALID_ARGUMENT, where + "negative seg_map_mul");
    if (e.seg_map_sym >= d->n_symbols || e.seg_map_sym < -1) return fail(FCP_ERR_INVALID_ARGUMENT, where + "seg_map_sym out of range");
    if (e.seg_map_sym >= 0 && !(e.seg_map_sym_slot == 4 || (e.seg_map_sym_slot >= 0 && e.seg_map_sym_slot < e.seg_map_n)))
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "seg_map_sym_slot out of range");
  }
  return FCP_OK;
}

// Per-input table formats (FCP_FLAG_TABLES_PER_INPUT): the kind of every column's table from fcp_column_ext_t::table_kind1.
// `col_kind` receives one FCP_TAB_* per column (FCP_TAB_F32 for columns without a table), `uniform` the one kind all tables of
// the plan share, or -1 when they really differ.
int resolve_table_kinds(const fcp_plan_desc_t *d, const fcp_column_ext_t *ext, std::vector<int8_t> *col_kind, int *uniform) {
  if (d->flags & (FCP_FLAG_TABLES_BF16 | FCP_FLAG_TABLES_F16 | FCP_FLAG_TABLES_Q8))
    return fail(FCP_ERR_INVALID_ARGUMENT, "FCP_FLAG_TABLES_PER_INPUT and FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16 / FCP_FLAG_TABLES_Q8 exclude each other");
  std::vector<int> in_kind(d->n_device_inputs, -1), in_col(d->n_device_inputs, -1);
  col_kind->assign(d->n_columns, (int8_t)FCP_TAB_F32);
  *uniform = -2; // no table seen yet
  for (int k = 0; k < d->n_columns; ++k) {
    const fcp_column_desc_t &c = d->columns[k];
    const std::string where = "column " + std::to_string(k) + ": ";
    const int kind1 = ext ? ext[k].table_kind1 : 0;
    if (kind1 < 0 || kind1 > 1 + FCP_TAB_Q8) return fail(FCP_ERR_INVALID_ARGUMENT, where + "table_kind1 is no 1 + FCP_TAB_* value");
    const bool lookup = c.form == FCP_FORM_GATHER || c.form == FCP_FORM_SEGMENT_REDUCE || c.form == FCP_FORM_GATHER_SCATTER;
    if (!lookup) {
      if (kind1 != 0) return fail(FCP_ERR_INVALID_ARGUMENT, where + "a column without a table carries table_kind1 0");
      continue;
    }
    const int kind = kind1 ? kind1 - 1 : FCP_TAB_F32, t = c.table_input;
    if (in_kind[t] >= 0 && in_kind[t] != kind)
      return fail(FCP_ERR_INVALID_ARGUMENT, "columns " + std::to_string(in_col[t]) + " and " + std::to_string(k) + " share table input " +
                                                std::to_string(t) + " but name different table kinds");
    if (in_kind[t] < 0) {
      in_kind[t] = kind;
      in_col[t] = k;
    }
    (*col_kind)[k] = (int8_t)kind;
    *uniform = *uniform == -2 || *uniform == kind ? kind : -1;
  }
  if (*uniform == -2) *uniform = FCP_TAB_F32; // a plan without tables
  return FCP_OK;
}

// What the kernels of a storage format do not serve is refused here, by name, for device and host-only plans alike: ONE list
// of rules, applied once per format family the plan is of, in the families' order.  A rule: the families it applies to, its
// condition — over the plan, or (COLUMN) over one column and its extension record, reported as "column k: " for the lowest
// such k —, the status, and the message with {S} for the family's subject phrase and {K} for its kernels' name.
enum { NARROW = 1, MIXED = 2, Q8 = 4, TAB16 = 8, TABLES = MIXED | Q8 | TAB16, ALL = NARROW | TABLES };
const char *const kSubject[] = {"narrow output", "per-input table formats", "8-bit tables", "16-bit tables"}; // by family bit
const char *const kKernels[] = {"narrow", "mixed-table", "8-bit-table", "16-bit-table"};
constexpr uint32_t kTab16Flags = FCP_FLAG_TABLES_BF16 | FCP_FLAG_TABLES_F16;
struct Rule {
  unsigned families;
  bool column;
  bool (*hit)(const fcp_plan_desc_t &d, const fcp_column_desc_t &c, const fcp_column_ext_t *e);
  int status;
  const char *text;
};
#define PLAN(cond) false, [](const fcp_plan_desc_t &d, const fcp_column_desc_t &, const fcp_column_ext_t *) -> bool { return cond; }
#define COLUMN(cond) true, [](const fcp_plan_desc_t &, const fcp_column_desc_t &c, const fcp_column_ext_t *e) -> bool { return cond; }
const Rule kRules[] = {
    {NARROW, PLAN((d.flags & fcpf::kOutFlags) == fcpf::kOutFlags), FCP_ERR_INVALID_ARGUMENT, "FCP_FLAG_OUT_BF16 and FCP_FLAG_OUT_F16 exclude each other"},
    {Q8, PLAN(d.flags & kTab16Flags), FCP_ERR_INVALID_ARGUMENT, "FCP_FLAG_TABLES_Q8 and FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16 exclude each other"},
    {TAB16, PLAN((d.flags & kTab16Flags) == kTab16Flags), FCP_ERR_INVALID_ARGUMENT, "FCP_FLAG_TABLES_BF16 and FCP_FLAG_TABLES_F16 exclude each other"},
    {TABLES, PLAN(d.flags & fcpf::kOutFlags), FCP_ERR_UNSUPPORTED, "{S} with narrow output (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16): the {K} kernels store float32"},
    {NARROW, PLAN(d.shard_world > 1), FCP_ERR_UNSUPPORTED, "{S} on a row-sharded plan (shard_world > 1): partial sums cross the exchange in float32"},
    {TABLES, PLAN(d.shard_world > 1), FCP_ERR_UNSUPPORTED, "{S} on a row-sharded plan (shard_world > 1): the sharded kernels read float32 tables"},
    {NARROW, PLAN(d.layout == FCP_LAYOUT_PER_COLUMN), FCP_ERR_UNSUPPORTED, "{S} needs FCP_LAYOUT_CONCAT: FCP_LAYOUT_PER_COLUMN is the reference's float32 arena"},
    {NARROW, COLUMN(c.form == FCP_FORM_EXTERNAL), FCP_ERR_UNSUPPORTED, "{S} with an FCP_FORM_EXTERNAL slot: fcp_concat_outputs_host scatters float32 payloads"},
    {ALL, COLUMN(e && e->weights_input1 > 0), FCP_ERR_UNSUPPORTED, "{S} with per-id weights: weighted plans take the float32 weighted kernel"},
    {ALL, COLUMN(c.combiner == FCP_COMBINER_SQRTN && c.form == FCP_FORM_SEGMENT_REDUCE), FCP_ERR_UNSUPPORTED, "{S} with FCP_COMBINER_SQRTN: sqrtn plans take the float32 weighted kernel"},
};
#undef PLAN
#undef COLUMN

int run_refusals(const fcp_plan_desc_t &d, const fcp_column_ext_t *ext, unsigned families) {
  for (int f = 0; f < 4; ++f) {
    if (!(families >> f & 1)) continue;
    for (int k = -1; k < d.n_columns; ++k) // -1: the rules about the plan, ahead of every column's
      for (const Rule &r : kRules) {
        if (!(r.families >> f & 1) || r.column != (k >= 0) || !r.hit(d, d.columns[std::max(k, 0)], ext ? &ext[std::max(k, 0)] : nullptr)) continue;
        std::string msg = (k < 0 ? "" : "column " + std::to_string(k) + ": ") + r.text;
        size_t at;
        if ((at = msg.find("{S}")) != std::string::npos) msg.replace(at, 3, kSubject[f]);
        if ((at = msg.find("{K}")) != std::string::npos) msg.replace(at, 3, kKernels[f]);
        return fail(r.status, msg);
      }
  }
  return FCP_OK;
}

// A column-plan file in memory (see include/fcp_hip.h for the format).
struct ParsedPlanFile {
  fcp_plan_desc_t d;
  std::vector<int32_t> ranks, esz;
  std::vector<fcp_column_desc_t> cols;
  std::vector<std::vector<float>> bnd;
  std::vector<std::vector<int64_t>> xlo, xhi;
  std::vector<fcp_column_ext_t> ext; // "weights" (version 5) and "segmaps" (version 4) sections; empty = no column has extensions
  // "stage" section (version 3): what Addons>ConcatInputs does to each of ITS inputs while packing
  std::vector<uint8_t> stage_modes;
  std::vector<int32_t> stage_rows_symbol;
  int32_t stage_symbols_input = -1;
  bool has_stage = false;
  int out_kind = FCP_OUT_F32; // the "out_dtype" line (version 6)
  int tab_kind = FCP_TAB_F32; // the "table_dtype" line (version 7)
  std::vector<int> in_kinds;  // the "table_dtypes" line (version 8): FCP_TAB_* per device input, -1 = "-"
};

int parse_plan_file(const char *path, ParsedPlanFile &P) {
  std::FILE *f = std::fopen(path, "r");
  if (!f) return fail(FCP_ERR_INVALID_ARGUMENT, std::string("cannot open column plan ") + path);
  struct Closer {
    std::FILE *f;
    ~Closer() { std::fclose(f); }
  } closer{f};
  const std::string where = std::string("column plan ") + path + ": ";
  char tag[32], t2[32], t3[32];
  int version = 0, n_host = 0, n_cols = 0;
  fcp_plan_desc_t &d = P.d;
  std::memset(&d, 0, sizeof(d));
  if (std::fscanf(f, "%31s %d", tag, &version) != 2 || std::strcmp(tag, "fcp_plan") || version < 1 || version > 8)
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad header");
  if (version >= 8) { // plans whose tables have more than one format: "table_dtypes D k0 ... k(D-1)", under the same rules
    int n_kinds = -1;
    if (std::fscanf(f, "%31s %d", tag, &n_kinds) != 2 || std::strcmp(tag, "table_dtypes") || n_kinds < 0 || n_kinds > (1 << 24))
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'table_dtypes D k0 ... k(D-1)'");
    P.in_kinds.resize(n_kinds);
    for (int t = 0; t < n_kinds; ++t) {
      if (std::fscanf(f, "%31s", t2) != 1) return fail(FCP_ERR_INVALID_ARGUMENT, where + "truncated table_dtypes line");
      const int kind = fcpf::tab_kind_of_name(t2);
      if (kind < 0 && std::strcmp(t2, "-")) return fail(FCP_ERR_INVALID_ARGUMENT, where + "unknown table dtype '" + t2 + "' in the table_dtypes line");
      P.in_kinds[t] = kind;
    }
  } else if (version >= 7) { // plans with 16-bit tables: "table_dtype bf16|f16", under the rules of version 6's line, which they never carry
    if (std::fscanf(f, "%31s %31s", tag, t2) != 2 || std::strcmp(tag, "table_dtype") || (P.tab_kind = fcpf::tab_kind_of_name(t2)) <= FCP_TAB_F32)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'table_dtype bf16', 'table_dtype f16' or 'table_dtype q8'");
  } else if (version >= 6) { // narrow-output plans: "out_dtype bf16|f16", here and nowhere else (anywhere else it is no 'layout' / section)
    if (std::fscanf(f, "%31s %31s", tag, t2) != 2 || std::strcmp(tag, "out_dtype") || (P.out_kind = fcpf::out_kind_of_name(t2)) <= FCP_OUT_F32)
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'out_dtype bf16' or 'out_dtype f16'");
  }
  if (std::fscanf(f, "%31s %d", tag, &d.layout) != 2 || std::strcmp(tag, "layout"))
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'layout'");
  if (std::fscanf(f, "%31s %d %31s %d %31s %d", tag, &d.n_groups, t2, &d.n_symbols, t3, &d.n_device_inputs) != 6 ||
      std::strcmp(tag, "groups") || std::strcmp(t2, "symbols") || std::strcmp(t3, "device_inputs"))
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'groups G symbols S device_inputs D'");
  if (version >= 8 && (int)P.in_kinds.size() != d.n_device_inputs)
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "the table_dtypes line names " + std::to_string(P.in_kinds.size()) + " inputs, the plan has " +
                                              std::to_string(d.n_device_inputs) + " device inputs");
  if (std::fscanf(f, "%31s %d", tag, &n_host) != 2 || std::strcmp(tag, "host_inputs") || n_host < 0 || n_host > (1 << 24))
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'host_inputs N'");
  P.ranks.resize(n_host);
  P.esz.resize(n_host);
  for (int i = 0; i < n_host; ++i)
    if (std::fscanf(f, "%d %d", &P.ranks[i], &P.esz[i]) != 2) return fail(FCP_ERR_INVALID_ARGUMENT, where + "truncated host input list");
  if (std::fscanf(f, "%31s %d", tag, &n_cols) != 2 || std::strcmp(tag, "columns") || n_cols < 0 || n_cols > (1 << 24))
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'columns C'");
  P.cols.resize(n_cols);
  P.bnd.resize(n_cols);
  P.xlo.resize(n_cols);
  P.xhi.resize(n_cols);
  for (int k = 0; k < n_cols; ++k) {
    fcp_column_desc_t &c = P.cols[k];
    std::memset(&c, 0, sizeof(c));
    long long vocab = 0;
    if (std::fscanf(f, "%d %d %d %d %lld %d %d %d %d %d %d %d %d %d %d", &c.form, &c.combiner, &c.dim, &c.id_source, &vocab,
                    &c.table_input, &c.ids_input, &c.seg_input, &c.seg_kind, &c.seg_stride, &c.rows_source, &c.rows_arg,
                    &c.concat_group, &c.concat_slot, &c.n_boundaries) != 15 ||
        c.n_boundaries < 0 || c.n_boundaries > (1 << 24))
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "truncated or malformed column " + std::to_string(k));
    c.vocab = vocab;
    P.bnd[k].resize(c.n_boundaries);
    for (int b = 0; b < c.n_boundaries; ++b)
      if (std::fscanf(f, "%f", &P.bnd[k][b]) != 1) return fail(FCP_ERR_INVALID_ARGUMENT, where + "truncated boundary list");
    c.boundaries = c.n_boundaries ? P.bnd[k].data() : nullptr;
    if (version >= 2) { // id transform: mode, number of intervals, substitute, (lo, hi) pairs
      long long sub = 0, hb = 0;
      if (std::fscanf(f, "%d %d %lld %lld", &c.xform_mode, &c.xform_n, &sub, &hb) != 4 || c.xform_n < 0 || c.xform_n > (1 << 20))
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "truncated or malformed id transform of column " + std::to_string(k));
      c.xform_substitute = sub;
      c.hash_buckets = hb;
      P.xlo[k].resize(c.xform_n);
      P.xhi[k].resize(c.xform_n);
      for (int i = 0; i < c.xform_n; ++i) {
        long long lo = 0, hi = 0;
        if (std::fscanf(f, "%lld %lld", &lo, &hi) != 2) return fail(FCP_ERR_INVALID_ARGUMENT, where + "truncated interval list");
        P.xlo[k][i] = lo;
        P.xhi[k][i] = hi;
      }
      c.xform_lo = c.xform_n ? P.xlo[k].data() : nullptr;
      c.xform_hi = c.xform_n ? P.xhi[k].data() : nullptr;
    }
  }
  // optional trailing sections: "weights M" + M x "column input" (version 5), then "segmaps M" + M x "column n sym slot
  // mul0 mul1 mul2 mul3 div" (version 4), then "stage N symbols_input K" + N x "mode rows_symbol" (version 3)
  bool seen_maps = false, seen_weights = false;
  for (;;) {
    int count = 0;
    const int got = std::fscanf(f, "%31s %d", tag, &count);
    if (got == EOF || got == 0) break;
    if (got != 2) return fail(FCP_ERR_INVALID_ARGUMENT, where + "malformed trailing section");
    if (version >= 5 && !std::strcmp(tag, "weights") && !seen_weights && !seen_maps && !P.has_stage) {
      if (count < 0 || count > n_cols) return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad 'weights M'");
      seen_weights = true;
      if (count > 0) P.ext.assign(n_cols, fcp_column_ext_t{});
      for (int i = 0; i < count; ++i) {
        int col = -1, input = -1;
        if (std::fscanf(f, "%d %d", &col, &input) != 2 || col < 0 || col >= n_cols || input < 0 || input >= n_host ||
            P.ext[col].weights_input1 != 0)
          return fail(FCP_ERR_INVALID_ARGUMENT, where + "malformed weights entry " + std::to_string(i));
        P.ext[col].weights_input1 = input + 1;
      }
    } else if (version >= 4 && !std::strcmp(tag, "segmaps") && !seen_maps && !P.has_stage) {
      if (count < 0 || count > n_cols) return fail(FCP_ERR_INVALID_ARGUMENT, where + "bad 'segmaps M'");
      seen_maps = true;
      if (P.ext.empty()) P.ext.assign(n_cols, fcp_column_ext_t{});
      for (int i = 0; i < count; ++i) {
        int col = -1, n = 0, sym = -1, slot = 0;
        long long mul[4] = {0, 0, 0, 0}, div = 1;
        if (std::fscanf(f, "%d %d %d %d %lld %lld %lld %lld %lld", &col, &n, &sym, &slot, &mul[0], &mul[1], &mul[2], &mul[3], &div) != 9 ||
            col < 0 || col >= n_cols || n < 1 || n > FCP_SEG_MAP_MAX || P.ext[col].seg_map_n != 0)
          return fail(FCP_ERR_INVALID_ARGUMENT, where + "malformed segmaps entry " + std::to_string(i));
        fcp_column_ext_t &e = P.ext[col];
        e.seg_map_n = n;
        e.seg_map_sym = sym;
        e.seg_map_sym_slot = slot;
        for (int j = 0; j < 4; ++j) e.seg_map_mul[j] = mul[j];
        e.seg_map_div = div;
      }
    } else if (version >= 3 && !std::strcmp(tag, "stage") && !P.has_stage) {
      const int n_stage = count;
      int sym_in = -1;
      if (std::fscanf(f, "%31s %d", t2, &sym_in) != 2 || std::strcmp(t2, "symbols_input") || n_stage < 0 || n_stage > (1 << 24) ||
          sym_in < -1 || sym_in >= n_stage)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "expected 'stage N symbols_input K'");
      P.stage_modes.resize(n_stage);
      P.stage_rows_symbol.resize(n_stage);
      for (int i = 0; i < n_stage; ++i) {
        int mode = 0, sym = -1;
        if (std::fscanf(f, "%d %d", &mode, &sym) != 2 || mode < FCP_STAGE_COPY || mode > FCP_STAGE_SEG_TO_CSR || sym < -1 ||
            sym >= d.n_symbols || (mode == FCP_STAGE_SEG_TO_CSR && (sym < 0 || sym_in < 0)))
          return fail(FCP_ERR_INVALID_ARGUMENT, where + "malformed stage entry " + std::to_string(i));
        P.stage_modes[i] = (uint8_t)mode;
        P.stage_rows_symbol[i] = sym;
      }
      P.stage_symbols_input = sym_in;
      P.has_stage = true;
    } else {
      return fail(FCP_ERR_INVALID_ARGUMENT, where + "unexpected section '" + tag + "'");
    }
  }
  if (version >= 8) { // the kinds travel to fcp_plan_create_ex as every column's table_kind1
    if (P.ext.empty()) P.ext.assign(n_cols, fcp_column_ext_t{});
    std::vector<char> read(P.in_kinds.size(), 0);
    int first = -1;
    bool differ = false;
    for (int k = 0; k < n_cols; ++k) {
      const fcp_column_desc_t &c = P.cols[k];
      if (c.form != FCP_FORM_GATHER && c.form != FCP_FORM_SEGMENT_REDUCE && c.form != FCP_FORM_GATHER_SCATTER) continue;
      if (c.table_input < 0 || c.table_input >= (int)P.in_kinds.size() || P.in_kinds[c.table_input] < 0)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "column " + std::to_string(k) + " reads a table the table_dtypes line gives no dtype");
      read[c.table_input] = 1;
      const int kind = P.in_kinds[c.table_input];
      P.ext[k].table_kind1 = 1 + kind;
      differ = differ || (first >= 0 && kind != first);
      if (first < 0) first = kind;
    }
    for (size_t t = 0; t < read.size(); ++t)
      if (!read[t] && P.in_kinds[t] >= 0)
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "the table_dtypes line gives device input " + std::to_string(t) + ", which no lookup column reads, a dtype");
    if (!differ) return fail(FCP_ERR_INVALID_ARGUMENT, where + "version 8 is for plans whose tables have more than one dtype; this one is a version <= 7 plan");
  }
  d.abi_version = FCP_ABI_VERSION;
  d.n_columns = n_cols;
  d.columns = P.cols.data();
  d.n_host_inputs = n_host;
  d.host_input_ranks = P.ranks.data();
  d.host_input_elem_sizes = P.esz.data();
  d.shard_rank = 0;
  d.shard_world = 1;
  return FCP_OK;
}

} // namespace

int check_desc(const fcp_plan_desc_t *desc, const fcp_column_ext_t *ext, PlanFacts *facts) {
  int rc = validate_desc(desc);
  if (rc) return rc;
  if (ext && (rc = validate_ext(desc, ext))) return rc;
  // Per-input table formats: tables that all share one kind make this the plan-wide plan of that kind — the flags are
  // rewritten to that plan's here, and nothing behind this point knows the difference.  Only tables that really differ
  // keep their per-column kinds (col_kind) and take the mixed-table kernels.
  fcp_plan_desc_t d = *desc;
  facts->col_kind.clear();
  if (d.flags & FCP_FLAG_TABLES_PER_INPUT) {
    int uniform = -1;
    if ((rc = resolve_table_kinds(desc, ext, &facts->col_kind, &uniform))) return rc;
    d.flags &= ~(uint32_t)FCP_FLAG_TABLES_PER_INPUT;
    if (uniform >= 0) {
      facts->col_kind.clear();
      d.flags |= fcpf::kTab[uniform].flag;
    }
  }
  const bool mixed = !facts->col_kind.empty();
  const unsigned families = ((d.flags & fcpf::kOutFlags) ? NARROW : 0) | (mixed ? MIXED : 0) | ((d.flags & FCP_FLAG_TABLES_Q8) ? Q8 : 0) | ((d.flags & kTab16Flags) ? TAB16 : 0);
  if ((rc = run_refusals(d, ext, families))) return rc;
  facts->flags = d.flags;
  facts->out_kind = fcpf::out_kind_of_flags(d.flags);
  facts->tab_kind = mixed ? FCP_TAB_MIXED : fcpf::tab_kind_of_flags(d.flags);
  bool weighted = false; // per-id weights or the sqrtn combiner
  for (int k = 0; k < d.n_columns; ++k) weighted = weighted || (ext && ext[k].weights_input1 > 0) || d.columns[k].combiner == FCP_COMBINER_SQRTN;
  // (the refusals above leave a plan at most one of these)
  facts->variant = weighted                           ? FCP_VAR_WEIGHTED
                   : facts->out_kind != FCP_OUT_F32   ? FCP_VAR_NARROW
                   : mixed                            ? FCP_VAR_TABMIX
                   : facts->tab_kind == FCP_TAB_Q8    ? FCP_VAR_TABQ8
                   : facts->tab_kind != FCP_TAB_F32   ? FCP_VAR_TAB16
                                                      : FCP_VAR_F32;
  return FCP_OK;
}

} // namespace fcph

using namespace fcph;

// failure reporting for the units that do not include fcp_plan_desc.h (fcp_shard.hip, fcp_graph.cc)
int fcp_internal_fail(int code, const std::string &msg) { return fail(code, msg); }

extern "C" {

int fcp_abi_version(void) { return FCP_ABI_VERSION; }

const char *fcp_status_string(int status) {
  switch (status) {
  case FCP_OK: return "ok";
  case FCP_ERR_INVALID_ARGUMENT: return "invalid argument";
  case FCP_ERR_SHAPE_MISMATCH: return "run-time shapes do not match the plan";
  case FCP_ERR_ALLOC: return "allocator callback failed";
  case FCP_ERR_HIP: return "HIP runtime error";
  case FCP_ERR_UNSUPPORTED: return "unsupported";
  case FCP_ERR_NO_DEVICE: return "no usable gfx950 device";
  default: return "unknown status";
  }
}

const char *fcp_last_error(void) { return g_last_error.c_str(); }

// (fcp_plan_create_ex: fcp_plan.hip — or, where this unit is linked alone, whatever stands in for it)
int fcp_plan_create_from_file(const char *path, int32_t device, uint32_t flags, fcp_plan_t **out) {
  if (!path || !out) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  ParsedPlanFile P;
  const int rc = parse_plan_file(path, P);
  if (rc) return rc;
  const std::string where = std::string("column plan ") + path + ": ";
  if (P.has_stage && (int32_t)P.stage_modes.size() != P.d.n_host_inputs)
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "the stage section lists " + std::to_string(P.stage_modes.size()) + " inputs, the plan has " +
                                              std::to_string(P.d.n_host_inputs) + " host inputs");
  P.d.device = device;
  // the file names the dtypes: flag bits may repeat them, not contradict them (float32: no line, no bit, nothing to contradict)
  if (P.out_kind != FCP_OUT_F32 && (flags & fcpf::kOutFlags & ~fcpf::kOut[P.out_kind].flag))
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "flags ask for another output dtype than the file's out_dtype line");
  if (P.tab_kind != FCP_TAB_F32 && (flags & fcpf::kTabFlags & ~fcpf::kTab[P.tab_kind].flag))
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "flags ask for another table dtype than the file's table_dtype line");
  // (a version-8 file names every table's dtype: plan-wide table bits contradict it)
  if (!P.in_kinds.empty() && (flags & fcpf::kTabFlags))
    return fail(FCP_ERR_INVALID_ARGUMENT, where + "plan-wide table dtype flags with a file that carries a table_dtypes line");
  P.d.flags = flags | fcpf::kOut[P.out_kind].flag | fcpf::kTab[P.tab_kind].flag | (P.in_kinds.empty() ? 0u : FCP_FLAG_TABLES_PER_INPUT);
  return fcp_plan_create_ex(&P.d, P.ext.empty() ? nullptr : P.ext.data(), out);
}

int fcp_plan_file_stage_info(const char *path, int32_t *n_inputs, uint8_t *modes, int32_t *rows_symbol, int32_t capacity,
                             int32_t *symbols_input) {
  if (!path) return fail(FCP_ERR_INVALID_ARGUMENT, "null argument");
  ParsedPlanFile P;
  const int rc = parse_plan_file(path, P);
  if (rc) return rc;
  const int32_t n = P.has_stage ? (int32_t)P.stage_modes.size() : 0;
  if (n_inputs) *n_inputs = n;
  if (symbols_input) *symbols_input = P.has_stage ? P.stage_symbols_input : -1;
  for (int32_t i = 0; i < n && i < capacity; ++i) {
    if (modes) modes[i] = P.stage_modes[i];
    if (rows_symbol) rows_symbol[i] = P.stage_rows_symbol[i];
  }
  return FCP_OK;
}

int fcp_placement_assign(const int64_t *table_bytes, int32_t n_tables, int64_t hbm_bytes, int64_t reserve_bytes, int32_t world,
                         int32_t prefer_mode, int32_t *owner, fcp_placement_t *out) {
  if (!out || n_tables < 0 || (n_tables > 0 && !table_bytes) || hbm_bytes <= 0 || reserve_bytes < 0 || world < 1)
    return fail(FCP_ERR_INVALID_ARGUMENT, "bad placement arguments");
  if (prefer_mode != FCP_PLACE_COLUMN_SHARD && prefer_mode != FCP_PLACE_ROW_SHARD && prefer_mode != FCP_PLACE_MIXED)
    return fail(FCP_ERR_INVALID_ARGUMENT, "prefer_mode must be column sharding, row sharding or mixed");
  const int64_t budget = hbm_bytes - reserve_bytes;
  if (budget <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, "reserve_bytes leaves no room for tables");
  int64_t total = 0, largest = 0;
  for (int32_t t = 0; t < n_tables; ++t) {
    if (table_bytes[t] < 0) return fail(FCP_ERR_INVALID_ARGUMENT, "negative table size");
    total += table_bytes[t];
    largest = std::max(largest, table_bytes[t]);
  }
  out->min_world = (int32_t)std::max<int64_t>(1, (total + budget - 1) / budget);
  out->mode = FCP_PLACE_REPLICATE;
  out->bytes_per_gpu = total;
  if (owner)
    for (int32_t t = 0; t < n_tables; ++t) owner[t] = 0;
  if (total <= budget) return FCP_OK; // fits one GPU: replicas, no collective
  // row sharding: every table contributes ceil(rows / world) rows to every GPU (at most one row's worth of
  // rounding per table, ignored here: tables are >> one row)
  const int64_t row_share = (total + world - 1) / world;
  const bool row_ok = world > 1 && row_share <= budget;
  // whole tables, longest first onto the least loaded rank (longest-processing-time packing), on top of the row
  // share of the tables that are spread: `spread_over` = the threshold above which a table is spread by rows
  std::vector<int32_t> assign(n_tables, -1);
  int32_t n_whole = 0; // tables the last pack() left whole
  auto pack = [&](int64_t spread_over, int64_t *share) {
    int64_t spread = 0;
    std::vector<int32_t> order;
    for (int32_t t = 0; t < n_tables; ++t) {
      if (table_bytes[t] > spread_over) {
        spread += table_bytes[t];
        assign[t] = -1;
      } else {
        order.push_back(t);
      }
    }
    std::vector<int64_t> load(world, (spread + world - 1) / world);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return table_bytes[a] > table_bytes[b]; });
    for (int32_t t : order) {
      const int32_t r = (int32_t)(std::min_element(load.begin(), load.end()) - load.begin());
      load[r] += table_bytes[t];
      assign[t] = r;
    }
    *share = *std::max_element(load.begin(), load.end());
    n_whole = (int32_t)order.size();
    return *share <= budget;
  };
  int64_t col_share = 0, mixed_share = 0;
  const bool col_ok = world > 1 && largest <= budget && pack(INT64_MAX, &col_share);
  int mode;
  if (prefer_mode == FCP_PLACE_MIXED) {
    if (col_ok) mode = FCP_PLACE_COLUMN_SHARD;                                       // every table fits a GPU: no rows spread at all
    // (MIXED needs a whole table for every rank — the whole-column step gives every rank a block; with fewer, the few
    // small tables are spread by rows like the large ones: their partial sums are a rounding error on the wire)
    else if (world > 1 && largest > budget && pack(budget, &mixed_share) && n_whole >= world) mode = FCP_PLACE_MIXED;
    else if (row_ok) mode = FCP_PLACE_ROW_SHARD;
    else mode = -1;
  } else {
    if (!row_ok && !col_ok) mode = -1;
    else mode = (col_ok && (prefer_mode == FCP_PLACE_COLUMN_SHARD || !row_ok)) ? FCP_PLACE_COLUMN_SHARD : FCP_PLACE_ROW_SHARD;
  }
  if (mode < 0)
    return fail(FCP_ERR_UNSUPPORTED, "tables of " + std::to_string(total) + " bytes do not fit " + std::to_string(world) +
                                         " GPU(s) with " + std::to_string(budget) + " bytes each: needs at least " +
                                         std::to_string(out->min_world));
  out->mode = mode;
  if (mode == FCP_PLACE_COLUMN_SHARD) {
    (void)pack(INT64_MAX, &col_share); // (the mixed attempt may have run after it)
    out->bytes_per_gpu = col_share;
  } else if (mode == FCP_PLACE_MIXED) {
    out->bytes_per_gpu = mixed_share;
  } else {
    out->bytes_per_gpu = row_share;
    std::fill(assign.begin(), assign.end(), -1);
  }
  if (owner)
    for (int32_t t = 0; t < n_tables; ++t) owner[t] = assign[t];
  return FCP_OK;
}

int fcp_placement_decide(const int64_t *table_bytes, int32_t n_tables, int64_t hbm_bytes, int64_t reserve_bytes,
                         int32_t world, int32_t prefer_mode, fcp_placement_t *out) {
  return fcp_placement_assign(table_bytes, n_tables, hbm_bytes, reserve_bytes, world, prefer_mode, nullptr, out);
}

// Formats by budget, from the audits of fcp_table_audit (fcp_table_audit.hip; here they are host memory).  Per table the lower
// convex hull of (bytes, weighted error) over its admissible kinds, walked from float32 towards fewer bytes; all tables'
// hull steps in one list ordered by error added per byte saved, taken until the budget holds.  Every prefix of that list
// minimises error + lambda * bytes for the lambda of its last step, which is what makes the state optimal for the bytes it uses.
int fcp_table_formats_choose(const fcp_table_audit_t *audits, const int64_t *rows, const int32_t *dims, int32_t n_tables,
                             int64_t budget_bytes, uint32_t allowed_kinds, const double *table_weight, int32_t *kinds_out,
                             int64_t *bytes_out, double *error_out) {
  const char *who = "fcp_table_formats_choose: ";
  if (n_tables < 0) return fail(FCP_ERR_INVALID_ARGUMENT, std::string(who) + "n_tables is negative");
  if (n_tables > 0 && (!audits || !rows || !dims || !kinds_out))
    return fail(FCP_ERR_INVALID_ARGUMENT, std::string(who) + "audits, rows, dims or kinds_out is null");
  if (budget_bytes < 0) return fail(FCP_ERR_INVALID_ARGUMENT, std::string(who) + "budget_bytes is negative");
  struct Point {
    int kind;
    int64_t bytes;
    double err;
  };
  struct Step {
    double slope; // weighted error added per byte saved
    int32_t table, to;
  };
  std::vector<std::vector<Point>> hull(n_tables);
  std::vector<Step> steps;
  int64_t total = 0;
  for (int32_t t = 0; t < n_tables; ++t) {
    const std::string where = std::string(who) + "table " + std::to_string(t) + ": ";
    if (rows[t] < 0) return fail(FCP_ERR_INVALID_ARGUMENT, where + "rows is negative");
    if (dims[t] <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, where + "dim must be positive");
    const fcp_table_audit_t &a = audits[t];
    // (a sum of squares so small that its reciprocal overflows is a table of zeros to every format: weight 0, as for 0)
    const double w = table_weight ? table_weight[t] : (a.sum_sq > 0.0 && std::isfinite(1.0 / a.sum_sq) ? 1.0 / a.sum_sq : 0.0);
    if (!(w >= 0.0) || !std::isfinite(w)) return fail(FCP_ERR_INVALID_ARGUMENT, where + "weight is negative or not finite");
    std::vector<Point> pts;
    for (int k = 0; k < fcpf::kTabKinds; ++k) {
      int64_t bytes = 0;
      if (__builtin_mul_overflow(rows[t], fcpf::row_bytes(k, dims[t]), &bytes))
        return fail(FCP_ERR_INVALID_ARGUMENT, where + "rows x row bytes overflows 64 bits");
      if (k == FCP_TAB_F32) {
        pts.push_back({k, bytes, 0.0});
        continue;
      }
      if (!(allowed_kinds >> k & 1) || a.rows_nonfinite > 0 || a.kind[k].rows_bad > 0) continue;
      if (bytes >= pts[0].bytes) continue; // no smaller than float32, which loses nothing (q8 at dim 1 or 2)
      const double err = w * a.kind[k].sum_sq_err; // NaN or inf here would leave the steps without an order
      if (!(err >= 0.0) || !std::isfinite(err)) return fail(FCP_ERR_INVALID_ARGUMENT, where + "weight x sum_sq_err is negative or not finite");
      pts.push_back({k, bytes, err});
    }
    // most bytes first; equal bytes: the lower error, then the lower FCP_TAB_*, and only that one stays
    std::stable_sort(pts.begin(), pts.end(), [](const Point &p, const Point &q) {
      return p.bytes != q.bytes ? p.bytes > q.bytes : p.err != q.err ? p.err < q.err : p.kind < q.kind;
    });
    std::vector<Point> &h = hull[t];
    auto slope = [](const Point &p, const Point &q) { return (q.err - p.err) / (double)(p.bytes - q.bytes); };
    for (const Point &p : pts) {
      if (!h.empty() && p.bytes == h.back().bytes) continue;
      while (h.size() >= 2 && slope(h[h.size() - 2], h.back()) >= slope(h.back(), p)) h.pop_back();
      h.push_back(p);
    }
    for (size_t i = 1; i < h.size(); ++i) steps.push_back({slope(h[i - 1], h[i]), t, (int32_t)i});
    if (__builtin_add_overflow(total, h[0].bytes, &total)) return fail(FCP_ERR_INVALID_ARGUMENT, std::string(who) + "the float32 tables' bytes overflow 64 bits");
  }
  // (a table's slopes rise along its hull, so its steps stay in order)
  std::stable_sort(steps.begin(), steps.end(), [](const Step &p, const Step &q) {
    return p.slope != q.slope ? p.slope < q.slope : p.table != q.table ? p.table < q.table : p.to < q.to;
  });
  std::vector<int32_t> at(n_tables, 0);
  for (size_t i = 0; i < steps.size() && total > budget_bytes; ++i) {
    const Step &s = steps[i];
    total -= hull[s.table][s.to - 1].bytes - hull[s.table][s.to].bytes;
    at[s.table] = s.to;
  }
  if (bytes_out) *bytes_out = total;
  if (total > budget_bytes)
    return fail(FCP_ERR_UNSUPPORTED, std::string(who) + "the smallest admissible assignment needs " + std::to_string(total) + " bytes, the budget is " +
                                         std::to_string(budget_bytes));
  double error = 0.0;
  for (int32_t t = 0; t < n_tables; ++t) {
    kinds_out[t] = hull[t][at[t]].kind;
    error += hull[t][at[t]].err;
  }
  if (error_out) *error_out = error;
  return FCP_OK;
}

} // extern "C"
