// fcp_plan_shape.h — the host half of a plan (fcp_plan_shape.cc): everything plan creation decides without a device, and the
// one routine that turns a request's shapes into column records, arena layout and launch geometry.  No GPU header: the unit
// is ordinary C++ and can be linked, and tested under sanitizers, without the HIP runtime (tests/native/plan_shape_san.cc).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fcp_hip.h"
#include "fcp_internal.h"
#include "fcp_env.h"
#include "fcp_formats.h"
#include "fcp_plan_desc.h"

namespace fcph {

inline int64_t align128(int64_t x) { return (x + 127) / 128 * 128; } // alignmem, cuda_emitter.cc:967-969

constexpr uint32_t kFlagHostOnly = FCP_FLAG_HOST_ONLY; // plan without device resources (layout queries)

struct HostColumn {
  fcp_column_desc_t d;
  fcp_column_ext_t ext = {}; // extensions (segment-id map); all zeros = none
  std::vector<float> boundaries;
  int32_t weights_input = -1; // host input of the per-id weights (fcp_column_ext_t::weights_input1 - 1), or -1
  std::vector<int64_t> xf_lo, xf_hi; // id transform intervals (closed)
  int64_t xf_const_off = -1;         // byte offset in the const buffer of intervals 1.. as (lo, hi) pairs
  int32_t out_off = 0;
  int64_t const_off = -1; // byte offset of the boundaries in the const buffer
};

struct DynMeta {
  std::vector<int32_t> group_rows;
  std::vector<int64_t> group_base;
  int64_t arena_bytes = 0;
  int64_t csr_arena_off = 0;
  int32_t max_seg_nnz = 0;
  int32_t max_lookup_nnz = 0; // longest id stream of a lookup column (GATHER, SEGMENT_REDUCE, GATHER_SCATTER): fcp_plan_traffic_count's grid
  int64_t seg_pairs = 0;   // sum of rows over the segment-id columns: cost of the in-block search
  bool seg_search = false; // this request: blocks search the segment ids (no pre-pass launch)
  bool plain = false;      // plain dense plan and at least 64 rows: the request takes fcp_dense_kernel_plain (its span image is built)
  int64_t work_bytes = 0;  // table rows gathered + output written: what decides whether a private lane pays (fcp_plan_set_private_streams)
  // regular CSR (FcpLaunch::csr_reg): 0 = none, 1 = the arena scratch laid out by column position, 2 = CSR inputs that lie
  // one stride apart in the blob; byte offset of position 0's array in the arena / the blob; stride in int32 elements
  int32_t csr_reg_mode = 0, csr_reg_stride = 0;
  int64_t csr_reg_base = 0;
  // launch geometry per kernel kind: [0] dense kernel (spans whose columns all have exactly
  // one source row per output row), [1] ragged kernel (spans with pooled / scatter / reduction columns)
  struct Geo {
    int32_t grid_blocks = 0;
    int32_t rows_per_wave = 1;
    FcpGroupLaunch groups[FCP_MAX_GROUPS];
  } geo[2];
};

// What evaluate_shapes reads of a column, in concat (pos) order: the request path walks this array and nothing of `cols`.
struct ColFacts {        // 32 bytes
  int64_t out_off_bytes; // concat layout: byte offset of the column in its group's row
  int32_t ids_input, seg_input, rows_arg, dim, seg_stride;
  uint8_t form, rows_source, seg_kind, group;
};
// ... and what it reads only of columns with a segment-id map or per-id weights: by position as well, in a loop of its own
// that only such plans run, so that the walk of every other plan streams 32 bytes per column and holds no map in a register
// (profiles/plan_shape_refactor.txt)
struct ColRare {
  int64_t map_factor;    // segment-id map with a symbol: the factor the symbol's value is multiplied by
  int32_t weights_input; // host input of the per-id weights, or -1
  int32_t map_sym;       // segment-id map: index of its symbol, or -1
  uint8_t has_map;       // the column's segment ids go through a map (the index matrix must hold whole rows)
  uint8_t map_sym_min;   // the smallest value the map's symbol may take (1 where it divides, else 0)
};

struct HostPlan {
  fcp::Env env; // the shipping environment switches as they were when the plan was created (fcp_env.h)
  fcp_plan_desc_t desc;
  std::vector<HostColumn> cols;
  std::vector<int32_t> ranks, elem_sizes, shape_off;
  int32_t rank_sum = 0;
  std::vector<int32_t> group_width, group_nslots, group_map_off; // (group_map_off: the prefix sum of group_nslots)
  std::vector<int32_t> seg_cols;
  int32_t n_seg_plain = 0;  // seg_cols[0 .. n_seg_plain): pooled columns; the rest: any-order ScatterNd columns (inverse maps)
  bool seg_search = false;  // blocks search the segment ids themselves; no segment-offset pre-pass
  bool has_inverse = false; // some ScatterNd column brings its row ids as delivered (any order): inverse map in the pre-pass
  // (r6) the CSR scratch of segment-id columns is laid out by column POSITION (one row of round32(rows + 1) entries per
  // column of the plan, pooled or not) instead of packed: the ragged body then knows where a range is before it has the
  // column's record (FcpLaunch::csr_reg).  One concat group, no any-order ScatterNd column (their inverse maps are the
  // scratch's tail, cleared per request), and pooled columns at least half of the plan (the unused rows cost arena bytes,
  // never traffic: RAGGED 512 of 512 columns; the reference's models E / F, 10-20 of ~1000, keep the packed scratch).
  bool csr_by_pos = false;
  // device arrays are kept in concat order (group-major, ascending concat offset)
  // so that the columns of one output span are contiguous: order[pos] = column,
  // pos_of[column] = pos.
  std::vector<int32_t> order, pos_of;
  // compact per-column facts in concat (pos) order + per group the first column that has rows of its own (-1: external
  // slots only): what evaluate_shapes walks on the request path
  std::vector<ColFacts> col_facts;
  std::vector<ColRare> col_rare; // plans with segment-id maps or per-id weights; else empty
  std::vector<int32_t> group_rep;
  int vec = 1;
  bool dense_only = true;   // no span needs the ragged kernel
  // hybrid dispatch: per group, the spans served by the dense kernel and by the ragged kernel
  std::vector<uint32_t> span_list;                 // host copy of d_span_list
  std::vector<int32_t> list_off[2], list_n[2];     // [kind][group]
  bool host_only = false;
  bool has_seg_map = false;
  // Per-id weights / the sqrtn combiner (fcp_weighted.hip).  has_weights: some pooled column has weights — every descriptor
  // slot then carries, behind its FcpColDyn records, one int64 per column (concat order): the byte offset of the column's
  // weights in the request's blob, or -1 (shape-dependent like the records, installed and uploaded with them; plans
  // without weighted columns have no such array).  weighted_kernel: has_weights, or some column's combiner is SQRTN — all
  // spans of the plan run the weighted ragged kernel.
  bool has_weights = false, weighted_kernel = false;
  // Which unit's fused kernels serve the plan (fcp_internal.h): decided once, when the plan is created, by check_desc
  // (fcp_plan_desc.h); the request path dispatches on it and on nothing else.
  FcpVariant variant = FCP_VAR_F32;
  bool wide_rows = false; // some table shard has >= 2^32 - 3 slots: FcpLaunch::store_through bit 1
  // narrow output (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16): the element type (FCP_OUT_*) and its size in bytes — every byte
  // quantity of the output region (group sizes, column bases, the position of the CSR scratch) is formed with out_elem
  int out_kind = FCP_OUT_F32, out_elem = 4;
  // 16-bit tables (FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16): the element type (FCP_TAB_*) of every table and its size in
  // bytes.  Geometry, slot offsets and wide_rows are in elements and do not depend on it; fcp_plan_table_bytes does
  int tab_kind = FCP_TAB_F32, tab_elem = 4;
  // 8-bit row-quantised tables (FCP_FLAG_TABLES_Q8): tab_kind FCP_TAB_Q8, tab_elem 1, and 8 bytes of scale and bias behind
  // every row.  Geometry stays in elements; the row STRIDE in slots, (dim + 8) / vec, is what scales a row index and what
  // wide_rows is decided from
  int tab_row_tail = 0;
  // Per-input table formats (FCP_FLAG_TABLES_PER_INPUT) whose tables really differ: tab_kind FCP_TAB_MIXED, tab_elem 0, and the
  // kind of every column's table (FCP_TAB_*, by plan column; FCP_TAB_F32 for columns without one) — it rides in bits 16..17
  // of the column record's flags.  Plans whose tables all have one kind are the plan-wide plan of that kind: col_kind empty.
  std::vector<int8_t> col_kind;
  bool tab_mixed() const { return !col_kind.empty(); }
  int col_tab_kind(size_t k) const { return col_kind.empty() ? tab_kind : col_kind[k]; }
  // bytes of one row of the table column k reads
  int64_t col_row_bytes(size_t k, int dim) const {
    return fcpf::row_bytes(col_tab_kind(k), dim);
  }
};

// Fills `p` from a descriptor that check_desc has passed (`facts` is what it learnt; its col_kind is taken over): the copy of
// the descriptor, the format facts, concat order and widths, the segment-id decisions, the compact column facts and the
// span lists of the hybrid dispatch — for device and host-only plans alike.  Refuses a table shard of 2^32 - 3 rows or more
// and a concat group no column names.  Reads FCP_DIAG=csr_by_pos and FCP_DIAG=wide_rows.
int build_host_plan(const fcp_plan_desc_t *desc, const fcp_column_ext_t *ext, PlanFacts &facts, HostPlan *p);

// Run-time shapes -> per-column dynamic records (`dyn`, one per column in concat order), arena layout and launch geometry
// (`m`).  Mirrors what the generated host code evaluates per call from SymEngine expressions (cuda_emitter.cc:2151-2179,
// :2410-2455).  `wts`: plans with weighted columns, else null — per column in concat order the byte offset of its weights in
// the blob, or -1.  `blob_bytes` < 0: the blob's size is not known (layout queries).
//
// On the request path whenever shapes change: one pass over col_facts (and one over col_rare where a plan has it), no
// allocation once this thread's scratch has grown, no environment lookup, and text is built only for a refusal.  A request
// with several faults is answered with the first one met, in this order:
//   1. the host inputs by index: a negative dimension, a negative offset, an input that ends beyond the blob;
//   2. the groups by index: a group of external slots only, then the row count of the group's first column in concat
//      order that has rows of its own (missing symbols, out of range);
//   3. the columns in concat order, each: its row count against its group's, its form's size rules, its segment input, and
//      the id or segment input it reads at an offset not divisible by 4 (inputs no column reads may lie anywhere);
//   4. plans with segment-id maps or per-id weights, their columns in concat order, each: the index matrix and the map's
//      symbol, then the weights' count and alignment;
//   5. the CSR scratch and the grid exceeding 2^31.
// (The per-column layout's cursor runs in plan column order in a loop of its own, which refuses nothing.)
int evaluate_shapes(const HostPlan &p, const int32_t *offsets, const int32_t *shapes, const int32_t *symbols, int64_t blob_bytes,
                    FcpColDyn *dyn, int64_t *wts, DynMeta *m);

} // namespace fcph
