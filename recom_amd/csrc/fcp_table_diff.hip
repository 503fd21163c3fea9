// fcp_table_diff.hip — fcp_table_diff / fcp_table_diff_workspace_bytes: which rows of a served table (FCP_TAB_F32 / _BF16 / _F16 /
// _Q8) would CHANGE if a new float32 master — or a replica in the table's own format — were written over them, found where the
// table lies, in one pass over the new rows and the stored rows and without a temporary table.  The answer is the delta
// fcp_table_update_rows (fcp_table_rows.hip) and fcp_table_digest_rows (fcp_table_digest.hip) take: ascending row ids, the
// changed source rows behind one another, -1 behind the ids.  A row is changed when the bytes fcp_table_convert (fcp_convert.hip)
// writes for its source differ from the bytes stored; the format's bytes are formed in registers by the text fcp_table_convert
// is made of — RowSlots, minmax and q8_code of fcp_table_walk.h, narrow_bf16 / narrow_f16 of fcp_fused_bodies.h — and nothing is
// written to the table.  The reference reads float32 tables only and has no counterpart.
//
// The changed rows are selected by the classify / fold / compact pipeline of fcp_select_compact.h.  The workspace holds, in
// this order: kDiffBlocks + 1 of its records (one per block of the fixed grid, and the totals) and one flag byte per row.
//
//   fcp_diff_classify_kernel<F, V, G>   the selection grid, kDiffBlocks blocks at the most; a position is a row of the call.
//                     A row is handled by the power-of-two group of G lanes the
//                     quantiser gives it (group_of), every lane owning V-element slots; a block takes 256 / G rows at a time,
//                     kDiffUnroll (G == 64: 2) of such steps at once — their loads are issued before the first compare.  F is
//                     what lies between the source and the stored bytes:
//                       kDiffBits32 / 16 / 8   nothing: a float32 master against a float32 table, or a replica against a table of
//                                      its own format — slots of 4 * V, 2 * V, V bytes compared as bits (q8: and the pair);
//                       kDiffN16       float32 -> bf16 / fp16: fl16 per element, as st_out_narrow packs a slot;
//                       kDiffQ8        float32 -> q8: quantize_row's two passes — min / max over the row (the first
//                                      slots_in_registers<G>() slots stay in registers, a longer row's tail is read again),
//                                      the group's butterflies, scale and inv, then the codes V at a time — with the stores
//                                      replaced by compares: codes through Q8Codes<V>, scale and bias as one pair through
//                                      Q8Pair<V> in the group's first lane, the loads ld_q8_raw makes of a row at any byte.
//                     The lanes' differences are ORed over the group by __shfl_xor butterflies.  One flag byte per row
//                     (1: changed) from the group's first lane, and ONE partial record per block: changed, first, last.
//                     Lanes of rows beyond the chunk take part in the exchanges and touch no memory.
//   fcp_diff_fold_kernel        one wave: the records' offsets (select_offsets), the totals record, the report.
//   fcp_diff_compact_kernel<V, G>   select_compact, a thread per row: changed row number k of the call, in ascending row index,
//                     writes ids_out[k] = row0 + its position; positions i >= m write the -1 tail.  V > 0: the changed
//                     source rows as bits, src[p_k] -> rows_out[k].  V == 0: ids only.
// Every output byte is a function of the arguments alone: the grid is fixed by `rows`, integer sums, minima and maxima are
// exact in any order, and there is no atomic.  Vector loads and stores only.
// No scratch (-Rpass-analysis=kernel-resource-usage: ScratchSize 0 for every kernel); LDS: the classify kernel's fold (4 wave
// records of 24 bytes: 96 bytes), the compact kernel's changed-row list and wave counts (1 KiB + 16 bytes), none in the fold.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off) // every operation of the quantiser rounds once, by itself: fcp_table_walk.h's rule

#include "fcp_table_walk.h" // RowSlots, minmax, q8_code, vec_of, group_of, with_vec, with_group: the rows' walk and the host's dispatch
#include "fcp_block_fold.h" // wave_fold, block_fold
#include "fcp_select_compact.h" // select_grid, select_offsets, select_compact, with_compact_shape: the selection's shared tail

namespace {

constexpr int kDiffThreads = FCP_BLOCK_THREADS;
constexpr int kDiffTile = kSelectTile;    // rows of one step of a compact block; a chunk is whole tiles
constexpr int kDiffBlocks = 2048;         // the fixed grid of classify / compact: 8 blocks on each of 256 CUs; also the partial records
constexpr int kDiffMinChunkTiles = 4;     // a block's chunk is at least this many tiles
constexpr int kDiffUnroll = 4;            // steps of 256 / G rows a classify block has in flight (G == 64: half of it)
static_assert(kDiffTile == kDiffThreads, "select_compact takes a thread per row of a tile");

// What a block of the classify phase found, and, once the fold has run, where its changed rows go.  32 bytes.
struct DiffPartial {
  int64_t changed;
  int64_t first, last; // positions in the call's rows; kNoFirst / -1 when nothing changed
  int64_t offset;      // changed rows of the blocks before this one (the totals record: unused)
};
static_assert(sizeof(DiffPartial) == 32 && sizeof(fcp_table_diff_report_t) == 32, "records of 32 bytes");
constexpr int64_t kNoFirst = INT64_MAX;

// what a lane, a wave, a block and the fold's lanes hold
struct DiffCounts {
  int64_t changed, first, last;
  __device__ operator DiffPartial() const { return DiffPartial{changed, first, last, 0}; }
};
__device__ __forceinline__ void fold(DiffCounts &a, const DiffCounts &b) {
  a.changed += b.changed;
  a.first = b.first < a.first ? b.first : a.first;
  a.last = b.last > a.last ? b.last : a.last;
}

enum { kDiffBits32 = 0, kDiffBits16 = 1, kDiffBits8 = 2, kDiffN16 = 3, kDiffQ8 = 4 };

// V elements of E bytes as one load: what a slot of a stored row is
template <int E, int V> struct DiffSlot;
template <int V> struct DiffSlot<4, V> : Words<V> {};
template <int V> struct DiffSlot<2, V> { typedef typename NarrowType<V>::T T; };
template <int V> struct DiffSlot<1, V> { typedef typename Q8Codes<V>::T T; };

template <class T> __device__ __forceinline__ T ld_bits(const char *p) { return *as_global(reinterpret_cast<const T *>(p)); }
template <int V> __device__ __forceinline__ uint64_t ld_pair(const char *p) { return *(const FCP_GLOBAL typename Q8Pair<V>::T *)(p); }

// non-zero when a and b differ in any bit
template <class T> __device__ __forceinline__ uint32_t differ(const T &a, const T &b) {
  if constexpr (sizeof(T) < 4) {
    return (uint32_t)(a ^ b);
  } else {
    uint32_t wa[sizeof(T) / 4], wb[sizeof(T) / 4], d = 0;
    __builtin_memcpy(wa, &a, sizeof(T));
    __builtin_memcpy(wb, &b, sizeof(T));
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 4; ++i) d |= wa[i] ^ wb[i];
    return d;
  }
}

// the 2 * V bytes st_out_narrow stores for a slot; kind: FCP_TAB_BF16 | FCP_TAB_F16, the same for every wave
template <int V> __device__ __forceinline__ typename NarrowType<V>::T narrow_slot(const VF<V> &v, int kind) {
  uint32_t h[V];
  if (kind == FCP_TAB_BF16) {
#pragma unroll
    for (int i = 0; i < V; ++i) h[i] = narrow_bf16(v.v[i]);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) h[i] = narrow_f16(v.v[i]);
  }
  typename NarrowType<V>::T t;
  if constexpr (V == 4) {
    t.x = h[0] | (h[1] << 16);
    t.y = h[2] | (h[3] << 16);
  } else if constexpr (V == 2) {
    t = h[0] | (h[1] << 16);
  } else {
    t = (uint16_t)h[0];
  }
  return t;
}

// the V bytes st_codes stores for a slot; element i in byte i
template <int V> __device__ __forceinline__ typename Q8Codes<V>::T code_slot(const VF<V> &x, float mn, float inv) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < V; ++i) c |= q8_code(x.v[i], mn, inv) << (8 * i);
  return (typename Q8Codes<V>::T)c;
}

// One row between its loads (front) and its verdict (back), as ONE lane of the row's G-lane group holds it: the lane's first
// slots_in_registers<G>() slots of the source and of the stored row.  EVERY lane of a wave calls both; lanes of a group that is
// not live take part in the exchanges and touch no memory.  trow / srow: the stored row's and the source row's first byte.
template <int F, int V, int G> struct DiffRow {
  static constexpr bool kFromF32 = F == kDiffN16 || F == kDiffQ8;
  static constexpr int E = F == kDiffBits32 ? 4 : (F == kDiffBits16 || F == kDiffN16) ? 2 : 1; // bytes of a stored element
  static constexpr int S = slots_in_registers<G>();
  typedef typename DiffSlot<E, V>::T TS;
  RowSlots<V, G> r; // the source's slots as float32 (kFromF32)
  TS x[S];          // the source's slots as the format's bits (a replica, or float32 against float32)
  TS t[S];          // the stored slots
  uint64_t tpair, xpair;
  float mn, mx;

  __device__ __forceinline__ void front(const char *trow, const char *srow, int dim, int lane, bool live) {
    const int nslots = dim / V;
    mn = __builtin_inff(), mx = -__builtin_inff();
    if constexpr (F == kDiffQ8) // quantize_row's pass one: the kept slots, then the tail's min and max
      r.load(reinterpret_cast<const float *>(srow), nslots, lane, live, [&](const VF<V> &v) { minmax<V>(v, mn, mx); });
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int slot = lane + k * G;
      x[k] = t[k] = TS{};
      if constexpr (F == kDiffN16) r.x[k] = vzero<V>();
      if (live && slot < nslots) {
        if constexpr (F == kDiffN16) r.x[k] = ld_f32<V>(reinterpret_cast<const float *>(srow) + (int64_t)slot * V);
        if constexpr (!kFromF32) x[k] = ld_bits<TS>(srow + (int64_t)slot * sizeof(TS));
        t[k] = ld_bits<TS>(trow + (int64_t)slot * sizeof(TS));
      }
    }
    tpair = xpair = 0;
    if constexpr (E == 1) { // a q8 row's scale and bias: the group's first lane
      if (live && lane == 0) {
        tpair = ld_pair<V>(trow + dim);
        if constexpr (F == kDiffBits8) xpair = ld_pair<V>(srow + dim);
      }
    }
  }

  // non-zero when something this lane holds of the row differs from what is stored
  __device__ __forceinline__ uint32_t back(const char *trow, const char *srow, int dim, int kind, int lane, bool live) {
    const int nslots = dim / V;
    float inv = 0.0f;
    if constexpr (F == kDiffQ8) { // quantize_row, from the group's min and max to the pair
#pragma unroll
      for (int m = G / 2; m >= 1; m >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, m, 64));
        mx = fmaxf(mx, __shfl_xor(mx, m, 64));
      }
      const float range = mx - mn;
      const float scale = range / 255.0f;
      inv = 255.0f / (range + 1e-8f);
      xpair = (uint64_t)__float_as_uint(scale) | ((uint64_t)__float_as_uint(mn) << 32);
    }
    if (!live) return 0;
    const float *frow = reinterpret_cast<const float *>(srow);
    const auto formed = [&](const VF<V> &v) {
      if constexpr (F == kDiffQ8)
        return code_slot<V>(v, mn, inv);
      else
        return narrow_slot<V>(v, kind);
    };
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      if (lane + k * G < nslots) {
        if constexpr (kFromF32)
          d |= differ<TS>(formed(r.x[k]), t[k]);
        else
          d |= differ<TS>(x[k], t[k]);
      }
    }
    if constexpr (G == 64) {
      for (int slot = lane + S * G; slot < nslots; slot += G) { // beyond the register cap: both rows' tails, the source's again
        const TS stored = ld_bits<TS>(trow + (int64_t)slot * sizeof(TS));
        if constexpr (kFromF32)
          d |= differ<TS>(formed(ld_f32<V>(frow + (int64_t)slot * V)), stored);
        else
          d |= differ<TS>(ld_bits<TS>(srow + (int64_t)slot * sizeof(TS)), stored);
      }
    }
    if constexpr (E == 1) {
      if (lane == 0) d |= differ<uint64_t>(xpair, tpair);
    }
    return d;
  }
};

struct DiffClassify {
  const char *table, *src; // the table's base; the first source row
  int64_t row0, rows, chunk;
  int64_t trb, srb;        // bytes of a stored row and of a source row
  int32_t dim, kind;
  uint8_t *flags;
  DiffPartial *partials;
};

// chunk: rows of a block, a multiple of kDiffTile; every thread of a block takes the same number of steps.  A group never
// straddles a wave, and it is live or not as a whole.
template <int F, int V, int G> __global__ void __launch_bounds__(kDiffThreads) fcp_diff_classify_kernel(const DiffClassify A) {
  constexpr int kRowsPerStep = kDiffThreads / G;
  constexpr int U = G == 64 ? kDiffUnroll / 2 : kDiffUnroll;
  const int tid = threadIdx.x;
  const int lane = tid & (G - 1);
  const int64_t c0 = (int64_t)blockIdx.x * A.chunk;
  const int64_t c1 = c0 + A.chunk < A.rows ? c0 + A.chunk : A.rows;
  DiffCounts c = {0, kNoFirst, -1};
  for (int64_t t0 = c0; t0 < c1; t0 += U * kRowsPerStep) {
    DiffRow<F, V, G> row[U];
    const char *trow[U], *srow[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = t0 + u * kRowsPerStep + tid / G;
      live[u] = i < c1;
      trow[u] = A.table + (live[u] ? A.row0 + i : 0) * A.trb;
      srow[u] = A.src + (live[u] ? i : 0) * A.srb;
      row[u].front(trow[u], srow[u], A.dim, lane, live[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = t0 + u * kRowsPerStep + tid / G;
      uint32_t d = row[u].back(trow[u], srow[u], A.dim, A.kind, lane, live[u]);
#pragma unroll
      for (int m = G / 2; m >= 1; m >>= 1) d |= __shfl_xor(d, m, 64);
      if (live[u] && lane == 0) {
        *as_global(A.flags + i) = d != 0 ? 1 : 0;
        if (d != 0) {
          ++c.changed;
          c.first = i < c.first ? i : c.first;
          c.last = i; // (a lane's rows ascend)
        }
      }
    }
  }
  block_fold(c, A.partials);
}

// one wave; lane l owns the records [l * per, (l + 1) * per) of the nblocks the classify phase wrote (0: it was not launched)
__global__ void __launch_bounds__(64)
    fcp_diff_fold_kernel(DiffPartial *partials, int32_t nblocks, int64_t row0, int64_t rows, fcp_table_diff_report_t *report) {
  constexpr int per = kDiffBlocks / 64;
  const int lane = threadIdx.x;
  const int b0 = lane * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  DiffCounts c = {0, kNoFirst, -1};
  for (int b = b0; b < b1; ++b) fold(c, DiffCounts{partials[b].changed, partials[b].first, partials[b].last});
  select_offsets<kDiffBlocks>(partials, nblocks, c.changed);
  wave_fold(c);
  if (lane != 0) return;
  partials[kDiffBlocks] = c;
  fcp_table_diff_report_t r;
  r.rows = rows;
  r.changed = c.changed;
  r.first_changed = c.changed ? row0 + c.first : -1;
  r.last_changed = c.changed ? row0 + c.last : -1;
  *report = r;
}

struct DiffCompact {
  const float *src;
  const uint8_t *flags;
  const DiffPartial *partials;
  int64_t *ids_out;
  float *rows_out;
  int64_t row0, rows, chunk;
  int32_t dim;
};

// what select_compact asks of the unit: nothing to bring along, a changed row's table index, the -1 tail
struct DiffEmit {
  const DiffCompact &A;
  __device__ __forceinline__ int prepare(int64_t, bool) const { return 0; }
  __device__ __forceinline__ void emit(int64_t k, int64_t i, int) const { *as_global(A.ids_out + k) = A.row0 + i; }
  __device__ __forceinline__ void tail(int64_t i) const { *as_global(A.ids_out + i) = -1; }
};

// V == 0: ids only (rows_out is null and src is never read); else G lanes copy a changed row, V words at a time
template <int V, int G> __global__ void __launch_bounds__(kDiffThreads) fcp_diff_compact_kernel(const DiffCompact A) {
  select_compact<V, G, kDiffBlocks>(A.flags, A.partials, A.rows, A.chunk, A.src, A.rows_out, A.dim, DiffEmit{A});
}

int64_t partial_bytes() { return (int64_t)(kDiffBlocks + 1) * (int64_t)sizeof(DiffPartial); }

template <int F> void launch_classify(const DiffClassify &A, int vec, int nblocks, hipStream_t s) {
  with_vec(vec, [&](auto v) {
    with_group(group_of(A.dim, vec), [&](auto g) {
      hipLaunchKernelGGL((fcp_diff_classify_kernel<F, decltype(v)::value, decltype(g)::value>), dim3(nblocks), dim3(kDiffThreads), 0, s, A);
    });
  });
}

} // namespace

extern "C" int64_t fcp_table_diff_workspace_bytes(int64_t rows) {
  if (rows < 0 || rows >= fcpf::kRowLimit) return -1;
  return partial_bytes() + (rows + 7) / 8 * 8;
}

extern "C" int fcp_table_diff(const void *table, int32_t kind, int64_t table_rows, int32_t dim, const void *src, int32_t src_kind,
                              int64_t row0, int64_t rows, int64_t *ids_out, float *rows_out, fcp_table_diff_report_t *report,
                              void *workspace, int32_t device, void *stream) {
  const std::string w = "fcp_table_diff: ";
  if (rows < 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`rows` is negative");
  if (const std::string why = fcpf::row_limit_refusal("rows", rows, table_rows); !why.empty()) return fail(FCP_ERR_INVALID_ARGUMENT, w + why);
  if (row0 < 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`row0` is negative");
  if (row0 > table_rows - rows) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`row0` + rows must not exceed table_rows");
  if (dim <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`dim` must be positive");
  if (!fcpf::known_tab_kind(kind)) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`kind` is no FCP_TAB_* value");
  if (src_kind != FCP_TAB_F32 && src_kind != kind)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`src_kind` is FCP_TAB_F32 (a float32 master) or the table's kind (a replica)");
  if (rows_out && src_kind != FCP_TAB_F32)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`rows_out` with a " + kind_name(src_kind) + " source: a replica gives ids only");
  if (!report) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`report` is null");
  if (!workspace) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`workspace` is null");
  if (rows > 0 && !table) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`table` is null");
  if (rows > 0 && !src) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`src` is null");
  if (rows > 0 && !ids_out) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`ids_out` is null");
  const int vec = vec_of(dim);
  if ((uintptr_t)table % fcpf::base_alignment(kind, vec))
    return fail(FCP_ERR_INVALID_ARGUMENT,
                w + fcpf::not_aligned("table", fcpf::base_alignment(kind, vec), std::string(" (a ") + kind_name(kind) + " table of this dim)"));
  if ((uintptr_t)src % fcpf::base_alignment(src_kind, vec))
    return fail(FCP_ERR_INVALID_ARGUMENT,
                w + fcpf::not_aligned("src", fcpf::base_alignment(src_kind, vec), std::string(" (") + kind_name(src_kind) + " rows of this dim)"));
  if ((uintptr_t)ids_out % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + fcpf::not_aligned("ids_out", 8));
  if ((uintptr_t)rows_out % (4 * vec)) return fail(FCP_ERR_INVALID_ARGUMENT, w + fcpf::not_aligned("rows_out", 4 * vec, " (float32 rows of this dim)"));
  if ((uintptr_t)report % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + fcpf::not_aligned("report", 8));
  if ((uintptr_t)workspace % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + fcpf::not_aligned("workspace", 8));

  DiffPartial *partials = static_cast<DiffPartial *>(workspace);
  uint8_t *flags = static_cast<uint8_t *>(workspace) + partial_bytes();
  const auto grid = select_grid(rows, kDiffBlocks, kDiffMinChunkTiles); // of classify and compact
  DiffClassify A;
  A.table = static_cast<const char *>(table);
  A.src = static_cast<const char *>(src);
  A.row0 = row0;
  A.rows = rows;
  A.chunk = grid.chunk;
  A.trb = fcpf::row_bytes(kind, dim);
  A.srb = fcpf::row_bytes(src_kind, dim);
  A.dim = dim;
  A.kind = kind;
  A.flags = flags;
  A.partials = partials;
  DiffCompact B;
  B.src = static_cast<const float *>(src);
  B.flags = flags;
  B.partials = partials;
  B.ids_out = ids_out;
  B.rows_out = rows_out;
  B.row0 = row0;
  B.rows = rows;
  B.chunk = grid.chunk;
  B.dim = dim;
  return on_device("fcp_table_diff", device, stream, [&](hipStream_t s) {
    if (rows > 0) {
      if (src_kind == kind)
        kind == FCP_TAB_F32 ? launch_classify<kDiffBits32>(A, vec, grid.nblocks, s)
                            : kind == FCP_TAB_Q8 ? launch_classify<kDiffBits8>(A, vec, grid.nblocks, s) : launch_classify<kDiffBits16>(A, vec, grid.nblocks, s);
      else
        kind == FCP_TAB_Q8 ? launch_classify<kDiffQ8>(A, vec, grid.nblocks, s) : launch_classify<kDiffN16>(A, vec, grid.nblocks, s);
    }
    hipLaunchKernelGGL(fcp_diff_fold_kernel, dim3(1), dim3(64), 0, s, partials, (int32_t)grid.nblocks, row0, rows, report);
    if (rows == 0) return;
    with_compact_shape(rows_out != nullptr, dim, vec, [&](auto v, auto g) {
      hipLaunchKernelGGL((fcp_diff_compact_kernel<decltype(v)::value, decltype(g)::value>), dim3(grid.nblocks), dim3(kDiffThreads), 0, s, B);
    });
  });
}
