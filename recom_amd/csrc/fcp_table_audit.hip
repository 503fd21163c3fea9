// fcp_table_audit.hip — fcp_table_audit / fcp_table_audit_weighted / fcp_table_audit_workspace_bytes: what a float32 table (or the float32 rows of a delta)
// would lose in each of the compact formats the plans read (FCP_TAB_BF16 / _F16 / _Q8), and which of its rows a format
// cannot hold at all, judged on the device in ONE pass over the source — before fcp_table_convert or fcp_table_update_rows
// writes a single byte.  The reference reads float32 tables only and has no counterpart.
//
//   fcp_table_audit_kernel<V, G, WEIGHTED>   walks a row through RowSlots<V, G> (fcp_table_walk.h), the walk quantize_row uses — so the same 3 V x 7 G
//                     matrix, the same power-of-two group of G <= 64 lanes per row, loads of V = 4 | 2 | 1 elements, the row
//                     kept in registers between the two passes (kQSlots slots per lane of a 64-lane group; what lies beyond
//                     is read a second time).  A lane meets its slots in the same order in both passes: increasing k, then
//                     the tail in increasing slot.  Pass one (load): min, max and the largest |x| as a bit
//                     pattern — it says whether an element is NaN or +-inf, whether one's bf16 image is +-inf, whether one's
//                     fp16 image is —, joined over the group by __shfl_xor butterflies (order-free).  Pass two, per element x, all in
//                     float32 with every operation rounded once:
//                       bf16 / fp16   e = x - widen16(fl16(x)): narrow_bf16 / the hardware fp16 conversion and the exact widening,
//                                     the st_out_narrow / widen16 pair of fcp_fused_bodies.h without the store in between;
//                       q8            e = x - fma(code, scale, mn) with range, scale, inv and code formed as the quantiser forms
//                                     them and the fma ld_q8's.
//                     (double)e * e is exact; a lane adds it to its own float64 sums (one v_fma_f64), |e| to its own maxima, only for rows the
//                     kind can hold (the flags are the group's by then), so no NaN reaches a sum.  The group's first lane
//                     counts rows and keeps the smallest bad row index.  The grid is fixed (kAuditBlocks, fewer when the rows
//                     do not fill it); blocks walk the rows with a 64-bit grid-stride loop.  At the end a block folds its lanes
//                     — butterflies inside a wave, its four waves through one record each in LDS, in wave order — and writes
//                     ONE partial record to the workspace.
//                     <V, G, WEIGHTED> (fcp_table_audit_weighted): the same kernel with each term of the sums multiplied by
//                     the row's read count (uint32, what fcp_table_count_ids fills; exact in float64) inside the one
//                     v_fma_f64 — flags, counts of bad rows, first rows and maxima untouched.  The unweighted instantiations
//                     never read row_counts.
//   fcp_table_audit_fold_kernel    one wave: lane l folds records l, l + 64, ... in block order, a butterfly joins the lanes,
//                     lane 0 writes fcp_table_audit_t.  rows == 0 launches it alone (no record): zeros, every first_* -1.
// No floating-point atomics, no atomics at all: which lane adds which row is a function of (rows, dim) alone, every sum has one
// fixed order, and two calls on the same input leave the same bytes.  float64 sums of n non-negative terms: within n * 2^-53
// of the exact sum, relative, in any order (so within n * 2^-52 of any other such summation, which is what the tests hold).
//
// No scratch; LDS only for the 4 wave records of a block's fold.  The default modes of the other units (denormals kept,
// IEEE).  Contraction is off from here to the end of the file, as in fcp_convert.hip: every operation rounds once, by itself.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off)

#include "fcp_table_walk.h" // (behind the pragma: its code rounds every operation once, too)
#include "fcp_block_fold.h" // wave_fold, block_fold, kNoSuchRow: the fold of a lane's record into the block's, in one fixed order

static_assert(FCP_TAB_BF16 == 1 && FCP_TAB_F16 == 2 && FCP_TAB_Q8 == 3, "the audit's kind index k is FCP_TAB_* - 1");

namespace {

constexpr int kAuditBlocks = 2048;   // the fixed grid: 8 blocks of 256 threads on each of 256 CUs; also the records of the workspace

// What a lane, a wave, a block and the whole call have seen; k = FCP_TAB_* - 1.  96 bytes, 8-byte aligned.
struct AuditPartial {
  double sum_sq, sse[3];
  int64_t nonfinite, bad[3];
  uint32_t first_nonfinite, first_bad[3];
  float max_err[3];
  uint32_t pad;
};
static_assert(sizeof(AuditPartial) == 96, "the workspace is kAuditBlocks records of 96 bytes");

// widen16(fl16(x)) of one element: the bf16 pattern moves back to the high half; fp16 is v_cvt_f16_f32 then v_cvt_f32_f16
__device__ __forceinline__ float rt_bf16(float x) { return __uint_as_float(narrow_bf16(x) << 16); }
__device__ __forceinline__ float rt_f16(float x) {
  const uint16_t b = (uint16_t)narrow_f16(x);
  _Float16 h;
  __builtin_memcpy(&h, &b, 2);
  return (float)h;
}
__device__ __forceinline__ bool is_inf_or_nan(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

// |x| as a bit pattern orders like |x|, with every NaN above +inf: a row's largest pattern says whether an element is NaN or
// +-inf, and whether one rounds to +-inf in a 16-bit kind.  narrow_bf16 carries into the exponent from 0x7F7F8000 on (the
// tie above the largest bf16, 0x7F7F, goes to the even neighbour: inf); v_cvt_f16_f32 gives inf from 65520 on (likewise the
// tie above 65504).  (The tests hold the counts to the conversions themselves.)
constexpr uint32_t kAbsInf = 0x7F800000u, kAbsBf16Inf = 0x7F7F8000u, kAbsF16Inf = 0x477FF000u;

template <int V> __device__ __forceinline__ void look(const VF<V> &x, float &mn, float &mx, uint32_t &amax) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    mn = fminf(mn, x.v[i]);
    mx = fmaxf(mx, x.v[i]);
    amax = max(amax, __float_as_uint(x.v[i]) & 0x7FFFFFFFu);
  }
}

// (max_err as the bit pattern of |e|: errors of good rows are finite, and patterns of non-negative floats order as integers)
struct LaneSums {
  double sum_sq = 0.0, sse[3] = {0.0, 0.0, 0.0};
  uint32_t max_err[3] = {0, 0, 0};
  uint32_t nonfinite = 0, bad[3] = {0, 0, 0};
  uint32_t first_nonfinite = kNoSuchRow, first_bad[3] = {kNoSuchRow, kNoSuchRow, kNoSuchRow};
};

// one term: the square is exact in float64, and the fused multiply-add rounds the sum once.  WEIGHTED: the term is w * e * e
// with w the row's count (exact in float64), still ONE rounding of the sum — the product of the two squares' factors is formed
// exactly first (contraction is off: the multiply stays a multiply), then fma(w, e * e, sum).  w == 1 gives the bits of the
// unweighted form, w == 0 adds +0.  The maxima are never weighted.
template <bool WEIGHTED> __device__ __forceinline__ void add_sq(double &sum, uint32_t *max_bits, float e, double w) {
  if constexpr (WEIGHTED)
    sum = __builtin_fma(w, (double)e * (double)e, sum);
  else
    sum = __builtin_fma((double)e, (double)e, sum);
  if (max_bits) *max_bits = max(*max_bits, __float_as_uint(e) & 0x7FFFFFFFu);
}

// good: bit k set = kind k holds this row; the row is finite (the caller skips the others)
template <int V, bool WEIGHTED>
__device__ __forceinline__ void judge(const VF<V> &x, uint32_t good, float mn, float scale, float inv, double w, LaneSums &a) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const float v = x.v[i];
    add_sq<WEIGHTED>(a.sum_sq, nullptr, v, w);
    if (good & 1) add_sq<WEIGHTED>(a.sse[0], &a.max_err[0], v - rt_bf16(v), w);
    if (good & 2) add_sq<WEIGHTED>(a.sse[1], &a.max_err[1], v - rt_f16(v), w);
    if (good & 4) {
      const float code = (float)q8_code(v, mn, inv);
      add_sq<WEIGHTED>(a.sse[2], &a.max_err[2], v - __builtin_fmaf(code, scale, mn), w);
    }
  }
}

__device__ __forceinline__ void fold(AuditPartial &a, const AuditPartial &b) {
  a.sum_sq += b.sum_sq;
  a.nonfinite += b.nonfinite;
  a.first_nonfinite = min(a.first_nonfinite, b.first_nonfinite);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.sse[k] += b.sse[k];
    a.bad[k] += b.bad[k];
    a.first_bad[k] = min(a.first_bad[k], b.first_bad[k]);
    a.max_err[k] = fmaxf(a.max_err[k], b.max_err[k]);
  }
}

__device__ __forceinline__ AuditPartial nothing_seen() {
  AuditPartial p;
  p.sum_sq = 0.0;
  p.nonfinite = 0;
  p.first_nonfinite = kNoSuchRow;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p.sse[k] = 0.0;
    p.bad[k] = 0;
    p.first_bad[k] = kNoSuchRow;
    p.max_err[k] = 0.0f;
  }
  p.pad = 0;
  return p;
}

// src: the table's base; rows: all of them (< 2^32 - 3).  Block = 256 / G rows per step of the stride loop; a group never
// straddles a wave, and it is live or not as a whole — lanes of rows beyond the end take part in the butterflies and touch no
// memory.  Every thread of a block takes the same number of steps.
// WEIGHTED (fcp_table_audit_weighted): row_counts[row] weighs the row's terms of the sums and nothing else — every lane of the
// group loads the same dword (one address, issued with the row's first loads); the flags, the counts of bad rows, the first
// rows and the maxima are the unweighted kernel's.  The unweighted instantiations never read row_counts (the last argument).
template <int V, int G, bool WEIGHTED>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_table_audit_kernel(const float *src, int64_t rows, int32_t dim, AuditPartial *partials, const uint32_t *row_counts) {
  constexpr int kRowsPerBlock = FCP_BLOCK_THREADS / G;
  const int tid = threadIdx.x;
  const int lane = tid & (G - 1);
  const int nslots = dim / V;
  LaneSums a;
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < rows; base += (int64_t)gridDim.x * kRowsPerBlock) {
    const int64_t row = base + tid / G;
    const bool live = row < rows;
    const float *srow = src + row * dim;
    double w = 1.0;
    if constexpr (WEIGHTED) w = live ? (double)*as_global(row_counts + row) : 0.0;

    RowSlots<V, G> r;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    uint32_t amax = 0;
    r.load(srow, nslots, lane, live, [&](const VF<V> &x) { look<V>(x, mn, mx, amax); });
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, m, 64));
      mx = fmaxf(mx, __shfl_xor(mx, m, 64));
      amax = max(amax, __shfl_xor(amax, m, 64));
    }
    const float range = mx - mn;
    const float scale = range / 255.0f;
    const float inv = 255.0f / (range + 1e-8f);
    const uint32_t r32 = (uint32_t)row;
    if (live && amax >= kAbsInf) {
      if (lane == 0) {
        ++a.nonfinite;
        a.first_nonfinite = min(a.first_nonfinite, r32);
      }
    } else if (live) {
      // finite elements: mx - mn is finite or it overflowed to +inf
      const uint32_t bad = (amax >= kAbsBf16Inf ? 1u : 0u) | (amax >= kAbsF16Inf ? 2u : 0u) | (is_inf_or_nan(range) ? 4u : 0u);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (bad >> k & 1) {
            ++a.bad[k];
            a.first_bad[k] = min(a.first_bad[k], r32);
          }
      }
      const uint32_t good = ~bad & 7u;
      r.again(srow, nslots, lane, [&](int, const VF<V> &x) { judge<V, WEIGHTED>(x, good, mn, scale, inv, w, a); });
    }
  }

  AuditPartial p;
  p.sum_sq = a.sum_sq;
  p.nonfinite = a.nonfinite;
  p.first_nonfinite = a.first_nonfinite;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p.sse[k] = a.sse[k];
    p.bad[k] = a.bad[k];
    p.first_bad[k] = a.first_bad[k];
    p.max_err[k] = __uint_as_float(a.max_err[k]);
  }
  p.pad = 0;
  block_fold(p, partials);
}

// one wave; n: records of the workspace the first kernel wrote (0: it was not launched)
__global__ void __launch_bounds__(64) fcp_table_audit_fold_kernel(const AuditPartial *partials, int32_t n, int64_t rows, fcp_table_audit_t *out) {
  const int lane = threadIdx.x;
  AuditPartial p = nothing_seen();
  for (int i = lane; i < n; i += 64) fold(p, partials[i]);
  wave_fold(p);
  if (lane != 0) return;
  fcp_table_audit_t r;
  r.rows = rows;
  r.rows_nonfinite = p.nonfinite;
  r.first_nonfinite_row = p.first_nonfinite == kNoSuchRow ? -1 : (int64_t)p.first_nonfinite;
  r.sum_sq = p.sum_sq;
  r.kind[FCP_TAB_F32].rows_bad = 0;
  r.kind[FCP_TAB_F32].first_bad_row = -1;
  r.kind[FCP_TAB_F32].sum_sq_err = 0.0;
  r.kind[FCP_TAB_F32].max_abs_err = 0.0f;
  r.kind[FCP_TAB_F32].reserved = 0;
  for (int k = 0; k < 3; ++k) {
    r.kind[k + 1].rows_bad = p.bad[k];
    r.kind[k + 1].first_bad_row = p.first_bad[k] == kNoSuchRow ? -1 : (int64_t)p.first_bad[k];
    r.kind[k + 1].sum_sq_err = p.sse[k];
    r.kind[k + 1].max_abs_err = p.max_err[k];
    r.kind[k + 1].reserved = 0;
  }
  *out = r;
}

// blocks: what the rows fill of the fixed grid; row_counts: null = the unweighted kernels
template <int V, int G>
void audit_rows(const float *src, int64_t rows, int dim, int blocks, AuditPartial *partials, const uint32_t *row_counts, hipStream_t s) {
  if (row_counts)
    hipLaunchKernelGGL((fcp_table_audit_kernel<V, G, true>), dim3(blocks), dim3(FCP_BLOCK_THREADS), 0, s, src, rows, (int32_t)dim, partials,
                       row_counts);
  else
    hipLaunchKernelGGL((fcp_table_audit_kernel<V, G, false>), dim3(blocks), dim3(FCP_BLOCK_THREADS), 0, s, src, rows, (int32_t)dim, partials,
                       row_counts);
}

// Both entries: `who` names the entry in fcp_last_error; weighted: row_counts is an argument (checked, and handed to the kernels).
int audit_entry(const char *who, const float *src, int64_t rows, int32_t dim, bool weighted, const uint32_t *row_counts,
                fcp_table_audit_t *out, void *workspace, int32_t device, void *stream) {
  const std::string w = std::string(who) + ": ";
  if (rows < 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "rows is negative");
  if (dim <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "dim must be positive");
  if (!out) return fail(FCP_ERR_INVALID_ARGUMENT, w + "out is null");
  if (!workspace) return fail(FCP_ERR_INVALID_ARGUMENT, w + "workspace is null");
  if (rows > 0 && !src) return fail(FCP_ERR_INVALID_ARGUMENT, w + "src is null");
  if (weighted && rows > 0 && !row_counts) return fail(FCP_ERR_INVALID_ARGUMENT, w + "row_counts is null");
  if (rows >= fcpf::kRowLimit) return fail(FCP_ERR_INVALID_ARGUMENT, w + "rows must stay below 2^32 - 3, a plan's row limit");
  const int vec = vec_of(dim);
  if ((uintptr_t)src % (4 * vec))
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "src is not " + std::to_string(4 * vec) + "-byte aligned (a float32 table of this dim)");
  if (weighted && (uintptr_t)row_counts % 4) return fail(FCP_ERR_INVALID_ARGUMENT, w + "row_counts is not 4-byte aligned");
  if ((uintptr_t)out % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + "out is not 8-byte aligned");
  if ((uintptr_t)workspace % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + "workspace is not 8-byte aligned");
  AuditPartial *partials = static_cast<AuditPartial *>(workspace);
  const int g = group_of(dim, vec);
  const int64_t rows_per_block = FCP_BLOCK_THREADS / g;
  const int blocks = (int)std::min<int64_t>(kAuditBlocks, (rows + rows_per_block - 1) / rows_per_block);
  const uint32_t *counts = weighted ? row_counts : nullptr;
  return on_device(who, device, stream, [&](hipStream_t s) {
    if (blocks > 0) // (rows > 0: a weighted call's row_counts is not null)
      with_vec(vec, [&](auto v) {
        with_group(g, [&](auto gg) { audit_rows<decltype(v)::value, decltype(gg)::value>(src, rows, dim, blocks, partials, counts, s); });
      });
    hipLaunchKernelGGL(fcp_table_audit_fold_kernel, dim3(1), dim3(64), 0, s, partials, (int32_t)blocks, rows, out);
  });
}

} // namespace

extern "C" int64_t fcp_table_audit_workspace_bytes(void) { return (int64_t)kAuditBlocks * (int64_t)sizeof(AuditPartial); }

extern "C" int fcp_table_audit(const float *src, int64_t rows, int32_t dim, fcp_table_audit_t *out, void *workspace, int32_t device,
                               void *stream) {
  return audit_entry("fcp_table_audit", src, rows, dim, false, nullptr, out, workspace, device, stream);
}

extern "C" int fcp_table_audit_weighted(const float *src, int64_t rows, int32_t dim, const uint32_t *row_counts, fcp_table_audit_t *out,
                                        void *workspace, int32_t device, void *stream) {
  return audit_entry("fcp_table_audit_weighted", src, rows, dim, true, row_counts, out, workspace, device, stream);
}
