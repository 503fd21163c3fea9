// fcp_outputs_compare.hip — fcp_outputs_compare / fcp_outputs_compare_workspace_bytes: what two requests' outputs differ by, per
// column, judged on the device in ONE pass over both arenas.  Two plans (float32 tables and the formats
// fcp_table_formats_choose picked, say) serve the same request into two arenas; this call, in stream order behind them, leaves
// one fcp_output_error_t per column and one for all columns together.  It reads what fcp_process_result_t names (column
// pointers, row strides in elements, shapes) and touches no plan, no serving kernel and no arena byte.  The reference has no
// counterpart.
//
//   fcp_outputs_compare_kernel<KA, KB>   nine instantiations, one per pair of element kinds (FCP_OUT_*): the element load
//                     is decided at compile time.  (The alternative, one kernel with the kind as a wave-uniform branch in the
//                     load, keeps both widenings and three load widths per side live in one body; the ISA of the templated
//                     form has one straight-line load + widen per side and width, the column record in SGPRs by scalar
//                     loads, 64 to 69 VGPRs and no scratch, so the nine small kernels stayed.)
//                     The load WIDTH is a block-uniform branch inside the kernel: V = 4 | 2 | 1 elements per lane, the largest
//                     that divides dim, both strides and both bases' element offsets — decided per column on the host, so a
//                     bf16 column at an odd element offset of a concat matrix is read by 2-byte loads and its neighbours by
//                     8-byte ones (float32: 16 | 8 | 4 bytes; 16-bit kinds: 8 | 4 | 2).
//                     Grid: n_columns * T blocks of 256 threads, block b = (column b / T, tile b % T), T =
//                     clamp(ceil(4096 / n_columns), 1, 64): a function of n_columns alone, so a 1000-column plan and a
//                     one-column plan both fill 256 CUs, and never of the data.  A column's rows are cut into row tiles of
//                     R rows — with S = dim / V slots per row, R = 256 / S whole rows when a row fits a block (lane t reads
//                     slot t % S of row t / S: the lanes of a wave read whole rows, contiguously), R = 1 and a loop over
//                     the row's slots in steps of 256 otherwise — and block (column, tile) takes the row tiles tile,
//                     tile + T, tile + 2T, ... (two in flight: both tiles' loads are issued before the first is judged, the
//                     judging stays in tile order).  The lane's place in a tile never changes, so the one integer division is
//                     in front of the loop.  Per pair, with a and b widened exactly (widen16 of fcp_fused_bodies.h):
//                       differ     the float32 bit patterns differ (+0 against -0 differs, a NaN against the same NaN does not);
//                       finite     neither is NaN or +-inf; only finite pairs enter the sums and the maxima:
//                       e = b - a  one float32 subtraction; (double)e * e and (double)a * a are exact and each joins its
//                                  float64 sum by ONE fma; |e| and |a| join float32 maxima (as bit patterns: e of a finite
//                                  pair is never NaN, and patterns of non-negative floats order as integers, +inf — an
//                                  overflowed subtraction — on top).
//                     A non-finite pair adds +0 to the sums through the same fma (x + 0 = x for the non-negative x these
//                     sums are), so the loop has no branch on the data.  Each lane keeps its own sums; at the end the block
//                     folds them — butterflies inside a wave, its four waves through one record each in LDS, in wave order —
//                     and writes ONE partial record at [column][tile] of the workspace.  Which lane adds which pair is a
//                     function of (shapes, strides' and bases' alignment, n_columns) alone.
//   fcp_outputs_compare_fold_kernel    one lane per column: folds the column's T records in tile order, writes out[k].
//   fcp_outputs_compare_total_kernel   a third launch of one wave: lane l folds the column records l, l + 64, ... in
//                     ascending order, a butterfly joins the lanes, lane 0 writes out[n_columns].  One fixed order, a function
//                     of n_columns alone.  (ONE block of 1024 threads doing both — a thread per column, then its 16 waves
//                     through LDS — was built and measured as well: that block alone took 12.5 us on S2's 1000 columns where
//                     these two launches take 4.5 + 6.4 us, and the call 57.7 us against 54.2: profiles/outputs_compare.txt.)
//
// No faults, no races, by construction.  The descriptors (one 48-byte record per column) are written into the workspace by the
// upload kernel in front, on the same stream.  Block (k, t) of the compare kernel writes the partial record [k * T + t] and no
// other byte, whether it met a row or not; the fold's lane k reads exactly the records [k * T, (k + 1) * T): every workspace
// record the fold reads is written by exactly one block of the same call, and stream order puts all of them in front of it.
// The total kernel reads out[0 .. n_columns), each written by one lane of the fold.  No block waits for another, there is no
// atomic operation of any kind, and two calls on the same input leave the same bytes.  Every load lies inside a row of its
// column: row < rows, slot < dim / V, V divides dim.  float64 sums of n non-negative terms: within n * 2^-53 of the exact sum,
// relative, in any order (so within n * 2^-52 of any other such summation, which is what the tests hold).
//
// No scratch; LDS only for the 4 wave records of a block's fold.  The default modes of the other units (denormals kept, IEEE).
// Contraction is off from here to the end of the file, as in fcp_table_audit.hip: every operation rounds once, by itself.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off)

#include "fcp_block_fold.h" // wave_fold, block_fold, kNoSuchRow: the fold of a lane's record into the block's, in one fixed order

static_assert(FCP_OUT_BF16 == FCP_TAB_BF16 && FCP_OUT_F16 == FCP_TAB_F16, "widen16 takes FCP_TAB_*: the output kinds carry the same numbers");
static_assert(sizeof(fcp_output_error_t) == 64, "fcp_output_error_t is 64 bytes");
static_assert((int64_t)INT32_MAX < fcpf::kRowLimit, "shapes are int32: rows stay below the row limit by their type");

namespace {

constexpr int kTargetBlocks = 4096; // what the grid aims at: 16 blocks of 256 threads for each of 256 CUs
constexpr int kMaxTiles = 64;       // T's upper end: a one-column call is 64 blocks

// tiles per column: a function of n_columns alone
int tiles_of(int32_t n) { return n <= 0 ? 1 : std::min(kMaxTiles, std::max(1, (kTargetBlocks + n - 1) / n)); }

// One column as the kernels see it.  48 bytes (a multiple of 16: the upload kernel moves 16-byte words).
struct CmpColumn {
  const char *a, *b;          // byte addresses of the column's first elements
  int64_t stride_a, stride_b; // row strides in elements
  int32_t rows, dim;
  int32_t vec;       // V: elements per lane and load, 4 | 2 | 1
  int32_t tile_rows; // R: rows of a row tile
};
static_assert(sizeof(CmpColumn) == 48, "the descriptor image is n_columns records of 48 bytes");

// What a lane, a wave and a block have seen of a column.  48 bytes, 8-byte aligned.
struct CmpPartial {
  double sum_sq_ref, sum_sq_err;
  int64_t differ, nonfinite;
  uint32_t first_differ; // kNoSuchRow: none
  float max_err, max_ref;
  uint32_t pad;
};
static_assert(sizeof(CmpPartial) == 48, "the workspace's records are 48 bytes");

// (the maxima as bit patterns of |x|)
struct LaneSums {
  double sum_sq_ref = 0.0, sum_sq_err = 0.0;
  uint64_t differ = 0, nonfinite = 0;
  uint32_t first_differ = kNoSuchRow, max_err = 0, max_ref = 0;
};

__device__ __forceinline__ void fold(CmpPartial &a, const CmpPartial &b) {
  a.sum_sq_ref += b.sum_sq_ref;
  a.sum_sq_err += b.sum_sq_err;
  a.differ += b.differ;
  a.nonfinite += b.nonfinite;
  a.first_differ = min(a.first_differ, b.first_differ);
  a.max_err = fmaxf(a.max_err, b.max_err);
  a.max_ref = fmaxf(a.max_ref, b.max_ref);
}

__device__ __forceinline__ CmpPartial nothing_seen() {
  CmpPartial p;
  p.sum_sq_ref = p.sum_sq_err = 0.0;
  p.differ = p.nonfinite = 0;
  p.first_differ = kNoSuchRow;
  p.max_err = p.max_ref = 0.0f;
  p.pad = 0;
  return p;
}

// V elements of kind K at byte address p (V elements aligned), widened exactly
template <int K, int V> __device__ __forceinline__ VF<V> ld_elems(const char *p) {
  if constexpr (K == FCP_OUT_F32) {
    typedef typename VecType<V>::T T;
    const T t = *as_global(reinterpret_cast<const T *>(p));
    VF<V> r;
    __builtin_memcpy(&r, &t, sizeof(T));
    return r;
  } else {
    typedef typename NarrowType<V>::T T;
    return widen16<V>(*as_global(reinterpret_cast<const T *>(p)), K);
  }
}

template <int V> __device__ __forceinline__ void judge(const VF<V> &a, const VF<V> &b, uint32_t row, LaneSums &s) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const uint32_t ua = __float_as_uint(a.v[i]), ub = __float_as_uint(b.v[i]);
    const bool differ = ua != ub;
    const bool finite = (ua & 0x7F800000u) != 0x7F800000u && (ub & 0x7F800000u) != 0x7F800000u;
    s.differ += differ ? 1 : 0;
    s.first_differ = differ ? min(s.first_differ, row) : s.first_differ;
    s.nonfinite += finite ? 0 : 1;
    const float x = finite ? a.v[i] : 0.0f;
    const float e = finite ? b.v[i] - a.v[i] : 0.0f; // (a non-finite pair: +0 into both sums and both maxima)
    s.sum_sq_ref = __builtin_fma((double)x, (double)x, s.sum_sq_ref);
    s.sum_sq_err = __builtin_fma((double)e, (double)e, s.sum_sq_err);
    s.max_ref = max(s.max_ref, __float_as_uint(x) & 0x7FFFFFFFu);
    s.max_err = max(s.max_err, __float_as_uint(e) & 0x7FFFFFFFu);
  }
}

// The row tiles tile, tile + T, ... of column c, two in flight.  ea, eb: bytes of an element.
template <int KA, int KB, int V>
__device__ __forceinline__ void walk(const CmpColumn &c, int tile, int T, LaneSums &s) {
  constexpr int ea = KA == FCP_OUT_F32 ? 4 : 2, eb = KB == FCP_OUT_F32 ? 4 : 2;
  const int tid = threadIdx.x;
  const int S = c.dim / V, R = c.tile_rows;
  // the lane's place in every row tile: row r_local, slots slot, slot + 256, ... (a row of more than 256 slots: R == 1);
  // lanes beyond the tile's R * S slots have none
  int r_local = 0, slot = tid;
  if (S <= FCP_BLOCK_THREADS) {
    r_local = tid / S;
    slot = r_local < R ? tid - r_local * S : S;
  }
  const int64_t rows = c.rows;
  const int64_t tiles = (rows + R - 1) / R;
  for (int64_t t0 = tile; t0 < tiles; t0 += 2 * (int64_t)T) {
    const int64_t row0 = t0 * R + r_local, row1 = (t0 + T) * R + r_local; // (t0 + T may lie beyond the tiles: row1 >= rows then)
    const bool live0 = row0 < rows, live1 = row1 < rows;
    const char *a0 = c.a + row0 * c.stride_a * ea, *b0 = c.b + row0 * c.stride_b * eb;
    const char *a1 = c.a + row1 * c.stride_a * ea, *b1 = c.b + row1 * c.stride_b * eb;
    for (int q = slot; q < S; q += FCP_BLOCK_THREADS) {
      VF<V> xa0, xb0, xa1, xb1;
      if (live0) {
        xa0 = ld_elems<KA, V>(a0 + (int64_t)q * (V * ea));
        xb0 = ld_elems<KB, V>(b0 + (int64_t)q * (V * eb));
      }
      if (live1) {
        xa1 = ld_elems<KA, V>(a1 + (int64_t)q * (V * ea));
        xb1 = ld_elems<KB, V>(b1 + (int64_t)q * (V * eb));
      }
      if (live0) judge<V>(xa0, xb0, (uint32_t)row0, s);
      if (live1) judge<V>(xa1, xb1, (uint32_t)row1, s);
    }
  }
}

// cols: the descriptor image in the workspace; partials: [n_columns * T] records behind it.  Block b = (column b / T, tile b % T).
template <int KA, int KB>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_outputs_compare_kernel(const CmpColumn *__restrict__ cols, int32_t T, CmpPartial *__restrict__ partials) {
  const int k = blockIdx.x / T, tile = blockIdx.x - k * T;
  const CmpColumn c = cols[k]; // block-uniform, read-only: scalar loads
  LaneSums s;
  if (c.vec == 4)
    walk<KA, KB, 4>(c, tile, T, s);
  else if (c.vec == 2)
    walk<KA, KB, 2>(c, tile, T, s);
  else
    walk<KA, KB, 1>(c, tile, T, s);

  CmpPartial p;
  p.sum_sq_ref = s.sum_sq_ref;
  p.sum_sq_err = s.sum_sq_err;
  p.differ = (int64_t)s.differ;
  p.nonfinite = (int64_t)s.nonfinite;
  p.first_differ = s.first_differ;
  p.max_err = __uint_as_float(s.max_err);
  p.max_ref = __uint_as_float(s.max_ref);
  p.pad = 0;
  block_fold(p, partials);
}

__device__ __forceinline__ void write_record(fcp_output_error_t *out, int64_t elems, const CmpPartial &p) {
  fcp_output_error_t r;
  r.elems = elems;
  r.differ = p.differ;
  r.nonfinite = p.nonfinite;
  r.first_differ_row = p.first_differ == kNoSuchRow ? -1 : (int64_t)p.first_differ;
  r.sum_sq_ref = p.sum_sq_ref;
  r.sum_sq_err = p.sum_sq_err;
  r.max_abs_err = p.max_err;
  r.max_abs_ref = p.max_ref;
  r.reserved = 0;
  *out = r;
}

// one lane per column: its T records in tile order
__global__ void __launch_bounds__(64) fcp_outputs_compare_fold_kernel(const CmpColumn *cols, const CmpPartial *partials, int32_t n, int32_t T,
                                                                      fcp_output_error_t *out) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n) return;
  CmpPartial p = nothing_seen();
  for (int t = 0; t < T; ++t) fold(p, partials[(int64_t)k * T + t]);
  write_record(out + k, (int64_t)cols[k].rows * cols[k].dim, p);
}

// one wave: out[0 .. n) into out[n]; n == 0: the zero record
__global__ void __launch_bounds__(64) fcp_outputs_compare_total_kernel(int32_t n, fcp_output_error_t *out) {
  const int lane = threadIdx.x;
  CmpPartial p = nothing_seen();
  int64_t elems = 0;
  for (int k = lane; k < n; k += 64) {
    const fcp_output_error_t r = out[k];
    CmpPartial o;
    o.sum_sq_ref = r.sum_sq_ref;
    o.sum_sq_err = r.sum_sq_err;
    o.differ = r.differ;
    o.nonfinite = r.nonfinite;
    o.first_differ = r.first_differ_row < 0 ? kNoSuchRow : (uint32_t)r.first_differ_row;
    o.max_err = r.max_abs_err;
    o.max_ref = r.max_abs_ref;
    fold(p, o);
    elems += r.elems;
  }
  wave_fold(p);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) elems += __shfl_xor(elems, m, 64);
  if (lane == 0) write_record(out + n, elems, p);
}

template <int KA> void launch_compare_b(int kb, dim3 grid, hipStream_t s, const CmpColumn *cols, int32_t T, CmpPartial *partials) {
  const dim3 block(FCP_BLOCK_THREADS);
  if (kb == FCP_OUT_F32)
    hipLaunchKernelGGL((fcp_outputs_compare_kernel<KA, FCP_OUT_F32>), grid, block, 0, s, cols, T, partials);
  else if (kb == FCP_OUT_BF16)
    hipLaunchKernelGGL((fcp_outputs_compare_kernel<KA, FCP_OUT_BF16>), grid, block, 0, s, cols, T, partials);
  else
    hipLaunchKernelGGL((fcp_outputs_compare_kernel<KA, FCP_OUT_F16>), grid, block, 0, s, cols, T, partials);
}
void launch_compare(int ka, int kb, dim3 grid, hipStream_t s, const CmpColumn *cols, int32_t T, CmpPartial *partials) {
  if (ka == FCP_OUT_F32)
    launch_compare_b<FCP_OUT_F32>(kb, grid, s, cols, T, partials);
  else if (ka == FCP_OUT_BF16)
    launch_compare_b<FCP_OUT_BF16>(kb, grid, s, cols, T, partials);
  else
    launch_compare_b<FCP_OUT_F16>(kb, grid, s, cols, T, partials);
}

int elem_bytes(int kind) { return kind == FCP_OUT_F32 ? 4 : 2; }
bool known_kind(int kind) { return kind == FCP_OUT_F32 || kind == FCP_OUT_BF16 || kind == FCP_OUT_F16; }

// Every refusal, in the order the header documents; nothing here touches a device or dereferences a column pointer.
int check_args(const void *const *ptrs_a, const int64_t *row_strides_a, int32_t out_kind_a, const void *const *ptrs_b,
               const int64_t *row_strides_b, int32_t out_kind_b, const int32_t *shapes, int32_t n_columns, const void *out,
               const void *workspace) {
  const std::string w = "fcp_outputs_compare: ";
  auto bad = [&](const std::string &msg) { return fail(FCP_ERR_INVALID_ARGUMENT, w + msg); };
  auto col = [](int32_t k) { return "column " + std::to_string(k) + ": "; };
  if (n_columns != 0) {
    if (!ptrs_a) return bad("`ptrs_a` is null");
    if (!row_strides_a) return bad("`row_strides_a` is null");
    if (!ptrs_b) return bad("`ptrs_b` is null");
    if (!row_strides_b) return bad("`row_strides_b` is null");
    if (!shapes) return bad("`shapes` is null");
  }
  if (!known_kind(out_kind_a)) return bad("`out_kind_a` " + std::to_string(out_kind_a) + " is no FCP_OUT_* kind");
  if (!known_kind(out_kind_b)) return bad("`out_kind_b` " + std::to_string(out_kind_b) + " is no FCP_OUT_* kind");
  if (n_columns < 0) return bad("`n_columns` is negative");
  for (int32_t k = 0; k < n_columns; ++k) {
    if (shapes[2 * k] < 0) return bad(col(k) + "`shapes` holds negative rows");
    if (shapes[2 * k + 1] <= 0) return bad(col(k) + "`shapes` holds a dim that is not positive");
  }
  for (int32_t k = 0; k < n_columns; ++k) {
    if (row_strides_a[k] < shapes[2 * k + 1]) return bad(col(k) + "`row_strides_a` is below dim");
    if (row_strides_b[k] < shapes[2 * k + 1]) return bad(col(k) + "`row_strides_b` is below dim");
  }
  for (int32_t k = 0; k < n_columns; ++k) {
    if (shapes[2 * k] > 0 && !ptrs_a[k]) return bad(col(k) + "`ptrs_a` holds a null pointer and the column has rows");
    if (shapes[2 * k] > 0 && !ptrs_b[k]) return bad(col(k) + "`ptrs_b` holds a null pointer and the column has rows");
  }
  const int ea = elem_bytes(out_kind_a), eb = elem_bytes(out_kind_b);
  for (int32_t k = 0; k < n_columns; ++k) {
    if ((uintptr_t)ptrs_a[k] % ea) return bad(col(k) + "`ptrs_a` is not aligned to its " + std::to_string(ea) + "-byte elements");
    if ((uintptr_t)ptrs_b[k] % eb) return bad(col(k) + "`ptrs_b` is not aligned to its " + std::to_string(eb) + "-byte elements");
  }
  if (!out) return bad("`out` is null");
  if (!workspace) return bad("`workspace` is null");
  if ((uintptr_t)out % 8) return bad("`out` is not 8-byte aligned");
  if ((uintptr_t)workspace % 8) return bad("`workspace` is not 8-byte aligned");
  // (rows at or above fcpf::kRowLimit: `shapes` is int32, so no value of it gets there — the static_assert above)
  return FCP_OK;
}

// the widest V every address of the column is aligned for, on both sides
int vec_of_column(const CmpColumn &c, int ea, int eb) {
  int v = 4;
  const uint64_t bits = (uint64_t)c.dim | (uint64_t)c.stride_a | (uint64_t)c.stride_b;
  while (v > 1 && ((bits & (uint64_t)(v - 1)) || (uintptr_t)c.a % (uintptr_t)(v * ea) || (uintptr_t)c.b % (uintptr_t)(v * eb))) v >>= 1;
  return v;
}

} // namespace

extern "C" int64_t fcp_outputs_compare_workspace_bytes(int32_t n_columns) {
  if (n_columns < 0) return -1;
  // 16 bytes to bring the descriptor image to a 16-byte boundary, the image, and n_columns * T partial records: T <
  // 4096 / n + 1 and T <= 64, so min(64 n, 4096 + n) records hold them — non-decreasing in n, which n * T is not
  const int64_t n = n_columns;
  return 16 + n * (int64_t)sizeof(CmpColumn) + std::min<int64_t>(kMaxTiles * n, kTargetBlocks + n) * (int64_t)sizeof(CmpPartial);
}

extern "C" int fcp_outputs_compare(const void *const *ptrs_a, const int64_t *row_strides_a, int32_t out_kind_a, const void *const *ptrs_b,
                                   const int64_t *row_strides_b, int32_t out_kind_b, const int32_t *shapes, int32_t n_columns,
                                   fcp_output_error_t *out, void *workspace, int32_t device, void *stream_) {
  int rc = check_args(ptrs_a, row_strides_a, out_kind_a, ptrs_b, row_strides_b, out_kind_b, shapes, n_columns, out, workspace);
  if (rc) return rc;
  DeviceGuard guard;
  if ((rc = guard.enter(device))) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (n_columns == 0) {
    hipLaunchKernelGGL(fcp_outputs_compare_total_kernel, dim3(1), dim3(64), 0, stream, 0, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FCP_OK : hip_fail("fcp_outputs_compare: kernel launch", e);
  }
  if (stream_is_capturing(stream))
    return fail(FCP_ERR_UNSUPPORTED, "fcp_outputs_compare: stream capture of a call with columns: their descriptors are installed "
                                     "from the host by every call, which a replay would not repeat");
  // either side may be the result of a private-stream request: read behind it
  if ((rc = wait_for_inputs(ptrs_a, n_columns, stream_))) return rc;
  if ((rc = wait_for_inputs(ptrs_b, n_columns, stream_))) return rc;

  const int T = tiles_of(n_columns);
  const size_t image_bytes = (size_t)n_columns * sizeof(CmpColumn);
  // the descriptor image goes through a slot of this entry's pinned ring, filled in place (upload_image, fcp_host.h; the capture
  // was refused above, in front of the waits)
  static StageRings rings;
  const int ea = elem_bytes(out_kind_a), eb = elem_bytes(out_kind_b);
  char *d_image;
  rc = upload_image("fcp_outputs_compare", rings, device, stream, workspace, image_bytes, nullptr, [&](char *buf) {
    CmpColumn *h = reinterpret_cast<CmpColumn *>(buf);
    for (int32_t k = 0; k < n_columns; ++k) {
      CmpColumn c;
      c.a = static_cast<const char *>(ptrs_a[k]);
      c.b = static_cast<const char *>(ptrs_b[k]);
      c.stride_a = row_strides_a[k];
      c.stride_b = row_strides_b[k];
      c.rows = shapes[2 * k];
      c.dim = shapes[2 * k + 1];
      c.vec = vec_of_column(c, ea, eb);
      const int slots = c.dim / c.vec;
      c.tile_rows = slots <= FCP_BLOCK_THREADS ? FCP_BLOCK_THREADS / slots : 1;
      h[k] = c;
    }
  }, &d_image);
  if (rc) return rc;
  CmpColumn *d_cols = reinterpret_cast<CmpColumn *>(d_image);
  CmpPartial *d_partials = reinterpret_cast<CmpPartial *>(d_image + image_bytes);
  launch_compare(out_kind_a, out_kind_b, dim3((unsigned)((int64_t)n_columns * T)), stream, d_cols, (int32_t)T, d_partials);
  hipLaunchKernelGGL(fcp_outputs_compare_fold_kernel, dim3((unsigned)((n_columns + 63) / 64)), dim3(64), 0, stream, d_cols, d_partials,
                     n_columns, (int32_t)T, out);
  hipLaunchKernelGGL(fcp_outputs_compare_total_kernel, dim3(1), dim3(64), 0, stream, n_columns, out);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? FCP_OK : hip_fail("fcp_outputs_compare: kernel launch", le);
}
