// fcp_table_rows.hip — fcp_table_update_rows / fcp_table_read_rows: rows of a table in any of the formats the plans read
// (FCP_TAB_F32 / _BF16 / _F16 / _Q8), written from float32 rows and read back as float32 rows BY ID, on the device.  The day
// after the load: a trainer ships (row ids, float32 rows) deltas, and fcp_table_convert (fcp_convert.hip) writes contiguous runs
// only.  The reference reads float32 tables only and has no counterpart.
//
//   update -> q8      fcp_update_q8_kernel<V, G>: the row quantiser fcp_quantize_q8_kernel<V, G> calls, quantize_row<V, G> of
//                     fcp_table_walk.h — the one text, so the same 3 V x 7 G matrix, group of G lanes per row, register cap,
//                     butterflies, divisions and rounding — with the destination row taken from the row's id instead of its
//                     index.  Every lane of a group loads the same id (one address).  A group is live when its
//                     row exists and (uint64_t)id < table_rows; lanes of dead groups take part in the exchanges and touch no
//                     memory.  Codes leave V bytes at a time, scale and bias as one pair (Q8Pair<V>) from the group's first lane:
//                     id * (dim + 8) keeps the alignment dst_row0 * (dim + 8) has in fcp_convert.hip, a multiple of V.
//   update -> 16 / float32   fcp_update_rows_kernel<V>: streaming, one V-element slot per lane, thread -> (row, slot) as
//                     fcp_dequantize_q8_kernel; st_out_narrow<V> (fl16, rounded once) or a float32 slot store.
//   read <- any kind  fcp_read_rows_kernel<V>: the same mapping; ld_q8<V> (one v_fma_f32 per element), widen16<V> (exact) or a
//                     float32 slot load; a row of +0.0 for an id outside the table, the plans' rule.
// The element type of the two streaming kernels is a kernel argument (wave-uniform branch), as tab_kind is in the fused
// kernels.  Ids are whole 64-bit values, compared unsigned against table_rows: a negative id is outside.  Skipped rows are
// counted with at most one atomicAdd per wave (a ballot of the lanes that hold a skipped row's first slot).
// The host chunks every call into launches of at most 2^30 threads, so an in-launch index fits 32 bits; byte offsets are
// formed in 64 bits.
//
// No scratch, no LDS; the default modes of the other units (denormals kept, IEEE).  Contraction is off from here to the end of
// the file: every operation of the quantiser rounds once, by itself.  The divisions are the correctly rounded ones.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off)

#include "fcp_table_walk.h" // (behind the pragma: its code rounds every operation once, too)

static_assert(FCP_TAB_BF16 == FCP_OUT_BF16 && FCP_TAB_F16 == FCP_OUT_F16, "st_out_narrow takes the table kind as its output kind");

namespace {

// One vector atomicAdd per wave at most: `mine` is set in the one lane that speaks for a skipped row.  Every lane of the wave
// gets here (no lane has returned yet), so the wave's first lane is there to issue it.
__device__ __forceinline__ void count_skipped(unsigned long long *skipped, bool mine) {
  if (!skipped) return;
  const unsigned long long m = __ballot(mine);
  if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(skipped, (unsigned long long)__popcll(m));
}

// table: the table's base; ids / src: the first row of this launch; rows: of this launch (< 2^30).  Block = 256 / G rows; a
// group never straddles a wave, and it is live or not as a whole.
template <int V, int G>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_update_q8_kernel(char *table, const int64_t *ids, const float *src, int32_t rows, int32_t dim, uint64_t table_rows,
                         unsigned long long *skipped) {
  const int tid = threadIdx.x;
  const int lane = tid & (G - 1);
  const int64_t row = (int64_t)blockIdx.x * (FCP_BLOCK_THREADS / G) + tid / G;
  const bool have = row < rows;
  const uint64_t id = have ? (uint64_t)*as_global(ids + row) : ~0ull; // the whole group: one address
  const bool live = have && id < table_rows;
  count_skipped(skipped, have && !live && lane == 0);
  quantize_row<V, G>(table + (live ? id : 0) * ((uint64_t)dim + 8), src + row * dim, dim, lane, live);
}

// n: slots of this launch (<= 2^30, one row of more: < 2^31); ids / src: the first row of this launch; spr: slots per row,
// dim / V; kind: FCP_TAB_F32 | _BF16 | _F16, the same for every wave
template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_update_rows_kernel(char *table, const int64_t *ids, const float *src, uint32_t n, uint32_t spr, int32_t dim, int32_t kind,
                           uint64_t table_rows, unsigned long long *skipped) {
  const uint32_t i = blockIdx.x * FCP_BLOCK_THREADS + threadIdx.x;
  const bool have = i < n;
  const uint32_t r = have ? i / spr : 0;
  const uint32_t e = (i - r * spr) * V;
  const uint64_t id = have ? (uint64_t)*as_global(ids + r) : ~0ull;
  const bool live = have && id < table_rows;
  count_skipped(skipped, have && !live && e == 0);
  if (!live) return;
  const VF<V> x = ld_f32<V>(src + (uint64_t)i * V);
  if (kind == FCP_TAB_F32)
    st_f32<V>(reinterpret_cast<float *>(table) + (id * (uint64_t)dim + e), x);
  else
    st_out_narrow<V>(table + 2 * (id * (uint64_t)dim + e), x, FCP_ST_PLAIN, kind);
}

// dst / ids: the first row of this launch; kind: any FCP_TAB_* value, the same for every wave
template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_read_rows_kernel(float *dst, const char *table, const int64_t *ids, uint32_t n, uint32_t spr, int32_t dim, int32_t kind,
                         uint64_t table_rows) {
  const uint32_t i = blockIdx.x * FCP_BLOCK_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = i / spr;
  const uint32_t e = (i - r * spr) * V;
  const uint64_t id = (uint64_t)*as_global(ids + r);
  VF<V> x = vzero<V>();
  if (id < table_rows) {
    if (kind == FCP_TAB_F32) {
      x = ld_f32<V>(reinterpret_cast<const float *>(table) + (id * (uint64_t)dim + e));
    } else if (kind == FCP_TAB_Q8) {
      const char *row = table + id * ((uint64_t)dim + 8);
      x = ld_q8<V>(row + e, row + dim);
    } else {
      typedef typename NarrowType<V>::T T;
      const T t = *as_global(reinterpret_cast<const T *>(table + 2 * (id * (uint64_t)dim + e)));
      x = widen16<V>(t, kind);
    }
  }
  st_f32<V>(dst + (uint64_t)i * V, x);
}

// G: 1 for dims <= 4, else the power of two that holds the row's slots, at most 64 (group_of)
template <int V>
void update_q8(char *table, const int64_t *ids, const float *src, int64_t n, int dim, uint64_t table_rows, unsigned long long *skipped,
               hipStream_t s) {
  with_group(group_of(dim, V), [&](auto g) {
    constexpr int G = decltype(g)::value;
    const int64_t per_launch = kMaxLaunchThreads / G;
    for (int64_t r0 = 0; r0 < n; r0 += per_launch) {
      const int64_t rows = std::min(n - r0, per_launch);
      hipLaunchKernelGGL((fcp_update_q8_kernel<V, G>), blocks_for(rows * G), dim3(FCP_BLOCK_THREADS), 0, s, table, ids + r0,
                         src + r0 * dim, (int32_t)rows, (int32_t)dim, table_rows, skipped);
    }
  });
}

template <int V>
void update(void *table, int kind, const int64_t *ids, const float *src, int64_t n, int dim, uint64_t table_rows,
            unsigned long long *skipped, hipStream_t s) {
  if (kind == FCP_TAB_Q8) return update_q8<V>(static_cast<char *>(table), ids, src, n, dim, table_rows, skipped, s);
  const int64_t spr = dim / V;
  const int64_t per_launch = std::max<int64_t>(1, kMaxLaunchThreads / spr); // (one row of 2^31 - 1 elements: 2^31 threads)
  for (int64_t r0 = 0; r0 < n; r0 += per_launch) {
    const int64_t slots = std::min(n - r0, per_launch) * spr;
    hipLaunchKernelGGL(fcp_update_rows_kernel<V>, blocks_for(slots), dim3(FCP_BLOCK_THREADS), 0, s, static_cast<char *>(table),
                       ids + r0, src + r0 * dim, (uint32_t)slots, (uint32_t)spr, (int32_t)dim, (int32_t)kind, table_rows, skipped);
  }
}

template <int V>
void read(float *dst, const void *table, int kind, const int64_t *ids, int64_t n, int dim, uint64_t table_rows, hipStream_t s) {
  const int64_t spr = dim / V;
  const int64_t per_launch = std::max<int64_t>(1, kMaxLaunchThreads / spr);
  for (int64_t r0 = 0; r0 < n; r0 += per_launch) {
    const int64_t slots = std::min(n - r0, per_launch) * spr;
    hipLaunchKernelGGL(fcp_read_rows_kernel<V>, blocks_for(slots), dim3(FCP_BLOCK_THREADS), 0, s, dst + r0 * dim,
                       static_cast<const char *>(table), ids + r0, (uint32_t)slots, (uint32_t)spr, (int32_t)dim, (int32_t)kind,
                       table_rows);
  }
}

// The argument checks both entries share, in the stated order; `who` is the entry's name.  The argument is named between
// backquotes: `rows` is also part of two other arguments' names.
int check_args(const char *who, const void *table, int32_t kind, int64_t table_rows, int32_t dim, const void *row_ids, const void *rows,
               int64_t n, const void *skipped) {
  const std::string w = std::string(who) + ": ";
  if (n < 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`n` is negative");
  if (n >= fcpf::kRowLimit) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`n` must stay below 2^32 - 3");
  if (table_rows < 1 || table_rows >= fcpf::kRowLimit)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`table_rows` must lie in [1, 2^32 - 3), a plan's row limit");
  if (dim <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`dim` must be positive");
  if (!fcpf::known_tab_kind(kind)) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`kind` is no FCP_TAB_* value");
  if (n > 0 && !table) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`table` is null");
  if (n > 0 && !row_ids) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`row_ids` is null");
  if (n > 0 && !rows) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`rows` is null");
  const int vec = vec_of(dim);
  if ((uintptr_t)table % fcpf::base_alignment(kind, vec))
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`table` is not " + std::to_string(fcpf::base_alignment(kind, vec)) + "-byte aligned (a " +
                                              kind_name(kind) + " table of this dim)");
  if ((uintptr_t)rows % (4 * vec))
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`rows` is not " + std::to_string(4 * vec) + "-byte aligned (float32 rows of this dim)");
  if ((uintptr_t)row_ids % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`row_ids` is not 8-byte aligned");
  if ((uintptr_t)skipped % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`skipped` is not 8-byte aligned");
  return FCP_OK;
}

} // namespace

extern "C" int fcp_table_update_rows(void *table, int32_t kind, int64_t table_rows, int32_t dim, const int64_t *row_ids,
                                     const float *rows, int64_t n, int64_t *skipped, int32_t device, void *stream) {
  int rc = check_args("fcp_table_update_rows", table, kind, table_rows, dim, row_ids, rows, n, skipped);
  if (rc) return rc;
  if (n == 0) return FCP_OK;
  unsigned long long *sk = reinterpret_cast<unsigned long long *>(skipped);
  return on_device("fcp_table_update_rows", device, stream, [&](hipStream_t s) {
    with_vec(vec_of(dim), [&](auto v) { update<decltype(v)::value>(table, kind, row_ids, rows, n, dim, (uint64_t)table_rows, sk, s); });
  });
}

extern "C" int fcp_table_read_rows(float *rows, const void *table, int32_t kind, int64_t table_rows, int32_t dim,
                                   const int64_t *row_ids, int64_t n, int32_t device, void *stream) {
  int rc = check_args("fcp_table_read_rows", table, kind, table_rows, dim, row_ids, rows, n, nullptr);
  if (rc) return rc;
  if (n == 0) return FCP_OK;
  return on_device("fcp_table_read_rows", device, stream, [&](hipStream_t s) {
    with_vec(vec_of(dim), [&](auto v) { read<decltype(v)::value>(rows, table, kind, row_ids, n, dim, (uint64_t)table_rows, s); });
  });
}
