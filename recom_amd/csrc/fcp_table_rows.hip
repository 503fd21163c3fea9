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
#include "fcp_table_rows_bodies.h" // the three bodies and count_skipped: one text with fcp_tables_rows.hip
#include "fcp_tables_rows_plan.h"  // fcpr::check_row_args: the argument checks, shared with the grouped entries

static_assert(FCP_TAB_BF16 == FCP_OUT_BF16 && FCP_TAB_F16 == FCP_OUT_F16, "st_out_narrow takes the table kind as its output kind");

namespace {

// The bodies are those of fcp_table_rows_bodies.h with the block index of the launch.
template <int V, int G>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_update_q8_kernel(char *table, const int64_t *ids, const float *src, int32_t rows, int32_t dim, uint64_t table_rows,
                         unsigned long long *skipped) {
  update_q8_body<V, G>(table, ids, src, rows, dim, table_rows, skipped, blockIdx.x);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_update_rows_kernel(char *table, const int64_t *ids, const float *src, uint32_t n, uint32_t spr, int32_t dim, int32_t kind,
                           uint64_t table_rows, unsigned long long *skipped) {
  update_rows_body<V>(table, ids, src, n, spr, dim, kind, table_rows, skipped, blockIdx.x);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_read_rows_kernel(float *dst, const char *table, const int64_t *ids, uint32_t n, uint32_t spr, int32_t dim, int32_t kind,
                         uint64_t table_rows) {
  read_rows_body<V>(dst, table, ids, n, spr, dim, kind, table_rows, blockIdx.x);
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

// The argument checks both entries share, in the stated order (fcpr::check_row_args, fcp_tables_rows_plan.cc: the grouped
// entries run the same text per entry); `who` is the entry's name.
int check_args(const char *who, const void *table, int32_t kind, int64_t table_rows, int32_t dim, const void *row_ids, const void *rows,
               int64_t n, const void *skipped) {
  std::string why;
  const int rc = fcpr::check_row_args(std::string(who) + ": ", table, kind, table_rows, dim, row_ids, rows, n, &why);
  if (rc) return fail(rc, why);
  if ((uintptr_t)skipped % 8) return fail(FCP_ERR_INVALID_ARGUMENT, std::string(who) + ": `skipped` is not 8-byte aligned");
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
