// fcp_table_rows_bodies.h — the bodies of the rows-by-id kernels, written ONCE for the two units that launch them:
// fcp_table_rows.hip (one table per call: the block index is blockIdx.x) and fcp_tables_rows.hip (many tables per call: the
// block index is local to the entry the block found).  `block` is the only thing the two fronts hand over differently; every
// other argument is what the single-table kernels took.  The includer switches contraction off and includes fcp_table_walk.h
// in front (quantize_row rounds every operation once).  Unnamed namespace, as in fcp_table_walk.h.
#pragma once
#include "fcp_table_walk.h"

namespace {

// One vector atomicAdd per wave at most: `mine` is set in the one lane that speaks for a skipped row.  Every lane of the wave
// gets here (no lane has returned yet), so the wave's first lane is there to issue it.  The add is atomicAdd's — relaxed, device
// scope — on a pointer cast to the global address space: a counter that arrives in an entry's record instead of as a kernel
// argument would otherwise be a flat access.
__device__ __forceinline__ void count_skipped(unsigned long long *skipped, bool mine) {
  if (!skipped) return;
  const unsigned long long m = __ballot(mine);
  if (m != 0 && (threadIdx.x & 63) == 0)
    __hip_atomic_fetch_add(as_global(skipped), (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// table: the table's base; ids / src: the first row of this launch; rows: of this launch (< 2^30).  Block = 256 / G rows; a
// group never straddles a wave, and it is live or not as a whole.
template <int V, int G>
__device__ __forceinline__ void update_q8_body(char *table, const int64_t *ids, const float *src, int32_t rows, int32_t dim,
                                               uint64_t table_rows, unsigned long long *skipped, uint32_t block) {
  const int tid = threadIdx.x;
  const int lane = tid & (G - 1);
  const int64_t row = (int64_t)block * (FCP_BLOCK_THREADS / G) + tid / G;
  const bool have = row < rows;
  const uint64_t id = have ? (uint64_t)*as_global(ids + row) : ~0ull; // the whole group: one address
  const bool live = have && id < table_rows;
  count_skipped(skipped, have && !live && lane == 0);
  quantize_row<V, G>(table + (live ? id : 0) * ((uint64_t)dim + 8), src + row * dim, dim, lane, live);
}

// n: slots of this launch (<= 2^30, one row of more: < 2^31); ids / src: the first row of this launch; spr: slots per row,
// dim / V; kind: FCP_TAB_F32 | _BF16 | _F16, the same for every wave
template <int V>
__device__ __forceinline__ void update_rows_body(char *table, const int64_t *ids, const float *src, uint32_t n, uint32_t spr, int32_t dim,
                                                 int32_t kind, uint64_t table_rows, unsigned long long *skipped, uint32_t block) {
  const uint32_t i = block * FCP_BLOCK_THREADS + threadIdx.x;
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
__device__ __forceinline__ void read_rows_body(float *dst, const char *table, const int64_t *ids, uint32_t n, uint32_t spr, int32_t dim,
                                               int32_t kind, uint64_t table_rows, uint32_t block) {
  const uint32_t i = block * FCP_BLOCK_THREADS + threadIdx.x;
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

} // namespace
