// fcp_table_traffic.hip — fcp_table_count_ids: how often requests read each row of a table, counted on the device from the
// ids themselves (int64 or int32, as a plan's request delivers them) into a uint32 array of one cell per row.  The counts are
// what fcp_table_audit_weighted (fcp_table_audit.hip) weighs a table's errors by.  The reference has no counterpart.
//
//   fcp_table_count_ids_kernel<IdT>   a fixed grid (kCountBlocks, fewer when the ids do not fill it) of kCountThreads threads; a
//                     block takes tiles of kTileIds consecutive ids with a 64-bit grid-stride loop, a thread kIdsPerThread ids
//                     of a tile, kCountThreads apart (every load of a wave is one contiguous run).  An id is widened to 64 bits (int32:
//                     sign-extended) and compared unsigned against table_rows — the plans' rule, fcp_table_update_rows' rule:
//                     an id outside touches no memory and is counted, per wave by ballot and popcount in a wave-uniform
//                     register, per block through one LDS cell, with ONE 64-bit atomic per block at the end.
//                     One global atomic per id is the floor for ids spread over a large table and a cliff for the head of a
//                     Zipf distribution (adders on one address serialise at the memory side).  So a block first counts in
//                     LDS: the row table of fcp_block_fold.h, kCountSlots {row, count} cells, a claimed cell bumped by an LDS
//                     add.  A row that finds no cell within the probes goes straight to a global atomicAdd.  After its
//                     last tile the block flushes: one global atomicAdd per occupied cell.  Every id thus reaches counts[] exactly once, alone or inside a cell's count; unsigned
//                     adds modulo 2^32 commute, in LDS as in memory, so the result is exact and independent of any order,
//                     of the grid and of concurrent calls into the same array.
//                     The table is as large as LDS allows — one block of 16 waves per CU, 128 KiB of cells — because what it
//                     cannot hold costs a global atomic per read: rows of the warm middle of a Zipf distribution that find
//                     their cells taken by cold rows.  profiles/table_traffic.txt has the sizes that were measured.
//   fcp_plan_traffic_kernel<SLOTS>   fcp_plan_traffic_count: the rows ONE REQUEST of a plan reads, counted through the plan's own
//                     id path.  A 2-D grid: blockIdx.x names an entry of the plan's list of counted lookup columns
//                     (FcpTrafficCol: the column's position and its table's counts), blockIdx.y a tile of kTrafficTile
//                     positions of that column's id stream (a stride loop over tiles where the stream has more than the
//                     grid's y extent covers).  The block reads its column's static and dynamic records straight into
//                     wave-uniform registers — one column per block: no span machinery, no LDS copy — and leaves at once,
//                     before it touches LDS, when its first tile lies past the column's nnz (the grid's y extent is sized
//                     by the longest stream).  Every position i < nnz goes through fetch_slot_offset<1, false> with
//                     world = 1 — the id decoded from int32 / int64 / Bucketize(float32) (boundaries from global memory),
//                     hashed, passed through SELECT / FILTER, compared against the column's vocab — exactly as the fused
//                     bodies call it: a row adds 1 to counts[row], kFiltered adds nothing, kBadRow touches no memory and
//                     is counted per wave by ballot and popcount, one 64-bit atomic per wave that saw any.  The plan's own
//                     bad-id counter is never passed.
//                     The block's reads go through count_row's LDS table first (a block serves one column, hence one
//                     table: the same {row, count} cells, SLOTS of them) and are flushed at the end.  (One global atomic
//                     per counted id, no LDS, a build of the commit that introduced the kernel: the figures behind the
//                     choice are in DESIGN.md 3 and profiles/plan_traffic.txt.)
// Every atomic's result is unused except the compare-and-swap's: the global ones are the no-return vector forms
// (global_atomic_add / global_atomic_add_x2), nothing scalar.  No scratch; LDS: the two arrays and the skipped cell
// (fcp_table_count_ids: 128 KiB + 8 bytes — a CU holds one block, and the block waits for a CU whose LDS other kernels have
// left; fcp_plan_traffic_kernel: its two arrays, 16 KiB).
#include "fcp_fused_bodies.h"
#include "fcp_host.h"
#include "fcp_block_fold.h" // the block's LDS row table: lds_rows_clear / _claim / _flush

namespace {

constexpr int kCountThreads = 1024;         // 16 waves: one block fills a CU's LDS, so it brings the CU's waves itself
constexpr int kCountBlocks = 256;           // the fixed grid: one block on each of 256 CUs
constexpr int kIdsPerThread = 4;
constexpr int kTileIds = kCountThreads * kIdsPerThread; // ids of one step of a block's stride loop
constexpr int kCountSlots = 16384;          // cells of a block's LDS table (128 KiB of the CU's 160); a power of two

// one read of row r: into the block's cell for r, or — no cell within the probes — into counts[r] itself
template <int SLOTS> __device__ __forceinline__ void count_row(uint32_t *counts, uint32_t *s_key, uint32_t *s_cnt, uint32_t r) {
  const int slot = lds_rows_claim<SLOTS>((LdsU32 *)s_key, r);
  if (slot >= 0)
    (void)__hip_atomic_fetch_add((LdsU32 *)s_cnt + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    (void)__hip_atomic_fetch_add(as_global(counts + r), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ids: the call's n ids.  Every thread of a block takes the same number of steps, so whole waves reach the ballots.
template <typename IdT>
__global__ void __launch_bounds__(kCountThreads)
    fcp_table_count_ids_kernel(uint32_t *counts, uint64_t table_rows, const IdT *ids, int64_t n, unsigned long long *skipped) {
  __shared__ uint32_t s_key[kCountSlots];
  __shared__ uint32_t s_cnt[kCountSlots];
  __shared__ unsigned long long s_skipped;
  const int tid = threadIdx.x;
  if (tid == 0) s_skipped = 0;
  lds_rows_clear<kCountSlots, kCountThreads>(s_key, s_cnt, tid);

  unsigned long long outside = 0; // of this wave: the same value in every lane
  for (int64_t base = (int64_t)blockIdx.x * kTileIds; base < n; base += (int64_t)gridDim.x * kTileIds) {
    uint64_t id[kIdsPerThread];
    bool have[kIdsPerThread];
#pragma unroll
    for (int k = 0; k < kIdsPerThread; ++k) {
      const int64_t i = base + k * kCountThreads + tid;
      have[k] = i < n;
      id[k] = have[k] ? (uint64_t)(int64_t)ids[i] : 0;
    }
#pragma unroll
    for (int k = 0; k < kIdsPerThread; ++k) {
      const bool live = have[k] && id[k] < table_rows;
      outside += (unsigned long long)__popcll(__ballot(have[k] && !live));
      if (live) count_row<kCountSlots>(counts, s_key, s_cnt, (uint32_t)id[k]);
    }
  }
  if ((tid & 63) == 0 && outside != 0) atomicAdd(&s_skipped, outside);
  lds_rows_flush<kCountSlots, kCountThreads>(s_key, s_cnt, tid, [&](uint32_t r, uint32_t c) { atomicAdd(counts + r, c); });
  if (tid == 0 && skipped && s_skipped != 0) atomicAdd(skipped, s_skipped);
}


// ---- one request of a plan ---------------------------------------------------------------------------------------------------
constexpr int kTrafficThreads = 256;
constexpr int kTrafficIdsPerThread = 4;
constexpr int kTrafficTile = kTrafficThreads * kTrafficIdsPerThread; // positions of an id stream per block and step
constexpr int kTrafficMaxTilesY = 65535;                             // the grid's y extent; longer streams: the stride loop
constexpr int kTrafficSlots = 2048;                                  // cells of a block's table: 2 x 8 KiB of LDS for a tile of 1024 ids

template <int SLOTS>
__global__ void __launch_bounds__(kTrafficThreads) fcp_plan_traffic_kernel(FcpTrafficLaunch T) {
  __shared__ uint32_t s_key[SLOTS];
  __shared__ uint32_t s_cnt[SLOTS];
  const FcpTrafficCol tc = ld_rec(as_const(T.list) + blockIdx.x);
  const FcpColDyn d = ld_rec(as_const(T.dyn) + tc.pos);
  const int nnz = d.nnz;
  if ((int64_t)blockIdx.y * kTrafficTile >= nnz) return; // (uniform: the whole block, before it touches LDS)
  LdsCol c; // in registers, wave-uniform: what stage_col would put in LDS, less what the id path does not read
  static_cast<FcpColStatic &>(c) = ld_rec(as_const(T.cols) + tc.pos);
  c.ids = T.blob + d.ids_off;
  c.csr = nullptr;
  c.out_base = 0;
  c.out_stride = 0;
  c.nnz = nnz;
  const FcpXform *xf = T.xforms + tc.pos; // (only dereferenced by a column with a transform: then the array exists)
  uint32_t *counts = tc.counts;
  const int tid = threadIdx.x;
  lds_rows_clear<SLOTS, kTrafficThreads>(s_key, s_cnt, tid);

  unsigned long long outside = 0; // of this wave: the same value in every lane
  for (int64_t base = (int64_t)blockIdx.y * kTrafficTile; base < nnz; base += (int64_t)gridDim.y * kTrafficTile) {
#pragma unroll
    for (int k = 0; k < kTrafficIdsPerThread; ++k) {
      const int64_t i = base + k * kTrafficThreads + tid;
      bool bad = false;
      uint32_t row = kFiltered;
      if (i < nnz) row = fetch_slot_offset<1, false>(c, xf, i, nullptr, 0, 1, bad);
      outside += (unsigned long long)__popcll(__ballot(row == kBadRow));
      if (is_row(row)) count_row<SLOTS>(counts, s_key, s_cnt, row);
    }
  }
  if ((tid & 63) == 0 && outside != 0 && T.skipped)
    (void)__hip_atomic_fetch_add(as_global(T.skipped), outside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  lds_rows_flush<SLOTS, kTrafficThreads>(s_key, s_cnt, tid, [&](uint32_t r, uint32_t n) {
    (void)__hip_atomic_fetch_add(as_global(counts + r), n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
}

} // namespace

int fcp_launch_plan_traffic(const FcpTrafficLaunch &T, int n_list, int max_nnz, ihipStream_t *s) {
  if (n_list <= 0 || max_nnz <= 0) return 0;
  const int tiles = (int)std::min<int64_t>(((int64_t)max_nnz + kTrafficTile - 1) / kTrafficTile, kTrafficMaxTilesY);
  const dim3 grid((unsigned)n_list, (unsigned)tiles);
  hipLaunchKernelGGL(fcp_plan_traffic_kernel<kTrafficSlots>, grid, dim3(kTrafficThreads), 0, s, T);
  return (int)hipGetLastError();
}

extern "C" int fcp_table_count_ids(uint32_t *counts, int64_t table_rows, const void *ids, int32_t id_bytes, int64_t n, int64_t *skipped,
                                   int32_t device, void *stream) {
  const std::string w = "fcp_table_count_ids: ";
  if (n < 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`n` is negative");
  if (table_rows < 1 || table_rows >= fcpf::kRowLimit)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`table_rows` must lie in [1, 2^32 - 3), a plan's row limit");
  if (id_bytes != 4 && id_bytes != 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`id_bytes` is 4 (int32 ids) or 8 (int64 ids)");
  if (n > 0 && !counts) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`counts` is null");
  if (n > 0 && !ids) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`ids` is null");
  if ((uintptr_t)counts % 4) return fail(FCP_ERR_INVALID_ARGUMENT, w + fcpf::not_aligned("counts", 4));
  if ((uintptr_t)ids % (uintptr_t)id_bytes) return fail(FCP_ERR_INVALID_ARGUMENT, w + fcpf::not_aligned("ids", id_bytes));
  if ((uintptr_t)skipped % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + fcpf::not_aligned("skipped", 8));
  if (n == 0) return FCP_OK;
  unsigned long long *sk = reinterpret_cast<unsigned long long *>(skipped);
  const int blocks = (int)std::min<int64_t>(kCountBlocks, n / kTileIds + (n % kTileIds != 0));
  return on_device("fcp_table_count_ids", device, stream, [&](hipStream_t s) {
    if (id_bytes == 8)
      hipLaunchKernelGGL(fcp_table_count_ids_kernel<int64_t>, dim3(blocks), dim3(kCountThreads), 0, s, counts, (uint64_t)table_rows,
                         static_cast<const int64_t *>(ids), n, sk);
    else
      hipLaunchKernelGGL(fcp_table_count_ids_kernel<int32_t>, dim3(blocks), dim3(kCountThreads), 0, s, counts, (uint64_t)table_rows,
                         static_cast<const int32_t *>(ids), n, sk);
  });
}
