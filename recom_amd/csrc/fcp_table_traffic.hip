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
//                     LDS: an open-addressed table of kCountSlots {row, count} cells, home slot row mod kCountSlots, linear
//                     probing over at most kCountProbes cells.  A cell is claimed by an LDS compare-and-swap on its key (the
//                     key of a claimed cell never changes while the block runs, so a key that is read as another row's is
//                     another row's for good) and bumped by an LDS add.  A row that finds no cell within the probes goes
//                     straight to a global atomicAdd.  After its last tile the block flushes: one global atomicAdd per
//                     occupied cell.  Every id thus reaches counts[] exactly once, alone or inside a cell's count; unsigned
//                     adds modulo 2^32 commute, in LDS as in memory, so the result is exact and independent of any order,
//                     of the grid and of concurrent calls into the same array.
//                     The table is as large as LDS allows — one block of 16 waves per CU, 128 KiB of cells — because what it
//                     cannot hold costs a global atomic per read: rows of the warm middle of a Zipf distribution that find
//                     their cells taken by cold rows.  profiles/table_traffic.txt has the sizes that were measured.
// Every atomic's result is unused except the compare-and-swap's: the global ones are the no-return vector forms
// (global_atomic_add / global_atomic_add_x2), nothing scalar.  No scratch; LDS: the two arrays and the skipped cell
// (128 KiB + 8 bytes: a CU holds one block, and the block waits for a CU whose LDS other kernels have left).
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

namespace {

constexpr int kCountThreads = 1024;         // 16 waves: one block fills a CU's LDS, so it brings the CU's waves itself
constexpr int kCountBlocks = 256;           // the fixed grid: one block on each of 256 CUs
constexpr int kIdsPerThread = 4;
constexpr int kTileIds = kCountThreads * kIdsPerThread; // ids of one step of a block's stride loop
constexpr int kCountSlots = 16384;          // cells of a block's LDS table (128 KiB of the CU's 160); a power of two
constexpr int kCountProbes = 4;             // cells a row looks at, from its home slot on
constexpr uint32_t kEmptyCell = 0xFFFFFFFFu; // table_rows < 2^32 - 3: a row index fits 32 bits, and this is none
static_assert((kCountSlots & (kCountSlots - 1)) == 0 && kCountSlots % kCountThreads == 0, "slot masks and the flush loop");

// (explicit address spaces: with generic pointers the compiler merges the LDS add and the global add of the two exits into
// ONE flat atomic on either address)
typedef __attribute__((address_space(3))) uint32_t LdsU32;

// one read of row r: into the block's cell for r, or — no cell within the probes — into counts[r] itself
__device__ __forceinline__ void count_row(uint32_t *counts, LdsU32 *s_key, LdsU32 *s_cnt, uint32_t r) {
#pragma unroll
  for (int p = 0; p < kCountProbes; ++p) {
    const uint32_t slot = (r + p) & (kCountSlots - 1);
    uint32_t k = __hip_atomic_load(&s_key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == kEmptyCell) {
      // what the cell held: still empty = claimed for r
      uint32_t seen = kEmptyCell;
      __hip_atomic_compare_exchange_strong(&s_key[slot], &seen, r, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      k = seen == kEmptyCell ? r : seen;
    }
    if (k == r) {
      (void)__hip_atomic_fetch_add(&s_cnt[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return;
    }
  }
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
  for (int i = tid; i < kCountSlots; i += kCountThreads) {
    s_key[i] = kEmptyCell;
    s_cnt[i] = 0;
  }
  if (tid == 0) s_skipped = 0;
  __syncthreads();

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
      if (live) count_row(counts, (LdsU32 *)s_key, (LdsU32 *)s_cnt, (uint32_t)id[k]);
    }
  }
  if ((tid & 63) == 0 && outside != 0) atomicAdd(&s_skipped, outside);
  __syncthreads();

  for (int i = tid; i < kCountSlots; i += kCountThreads) {
    const uint32_t c = s_cnt[i];
    if (c != 0) atomicAdd(counts + s_key[i], c); // (c != 0: the cell was claimed, its key is a row < table_rows)
  }
  if (tid == 0 && skipped && s_skipped != 0) atomicAdd(skipped, s_skipped);
}

} // namespace

extern "C" int fcp_table_count_ids(uint32_t *counts, int64_t table_rows, const void *ids, int32_t id_bytes, int64_t n, int64_t *skipped,
                                   int32_t device, void *stream) {
  const std::string w = "fcp_table_count_ids: ";
  if (n < 0) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`n` is negative");
  if (table_rows < 1 || table_rows >= (1ll << 32) - 3)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`table_rows` must lie in [1, 2^32 - 3), a plan's row limit");
  if (id_bytes != 4 && id_bytes != 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`id_bytes` is 4 (int32 ids) or 8 (int64 ids)");
  if (n > 0 && !counts) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`counts` is null");
  if (n > 0 && !ids) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`ids` is null");
  if ((uintptr_t)counts % 4) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`counts` is not 4-byte aligned");
  if ((uintptr_t)ids % (uintptr_t)id_bytes)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`ids` is not " + std::to_string(id_bytes) + "-byte aligned");
  if ((uintptr_t)skipped % 8) return fail(FCP_ERR_INVALID_ARGUMENT, w + "`skipped` is not 8-byte aligned");
  if (n == 0) return FCP_OK;
  DeviceGuard guard;
  const int rc = guard.enter(device);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long *sk = reinterpret_cast<unsigned long long *>(skipped);
  const int blocks = (int)std::min<int64_t>(kCountBlocks, n / kTileIds + (n % kTileIds != 0));
  if (id_bytes == 8)
    hipLaunchKernelGGL(fcp_table_count_ids_kernel<int64_t>, dim3(blocks), dim3(kCountThreads), 0, s, counts, (uint64_t)table_rows,
                       static_cast<const int64_t *>(ids), n, sk);
  else
    hipLaunchKernelGGL(fcp_table_count_ids_kernel<int32_t>, dim3(blocks), dim3(kCountThreads), 0, s, counts, (uint64_t)table_rows,
                       static_cast<const int32_t *>(ids), n, sk);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("fcp_table_count_ids: kernel launch", e);
  return FCP_OK;
}
