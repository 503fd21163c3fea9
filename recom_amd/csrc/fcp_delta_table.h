// fcp_delta_table.h — what the two delta units share on the device: fcp_table_delta.hip (one table) and fcp_tables_delta.hip (a
// model's tables in one call) count a position into the same records and keep a row's winner in the same open-addressed hash
// table of {uint32 row, uint32 pos1} cells.  The records (DeltaPartial, DeltaCounts), the table (DeltaTable, home_of,
// insert_global, lookup_global), ld_id and the geometry's constants are written here ONCE, the text fcp_table_delta.hip held;
// that unit's header comment describes them.  The grouped entry's "byte for byte what the single-table entry leaves" rests on
// this: one hash, one probe order, one rule for who wins.  Unnamed namespace, as fcp_block_fold.h.
#pragma once
#include "fcp_fused_bodies.h"
#include "fcp_block_fold.h"     // kEmptyCell
#include "fcp_select_compact.h" // kSelectTile

namespace {

constexpr int kDeltaThreads = FCP_BLOCK_THREADS;
constexpr int kDeltaTile = kSelectTile;             // positions of one step of a classify / compact block
constexpr int kDeltaBlocks = 1024;                  // the fixed grid of classify / compact; also the partial records
constexpr int kDeltaMinChunkTiles = 4;              // a block's chunk is at least this many tiles
constexpr int kDeltaInsertIdsPerThread = 4;
constexpr int kDeltaInsertTile = kDeltaThreads * kDeltaInsertIdsPerThread;
constexpr int kDeltaInsertMaxBlocks = 65535;        // longer deltas: the stride loop
constexpr int kDeltaClearBlocks = 4096;
constexpr int kDeltaSlots = 2048;                   // cells of a block's LDS table: 2 x 8 KiB, for a tile of 1024 positions
constexpr int64_t kDeltaMinCells = 64;
constexpr uint64_t kDeltaHashMul = 0x9E3779B97F4A7C15ull;

// What a block of the classify phase counted, and, once the fold has run, where its winners go.  32 bytes.
struct DeltaPartial {
  int64_t winners, duplicates, skipped;
  int64_t offset; // winners of the blocks before this one (the totals record: unused)
};
static_assert(sizeof(DeltaPartial) == 32 && sizeof(fcp_table_delta_report_t) == 32, "records of 32 bytes");

// What a lane, a wave and a block of the classify phase count (uint32_t: a chunk stays below 2^32 positions), and what the
// lanes of the fold sum (int64_t)
template <class T> struct DeltaCounts {
  T winners, duplicates, skipped;
  __device__ operator DeltaPartial() const { return DeltaPartial{(int64_t)winners, (int64_t)duplicates, (int64_t)skipped, 0}; }
};
template <class T> __device__ __forceinline__ void fold(DeltaCounts<T> &a, const DeltaCounts<T> &b) {
  a.winners += b.winners;
  a.duplicates += b.duplicates;
  a.skipped += b.skipped;
}

struct DeltaTable {
  uint32_t *cells; // cell c: key at cells[2 c], pos1 at cells[2 c + 1]
  uint64_t mask;   // cells - 1
  int32_t shift;   // 64 - log2(cells)
};

__device__ __forceinline__ uint64_t ld_id(const void *ids, int64_t i, bool is64) {
  return is64 ? (uint64_t)*as_global(static_cast<const int64_t *>(ids) + i)
              : (uint64_t)(int64_t)*as_global(static_cast<const int32_t *>(ids) + i);
}

__device__ __forceinline__ uint64_t home_of(const DeltaTable &T, uint32_t row) { return ((uint64_t)row * kDeltaHashMul) >> T.shift; }

// pos1 into the cell of `row`, claiming one if the row has none yet.  At most `cells` steps; the load is at or below 0.5.
__device__ __forceinline__ void insert_global(const DeltaTable &T, uint32_t row, uint32_t pos1) {
  uint64_t c = home_of(T, row);
  for (uint64_t step = 0; step <= T.mask; ++step, c = (c + 1) & T.mask) {
    uint32_t *key = T.cells + 2 * c;
    uint32_t k = __hip_atomic_load(as_global(key), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kEmptyCell) {
      uint32_t seen = kEmptyCell; // what the cell held: still empty = claimed for row
      __hip_atomic_compare_exchange_strong(as_global(key), &seen, row, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      k = seen == kEmptyCell ? row : seen;
    }
    if (k == row) {
      (void)__hip_atomic_fetch_max(as_global(key + 1), pos1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
}

// the pos1 of `row`'s cell; 0 if the row has none (the insert phase gave every row inside the table one)
__device__ __forceinline__ uint32_t lookup_global(const DeltaTable &T, uint32_t row) {
  uint64_t c = home_of(T, row);
  for (uint64_t step = 0; step <= T.mask; ++step, c = (c + 1) & T.mask) {
    const uint64_t cell = *as_global(reinterpret_cast<const uint64_t *>(T.cells + 2 * c)); // key in the low half, pos1 in the high
    if ((uint32_t)cell == row) return (uint32_t)(cell >> 32);
    if ((uint32_t)cell == kEmptyCell) return 0;
  }
  return 0;
}

} // namespace
