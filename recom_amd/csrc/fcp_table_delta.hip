// fcp_table_delta.hip — fcp_table_delta_distinct / fcp_table_delta_workspace_bytes: make the ids of a delta pairwise distinct on
// the device, the LAST occurrence of an id winning, before fcp_table_update_rows (fcp_table_rows.hip) and fcp_table_digest_rows
// (fcp_table_digest.hip) see it — both ask for distinct ids and neither checks.  No sort and no lock: the winner of a row is the
// MAXIMUM of the positions that name it, and a maximum commutes.  The reference has no counterpart.
//
// The winners are selected by the classify / fold / compact pipeline of fcp_select_compact.h.  The workspace holds, in this
// order: kDeltaBlocks + 1 of its records (one per block of the fixed grid, and the totals), an open-addressed hash table of
// `cells` {uint32 row, uint32 pos1} cells — cells a power of two, at least 2 n and at least kDeltaMinCells, so the load
// stays at or below 0.5 and an empty cell always exists — and one flag byte per position.  A row's
// home cell is the top bits of row * kDeltaHashMul (64-bit, Fibonacci hashing: ids that share low bits, as the ids of one
// shard do, still spread); probing is linear.  The phases are separate launches; launch boundaries order them, no block ever
// waits for another, and every probe loop is bounded by the number of cells.
//
//   fcp_delta_clear_kernel      every cell {kEmptyCell, 0}: one 8-byte store per cell (what the workspace is aligned to), a stride loop.
//   fcp_delta_insert_kernel<SLOTS>   the grid of fcp_plan_traffic_kernel: 256 threads, tiles of kDeltaInsertTile positions, 4 per
//                     thread kDeltaThreads apart, a stride loop over tiles.  An id is widened to 64 bits (int32: sign-extended)
//                     and compared unsigned against table_rows; an id outside touches nothing.  insert_global: walk from the
//                     home cell, claim an empty cell's key with a compare-and-swap (a key never changes once claimed, so a
//                     relaxed load that sees a stale EMPTY only costs the compare-and-swap that tells the truth), then
//                     atomicMax(pos1, i + 1).  The block first resolves its share in LDS — the row table of
//                     fcp_block_fold.h, SLOTS {row, pos1} cells, an LDS max on a claimed cell, a row without one straight
//                     to insert_global — and flushes one insert_global per occupied cell: a row that every position names
//                     costs one global atomic per block, not one per position.  (One insert_global per position, no LDS, a
//                     build of the commit that introduced the kernel, is as fast on distinct ids and 7x (Zipf) to 260x
//                     (one row) slower on repeated ones: profiles/table_delta.txt)
//   fcp_delta_classify_kernel   the selection grid, kDeltaBlocks blocks at the most.  Position i with an id inside the table looks
//                     its row up (the row is there: the insert phase has run) and WINS when the cell's pos1 is i + 1.  One
//                     flag byte per position (1: wins), and ONE partial record per block: winners, duplicates, skipped.
//   fcp_delta_fold_kernel       one wave: the records' offsets (select_offsets), the totals record, the report.
//   fcp_delta_compact_kernel<V, G>   select_compact: winner number k of the call, in ascending position, writes ids_out[k] — its
//                     id, loaded before the ballot — and pos_out[k]; positions i >= m write the -1 tails.  V > 0: the
//                     winners' rows as bits, rows[p_k] -> rows_out[k].  V == 0: ids only.
// Every output byte is a function of the arguments alone: the hash, the grid and the order of the atomics decide only WHERE a
// row's cell lies and WHEN its maximum is reached.  Nothing is dereferenced by an id's value but the cell it maps to.
// All global atomics are vector forms at agent scope, results unused except the compare-and-swap's; nothing scalar.
// No scratch (-Rpass-analysis=kernel-resource-usage: ScratchSize 0 for every kernel); LDS: the insert kernel's two arrays
// (16 KiB at SLOTS 2048), the compact kernel's winner list and wave counts (1 KiB + 16 bytes), the classify kernel's fold (48 bytes).
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off) // (fcp_table_walk.h's rule; nothing here is floating point)

#include "fcp_table_walk.h" // vec_of, group_of, with_vec, with_group: the rows' V and G, the host's dispatch
#include "fcp_block_fold.h" // wave_fold, block_fold; the block's LDS row table, kEmptyCell
#include "fcp_select_compact.h" // select_grid, select_offsets, select_compact, with_compact_shape: the selection's shared tail
#include "fcp_delta_table.h" // the records, the hash table, ld_id, the geometry's constants: shared with fcp_tables_delta.hip
#include "fcp_tables_delta_plan.h" // check_delta_args, cells_for: the host-only level, shared with the grouped entry

static_assert(fcptd::kMinCells == kDeltaMinCells, "one rule for the cells of a hash table");

namespace {

// one cell per 8-byte store (the workspace is 8-byte aligned, no more)
__global__ void __launch_bounds__(kDeltaThreads) fcp_delta_clear_kernel(uint32_t *cells, uint64_t n_cells) {
  const uint64_t empty = (uint64_t)kEmptyCell; // key in the low half, pos1 = 0 in the high
  for (uint64_t i = (uint64_t)blockIdx.x * kDeltaThreads + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * kDeltaThreads)
    *as_global(reinterpret_cast<uint64_t *>(cells) + i) = empty;
}

template <int SLOTS>
__global__ void __launch_bounds__(kDeltaThreads)
    fcp_delta_insert_kernel(DeltaTable T, const void *ids, int32_t is64, int64_t n, uint64_t table_rows) {
  __shared__ uint32_t s_key[SLOTS];
  __shared__ uint32_t s_pos[SLOTS];
  const int tid = threadIdx.x;
  lds_rows_clear<SLOTS, kDeltaThreads>(s_key, s_pos, tid);
  for (int64_t base = (int64_t)blockIdx.x * kDeltaInsertTile; base < n; base += (int64_t)gridDim.x * kDeltaInsertTile) {
    uint64_t id[kDeltaInsertIdsPerThread];
#pragma unroll
    for (int k = 0; k < kDeltaInsertIdsPerThread; ++k) {
      const int64_t i = base + k * kDeltaThreads + tid;
      id[k] = i < n ? ld_id(ids, i, is64 != 0) : ~0ull; // (~0: outside every table)
    }
#pragma unroll
    for (int k = 0; k < kDeltaInsertIdsPerThread; ++k) {
      if (id[k] >= table_rows) continue;
      // one position of row r: into the block's cell for r, or — no cell within the probes — into the global table
      const uint32_t r = (uint32_t)id[k], pos1 = (uint32_t)(base + k * kDeltaThreads + tid + 1);
      const int slot = lds_rows_claim<SLOTS>((LdsU32 *)s_key, r);
      if (slot >= 0)
        (void)__hip_atomic_fetch_max((LdsU32 *)s_pos + slot, pos1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else
        insert_global(T, r, pos1);
    }
  }
  lds_rows_flush<SLOTS, kDeltaThreads>(s_key, s_pos, tid, [&](uint32_t r, uint32_t pos1) { insert_global(T, r, pos1); });
}

// chunk: positions of a block, a multiple of kDeltaTile; every thread of a block takes the same number of steps
__global__ void __launch_bounds__(kDeltaThreads)
    fcp_delta_classify_kernel(DeltaTable T, const void *ids, int32_t is64, int64_t n, int64_t chunk, uint64_t table_rows, uint8_t *flags,
                              DeltaPartial *partials) {
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * chunk;
  const int64_t c1 = c0 + chunk < n ? c0 + chunk : n;
  DeltaCounts<uint32_t> c = {0, 0, 0};
  for (int64_t t0 = c0; t0 < c1; t0 += kDeltaTile) {
    const int64_t i = t0 + tid;
    if (i < c1) {
      const uint64_t id = ld_id(ids, i, is64 != 0);
      bool win = false;
      if (id < table_rows) {
        win = lookup_global(T, (uint32_t)id) == (uint32_t)(i + 1);
        c.winners += win;
        c.duplicates += !win;
      } else {
        ++c.skipped;
      }
      *as_global(flags + i) = win ? 1 : 0;
    }
  }
  block_fold(c, partials);
}

// one wave; lane l owns the records [l * per, (l + 1) * per) of the nblocks the classify phase wrote (0: it was not launched)
__global__ void __launch_bounds__(64)
    fcp_delta_fold_kernel(DeltaPartial *partials, int32_t nblocks, int64_t n, fcp_table_delta_report_t *report) {
  constexpr int per = kDeltaBlocks / 64;
  const int lane = threadIdx.x;
  const int b0 = lane * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  DeltaCounts<int64_t> c = {0, 0, 0};
  for (int b = b0; b < b1; ++b) fold(c, DeltaCounts<int64_t>{partials[b].winners, partials[b].duplicates, partials[b].skipped});
  select_offsets<kDeltaBlocks>(partials, nblocks, c.winners);
  wave_fold(c);
  if (lane != 0) return;
  partials[kDeltaBlocks] = c;
  fcp_table_delta_report_t r;
  r.n = n;
  r.distinct = c.winners;
  r.duplicates = c.duplicates;
  r.skipped = c.skipped;
  *report = r;
}

struct DeltaCompact {
  const void *ids;
  const float *rows;
  const uint8_t *flags;
  const DeltaPartial *partials;
  int64_t *ids_out, *pos_out; // pos_out may be null
  float *rows_out;
  int64_t n, chunk;
  int32_t is64, dim;
};

// what select_compact asks of the unit: a position's id (loaded before the ballot), a winner's outputs, the -1 tails
struct DeltaEmit {
  const DeltaCompact &A;
  __device__ __forceinline__ uint64_t prepare(int64_t i, bool have) const { return have ? ld_id(A.ids, i, A.is64 != 0) : 0; }
  __device__ __forceinline__ void emit(int64_t k, int64_t i, uint64_t id) const {
    *as_global(A.ids_out + k) = (int64_t)id;
    if (A.pos_out) *as_global(A.pos_out + k) = i;
  }
  __device__ __forceinline__ void tail(int64_t i) const {
    *as_global(A.ids_out + i) = -1;
    if (A.pos_out) *as_global(A.pos_out + i) = -1;
  }
};

// V == 0: ids only (rows and rows_out are null and never read); else G lanes copy a winner's row, V words at a time
template <int V, int G> __global__ void __launch_bounds__(kDeltaThreads) fcp_delta_compact_kernel(const DeltaCompact A) {
  select_compact<V, G, kDeltaBlocks>(A.flags, A.partials, A.n, A.chunk, A.rows, A.rows_out, A.dim, DeltaEmit{A});
}

using fcptd::cells_for;
int64_t partial_bytes() { return (int64_t)(kDeltaBlocks + 1) * (int64_t)sizeof(DeltaPartial); }

} // namespace

extern "C" int64_t fcp_table_delta_workspace_bytes(int64_t n) {
  if (n < 0 || n >= fcpf::kRowLimit) return -1;
  return partial_bytes() + cells_for(n) * 8 + (n + 7) / 8 * 8;
}

extern "C" int fcp_table_delta_distinct(const void *row_ids, int32_t id_bytes, const float *rows, int32_t dim, int64_t n, int64_t table_rows,
                                        int64_t *ids_out, float *rows_out, int64_t *pos_out, fcp_table_delta_report_t *report,
                                        void *workspace, int32_t device, void *stream) {
  std::string why;
  if (const int rc = fcptd::check_delta_args("fcp_table_delta_distinct: ", row_ids, id_bytes, rows, dim, n, table_rows, ids_out, rows_out, pos_out,
                                             report, workspace, &why))
    return fail(rc, why);
  const int vec = rows ? vec_of(dim) : 1;

  DeltaPartial *partials = static_cast<DeltaPartial *>(workspace);
  const int64_t cells = cells_for(n);
  DeltaTable T;
  T.cells = reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + partial_bytes());
  T.mask = (uint64_t)cells - 1;
  T.shift = 64 - __builtin_ctzll((unsigned long long)cells);
  uint8_t *flags = reinterpret_cast<uint8_t *>(T.cells) + cells * 8;
  const auto grid = select_grid(n, kDeltaBlocks, kDeltaMinChunkTiles); // of classify and compact
  const int64_t insert_tiles = (n + kDeltaInsertTile - 1) / kDeltaInsertTile;
  DeltaCompact A;
  A.ids = row_ids;
  A.rows = rows;
  A.flags = flags;
  A.partials = partials;
  A.ids_out = ids_out;
  A.pos_out = pos_out;
  A.rows_out = rows_out;
  A.n = n;
  A.chunk = grid.chunk;
  A.is64 = id_bytes == 8;
  A.dim = dim;
  return on_device("fcp_table_delta_distinct", device, stream, [&](hipStream_t s) {
    const dim3 threads(kDeltaThreads);
    if (n > 0) {
      const unsigned clear_blocks = (unsigned)std::min<int64_t>(kDeltaClearBlocks, (cells + kDeltaThreads - 1) / kDeltaThreads);
      hipLaunchKernelGGL(fcp_delta_clear_kernel, dim3(clear_blocks), threads, 0, s, T.cells, (uint64_t)cells);
      hipLaunchKernelGGL(fcp_delta_insert_kernel<kDeltaSlots>, dim3((unsigned)std::min<int64_t>(insert_tiles, kDeltaInsertMaxBlocks)), threads,
                         0, s, T, row_ids, A.is64, n, (uint64_t)table_rows);
      hipLaunchKernelGGL(fcp_delta_classify_kernel, dim3(grid.nblocks), threads, 0, s, T, row_ids, A.is64, n, grid.chunk, (uint64_t)table_rows, flags,
                         partials);
    }
    hipLaunchKernelGGL(fcp_delta_fold_kernel, dim3(1), dim3(64), 0, s, partials, (int32_t)grid.nblocks, n, report);
    if (n == 0) return;
    with_compact_shape(rows != nullptr, dim, vec, [&](auto v, auto g) {
      hipLaunchKernelGGL((fcp_delta_compact_kernel<decltype(v)::value, decltype(g)::value>), dim3(grid.nblocks), threads, 0, s, A);
    });
  });
}
