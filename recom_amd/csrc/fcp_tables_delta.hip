// fcp_tables_delta.hip — fcp_tables_delta_distinct / fcp_tables_delta_launches: fcp_table_delta_distinct (fcp_table_delta.hip) for
// MANY tables in one call.  The grouped row entries (fcp_tables_rows.hip, fcp_tables_digest.hip) ask that the ids of each entry
// be pairwise distinct and none of them checks; the single-table entry that guarantees it makes five launches per table.  Here
// the number of launches does not grow with the number of tables, and entry k is left, byte for byte, what one
// fcp_table_delta_distinct call with its arguments leaves.  The reference has no counterpart.
//
//   front     The host (fcp_tables_delta_plan.cc) sorts the entries with ids into compact classes — ids only, or the (V, G) of
//             with_compact_shape — deals each entry its classify / compact grid (the lone select_grid, scaled down when a call's
//             lone grids sum past 8192) and builds ONE image per call: 128-byte records sorted by class, a first-block table per
//             compact launch, one for the insert launch and one for the classify launch (both take every record), and one run
//             per entry of the call for the fold.  The image goes through a slot of a pinned ring and the upload kernel into the
//             workspace, on the caller's stream.  Block b finds its entry by find_piece (fcp_find_piece.h): scalar loads through
//             the constant address space, so every lane of the block agrees on the entry by construction, and A BLOCK BELONGS TO
//             ONE ENTRY FOR ITS WHOLE LIFE — the insert block's LDS row table never mixes entries, and its stride loop runs over
//             the block's LOCAL index and the entry's LOCAL grid, both from the record.
//   tables    Every entry has its OWN hash table of cells_for(n) cells, keys the entry's 32-bit rows; the tables lie back to back,
//             so ONE clear launch covers them.  Two entries with the same ids, for the same table or not, never meet.
//   kernels   clear; insert<SLOTS>, classify, compact<V, G>: the single-table unit's steps (fcp_delta_table.h: one hash, one
//             probe order, one rule for who wins; select_compact_at, block_fold_to: the run-time forms) with the block index
//             local to the entry; fold: one wave per entry of the call, `per` records per lane a run-time value, the entry's
//             offsets, its totals record and reports[k].  An entry without ids: zeros into reports[k], nothing else.
// Byte equality with the single-table call follows from that entry's own "every output byte is a function of the arguments
// alone": the hash, the grid, the deal and the order of the atomics decide only WHERE a row's cell lies and WHEN its maximum is
// reached.  The workspace's content before the call plays no part: every cell, flag, record and offset a kernel reads was
// written by a launch in front of it on the same stream.
//
// No faults, no races beyond the single-table entry's, by construction.  An entry's blocks are exactly its record's nblocks /
// insert_blocks, so the bodies' own bounds (i < n) hold as they do alone; an entry's sections of the workspace are disjoint
// from every other's (fcp_tables_delta_plan.h: the layout).  No block waits for another; every probe and search loop is
// bounded (the cells of a table, kSearchSteps); byte offsets are formed in 64 bits.  All global atomics are vector forms at agent
// scope, results unused except the compare-and-swap's; nothing scalar is written.  No scratch
// (-Rpass-analysis=kernel-resource-usage: ScratchSize 0 for every kernel of this unit); LDS: the insert kernel's two arrays
// (16 KiB), the compact kernel's winner list and wave counts (1 KiB + 16 bytes), the classify kernel's fold (48 bytes).
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off) // (fcp_table_walk.h's rule; nothing here is floating point)

#include "fcp_table_walk.h"     // with_vec, with_group: the host's dispatch
#include "fcp_block_fold.h"     // wave_fold, block_fold_to; the block's LDS row table
#include "fcp_select_compact.h" // select_offsets_n, select_compact_at
#include "fcp_delta_table.h"    // the records, the hash table, ld_id, the geometry's constants
#include "fcp_grouped_front.h"  // find_piece: the search of a block for its entry, asserted against the launch list's bounds
#include "fcp_tables_delta_plan.h"

static_assert(fcptd::kBlockThreads == FCP_BLOCK_THREADS && fcptd::kTile == kDeltaTile && fcptd::kLoneBlocks == kDeltaBlocks &&
                  fcptd::kMinChunkTiles == kDeltaMinChunkTiles && fcptd::kInsertTile == kDeltaInsertTile &&
                  fcptd::kInsertMaxBlocks == kDeltaInsertMaxBlocks && fcptd::kMinCells == kDeltaMinCells,
              "the deal of blocks and the layout are made for these kernels");
static_assert(fcptd::kPartialBytes == sizeof(DeltaPartial), "the workspace formula counts these records");
static_assert(sizeof(fcp_table_delta_entry_t) == 64, "fcp_table_delta_entry_t is 64 bytes");

namespace {

using fcptd::Rec;
using fcptd::Run;

constexpr int kFoldWaves = FCP_BLOCK_THREADS / 64; // entries per block of the fold kernel

__device__ __forceinline__ DeltaTable table_of(const Rec &r) {
  DeltaTable T;
  T.cells = r.cells;
  T.mask = (1ull << (64 - r.shift)) - 1;
  T.shift = r.shift;
  return T;
}

// every cell of every entry's table: one cell per 8-byte store
__global__ void __launch_bounds__(kDeltaThreads) fcp_tables_delta_clear_kernel(uint64_t *cells, uint64_t n_cells) {
  const uint64_t empty = (uint64_t)kEmptyCell; // key in the low half, pos1 = 0 in the high
  for (uint64_t i = (uint64_t)blockIdx.x * kDeltaThreads + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * kDeltaThreads)
    *as_global(cells + i) = empty;
}

// fcp_delta_insert_kernel for the block's entry: tile `block`, `block + insert_blocks`, ... of the entry's positions
template <int SLOTS>
__global__ void __launch_bounds__(kDeltaThreads) fcp_tables_delta_insert_kernel(const Rec *recs, const uint32_t *prefix, uint32_t n_recs) {
  __shared__ uint32_t s_key[SLOTS];
  __shared__ uint32_t s_pos[SLOTS];
  uint32_t block;
  const Rec r = find_piece(recs, prefix, n_recs, blockIdx.x, &block);
  const DeltaTable T = table_of(r);
  const int tid = threadIdx.x;
  lds_rows_clear<SLOTS, kDeltaThreads>(s_key, s_pos, tid);
  for (int64_t base = (int64_t)block * kDeltaInsertTile; base < r.n; base += (int64_t)r.insert_blocks * kDeltaInsertTile) {
    uint64_t id[kDeltaInsertIdsPerThread];
#pragma unroll
    for (int k = 0; k < kDeltaInsertIdsPerThread; ++k) {
      const int64_t i = base + k * kDeltaThreads + tid;
      id[k] = i < r.n ? ld_id(r.ids, i, r.is64 != 0) : ~0ull; // (~0: outside every table)
    }
#pragma unroll
    for (int k = 0; k < kDeltaInsertIdsPerThread; ++k) {
      if (id[k] >= r.table_rows) continue;
      // one position of row row: into the block's cell for it, or — no cell within the probes — into the entry's global table
      const uint32_t row = (uint32_t)id[k], pos1 = (uint32_t)(base + k * kDeltaThreads + tid + 1);
      const int slot = lds_rows_claim<SLOTS>((LdsU32 *)s_key, row);
      if (slot >= 0)
        (void)__hip_atomic_fetch_max((LdsU32 *)s_pos + slot, pos1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      else
        insert_global(T, row, pos1);
    }
  }
  lds_rows_flush<SLOTS, kDeltaThreads>(s_key, s_pos, tid, [&](uint32_t row, uint32_t pos1) { insert_global(T, row, pos1); });
}

// fcp_delta_classify_kernel for the block's entry: chunk `block` of its positions, ONE record at the entry's partials[block]
__global__ void __launch_bounds__(kDeltaThreads) fcp_tables_delta_classify_kernel(const Rec *recs, const uint32_t *prefix, uint32_t n_recs) {
  uint32_t block;
  const Rec r = find_piece(recs, prefix, n_recs, blockIdx.x, &block);
  const DeltaTable T = table_of(r);
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)block * r.chunk;
  const int64_t c1 = c0 + r.chunk < r.n ? c0 + r.chunk : r.n;
  DeltaCounts<uint32_t> c = {0, 0, 0};
  for (int64_t t0 = c0; t0 < c1; t0 += kDeltaTile) {
    const int64_t i = t0 + tid;
    if (i < c1) {
      const uint64_t id = ld_id(r.ids, i, r.is64 != 0);
      bool win = false;
      if (id < r.table_rows) {
        win = lookup_global(T, (uint32_t)id) == (uint32_t)(i + 1);
        c.winners += win;
        c.duplicates += !win;
      } else {
        ++c.skipped;
      }
      *as_global(r.flags + i) = win ? 1 : 0;
    }
  }
  block_fold_to(c, static_cast<DeltaPartial *>(r.partials) + block);
}

// wave w of block b: entry 4 b + w of the call.  Lane l owns the records [l * per, (l + 1) * per) of the entry's nblocks.  A wave
// beyond the last entry, and one of an entry without ids, leaves as a whole (there is no barrier here).  runs == null: no entry
// of the call has ids.
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_tables_delta_fold_kernel(const Run *runs, DeltaPartial *partials, int32_t n_tables, fcp_table_delta_report_t *reports) {
  const int lane = threadIdx.x & 63;
  const int k = (int)blockIdx.x * kFoldWaves + (int)(threadIdx.x >> 6);
  if (k >= n_tables) return;
  const Run run = runs ? runs[k] : Run{0, 0, 0};
  const int nblocks = (int)run.nblocks;
  if (nblocks == 0) {
    if (lane == 0) reports[k] = fcp_table_delta_report_t{0, 0, 0, 0};
    return;
  }
  DeltaPartial *mine = partials + run.first;
  const int per = (nblocks + 63) / 64;
  const int b0 = lane * per < nblocks ? lane * per : nblocks, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  DeltaCounts<int64_t> c = {0, 0, 0};
  for (int b = b0; b < b1; ++b) fold(c, DeltaCounts<int64_t>{mine[b].winners, mine[b].duplicates, mine[b].skipped});
  select_offsets_n(mine, nblocks, per, c.winners);
  wave_fold(c);
  if (lane != 0) return;
  mine[nblocks] = c;
  fcp_table_delta_report_t r;
  r.n = run.n;
  r.distinct = c.winners;
  r.duplicates = c.duplicates;
  r.skipped = c.skipped;
  reports[k] = r;
}

// what select_compact_at asks of the unit: a position's id (loaded before the ballot), a winner's outputs, the -1 tails
struct TablesDeltaEmit {
  const Rec &r;
  __device__ __forceinline__ uint64_t prepare(int64_t i, bool have) const { return have ? ld_id(r.ids, i, r.is64 != 0) : 0; }
  __device__ __forceinline__ void emit(int64_t k, int64_t i, uint64_t id) const {
    *as_global(r.ids_out + k) = (int64_t)id;
    if (r.pos_out) *as_global(r.pos_out + k) = i;
  }
  __device__ __forceinline__ void tail(int64_t i) const {
    *as_global(r.ids_out + i) = -1;
    if (r.pos_out) *as_global(r.pos_out + i) = -1;
  }
};

// V == 0: ids only (rows and rows_out are null and never read); else G lanes copy a winner's row, V words at a time
template <int V, int G>
__global__ void __launch_bounds__(kDeltaThreads) fcp_tables_delta_compact_kernel(const Rec *recs, const uint32_t *prefix, uint32_t n_recs) {
  uint32_t block;
  const Rec r = find_piece(recs, prefix, n_recs, blockIdx.x, &block);
  select_compact_at<V, G>(r.flags, static_cast<const DeltaPartial *>(r.partials), block, r.nblocks, r.n, r.chunk, r.rows, r.rows_out, r.dim,
                          TablesDeltaEmit{r});
}

void launch_compact(const fcptd::Launch &l, const Rec *recs, const uint32_t *prefix, hipStream_t s) {
  const dim3 grid(l.blocks), block(kDeltaThreads);
  if (l.vec == 0) {
    hipLaunchKernelGGL((fcp_tables_delta_compact_kernel<0, 1>), grid, block, 0, s, recs, prefix, l.n_recs);
    return;
  }
  with_vec(l.vec, [&](auto v) {
    with_group(l.group, [&](auto g) {
      hipLaunchKernelGGL((fcp_tables_delta_compact_kernel<decltype(v)::value, decltype(g)::value>), grid, block, 0, s, recs, prefix, l.n_recs);
    });
  });
}

} // namespace

extern "C" int32_t fcp_tables_delta_deal_blocks(void) { return (int32_t)fcptd::kDealBlocks; }

extern "C" int32_t fcp_tables_delta_grid(const fcp_table_delta_entry_t *entries, int32_t n_tables, int32_t *blocks) {
  std::string why;
  const int rc = fcptd::check_entries("fcp_tables_delta_grid", entries, n_tables, &why);
  if (rc) return -fail(rc, why);
  fcptd::LaunchList L;
  fcptd::build_launches(entries, n_tables, 0, &L);
  if (blocks)
    for (int32_t k = 0; k < n_tables; ++k) blocks[k] = (int32_t)L.blocks[k];
  return (int32_t)L.classify_grid();
}

extern "C" int32_t fcp_tables_delta_launches(const fcp_table_delta_entry_t *entries, int32_t n_tables) {
  std::string why;
  const int rc = fcptd::check_entries("fcp_tables_delta_launches", entries, n_tables, &why);
  if (rc) return -fail(rc, why);
  fcptd::LaunchList L;
  fcptd::build_launches(entries, n_tables, 0, &L);
  return L.n_launches();
}

extern "C" int fcp_tables_delta_distinct(const fcp_table_delta_entry_t *entries, int32_t n_tables, fcp_table_delta_report_t *reports,
                                         void *workspace, int32_t device, void *stream_) {
  static StageRings rings;
  const char *who = "fcp_tables_delta_distinct";
  std::string why;
  int rc = fcptd::check_call(entries, n_tables, reports, workspace, &why);
  if (rc) return fail(rc, why);
  if (n_tables == 0) return FCP_OK;
  char *image = reinterpret_cast<char *>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  fcptd::LaunchList L;
  fcptd::build_launches(entries, n_tables, (uintptr_t)image, &L);
  const std::string w = std::string(who) + ": ";
  if ((int64_t)L.image_bytes() > fcptd::image_room(n_tables)) // (never: one record per entry, one launch per class)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`entries` need more records than the workspace holds");

  DeviceGuard guard;
  if ((rc = guard.enter(device))) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const dim3 threads(kDeltaThreads), fold_grid((n_tables + kFoldWaves - 1) / kFoldWaves);
  if (L.recs.empty()) { // every n == 0: only the reports are written, and nothing is installed
    hipLaunchKernelGGL(fcp_tables_delta_fold_kernel, fold_grid, threads, 0, stream, (const Run *)nullptr, (DeltaPartial *)nullptr, n_tables, reports);
    const hipError_t le = hipGetLastError();
    return le == hipSuccess ? FCP_OK : hip_fail((w + "kernel launch").c_str(), le);
  }
  char *d_image;
  rc = upload_image(who, rings, device, stream, workspace, L.image_bytes(),
                    "stream capture of a call with ids: the entries' records are installed from the host by every call, which a replay "
                    "would not repeat",
                    [&](char *buf) { L.write_image(buf); }, &d_image);
  if (rc) return rc;
  const fcptd::Layout lay = fcptd::layout_of(entries, n_tables);
  const Rec *d_recs = reinterpret_cast<const Rec *>(d_image);
  const uint32_t *d_prefix = reinterpret_cast<const uint32_t *>(d_image + L.recs_bytes());
  const uint32_t *d_insert = reinterpret_cast<const uint32_t *>(d_image + L.insert_off());
  const uint32_t *d_classify = reinterpret_cast<const uint32_t *>(d_image + L.classify_off());
  const Run *d_runs = reinterpret_cast<const Run *>(d_image + L.runs_off());
  DeltaPartial *d_partials = reinterpret_cast<DeltaPartial *>(d_image + lay.partials_off);
  const uint32_t n_recs = (uint32_t)L.recs.size();
  const unsigned clear_blocks = (unsigned)std::min<uint64_t>(kDeltaClearBlocks, (L.total_cells + kDeltaThreads - 1) / kDeltaThreads);
  hipLaunchKernelGGL(fcp_tables_delta_clear_kernel, dim3(clear_blocks), threads, 0, stream, reinterpret_cast<uint64_t *>(d_image + lay.cells_off),
                     L.total_cells);
  hipLaunchKernelGGL(fcp_tables_delta_insert_kernel<kDeltaSlots>, dim3(L.insert_grid()), threads, 0, stream, d_recs, d_insert, n_recs);
  hipLaunchKernelGGL(fcp_tables_delta_classify_kernel, dim3(L.classify_grid()), threads, 0, stream, d_recs, d_classify, n_recs);
  hipLaunchKernelGGL(fcp_tables_delta_fold_kernel, fold_grid, threads, 0, stream, d_runs, d_partials, n_tables, reports);
  for (const fcptd::Launch &l : L.launches) launch_compact(l, d_recs + l.first_rec, d_prefix + l.prefix_off, stream);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? FCP_OK : hip_fail((w + "kernel launch").c_str(), le);
}
