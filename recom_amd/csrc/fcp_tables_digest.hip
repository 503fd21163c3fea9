// fcp_tables_digest.hip — fcp_tables_digest / fcp_tables_digest_launches: the digest entries of fcp_table_digest.hip for MANY
// tables in one call.  A model has hundreds to thousands of tables; one call per table is one result, one workspace, two
// launches — nearly every one far too small to fill the machine — and, for a caller that reads the sums, one synchronise per
// table.  Here the number of launches does not grow with the number of tables, and out[k] holds exactly the 32 bytes
// fcp_table_digest (row_ids null) or fcp_table_digest_rows would have left for entry k.  The reference has no counterpart.
//
//   body      digest_body<A, G, BY_ID> of fcp_table_digest_bodies.h: the text the single-table kernel runs, with the block index
//             and the number of blocks LOCAL to the entry.  Nothing about a row's value is written here.
//   front     The host sorts the entries with rows into classes (fcp_tables_digest_plan.cc: (A, G, by-id), the body's template
//             parameters, not folded), deals each entry its blocks — the lone grid, scaled down when a call's lone grids sum to
//             more than 8192 — and builds ONE image per call: 64-byte records, one per entry with rows; per launch a uint32 table
//             of first blocks, prefix[0] = 0 ... prefix[n_recs] = the grid; and one {first, n} run of partial records per entry
//             of the call.  The image goes through a slot of a pinned ring and the upload kernel into the workspace, on the
//             caller's stream; then one launch per class present.  Block b finds its entry by find_piece (fcp_find_piece.h):
//             scalar loads through the constant address space, so every lane of the block agrees on the entry by construction.
//             It ends in block_fold and writes ONE partial record at the launch's partial base + blockIdx.x.
//   fold      fcp_tables_digest_fold_kernel: one wave per entry of the call, in entry order; lane l folds records l, l + 64, ...
//             of the entry's own run (at most 2048), a butterfly joins the lanes, lane 0 writes out[k].  An entry without rows
//             has an empty run: zeros.
//
// No faults, no races, by construction.  Every record, prefix value and run a launch reads was written by the upload in front of
// it on the same stream; the partial records of a call's launches are disjoint runs of kDealBlocks + n_tables records at the
// most, behind the image; the fold reads only what the launches in front of it wrote.  The body's own bounds (i < count, id <
// table_rows) hold as they do alone, whatever the entry's share of blocks is.  No atomics: integer sums are exact in any
// order, so the deal plays no part in the result, and two calls leave the same bytes.  No scratch; LDS only for the 4 wave
// records of a block's fold; no block waits for another; every loop is bounded; byte offsets are formed in 64 bits (the
// body's).  Integer code only.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"
#include "fcp_table_digest.h"

#pragma clang fp contract(off) // (the header's rule; nothing here is floating point)

#include "fcp_table_walk.h"          // with_group, with_one_of: the host's dispatch
#include "fcp_table_digest_bodies.h" // digest_body, DigestPartial
#include "fcp_block_fold.h"          // wave_fold, block_fold
#include "fcp_grouped_front.h"       // find_piece: the search of a block for its entry, asserted against the launch list's bounds
#include "fcp_tables_digest_plan.h"

static_assert(fcpg::kBlockThreads == FCP_BLOCK_THREADS, "the deal of blocks is made for these kernels");
static_assert(sizeof(fcp_table_digest_entry_t) == 64, "fcp_table_digest_entry_t is 64 bytes");

namespace {

using fcpg::Rec;
using fcpg::Run;
static_assert(fcpg::kPartialBytes == sizeof(DigestPartial), "the workspace formula counts these records");

constexpr int kFoldWaves = FCP_BLOCK_THREADS / 64; // entries per block of the fold kernel

template <int A, int G, bool BY_ID>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_tables_digest_kernel(const Rec *recs, const uint32_t *prefix, uint32_t n_recs, DigestPartial *partials) {
  uint32_t block;
  const Rec r = find_piece(recs, prefix, n_recs, blockIdx.x, &block);
  block_fold(digest_body<A, G, BY_ID>(r.base, (int64_t)r.count, r.rb, r.salt, r.row0, r.row_step, r.ids, r.table_rows, block, r.blocks), partials);
}

// wave w of block b: entry 4 b + w.  A wave beyond the last entry leaves as a whole (there is no barrier here).
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_tables_digest_fold_kernel(const Run *runs, const DigestPartial *partials, int32_t n_tables, fcp_table_digest_t *out) {
  const int lane = threadIdx.x & 63;
  const int k = (int)blockIdx.x * kFoldWaves + (int)(threadIdx.x >> 6);
  if (k >= n_tables) return;
  const Run run = runs[k];
  const DigestPartial *mine = partials + run.first;
  DigestPartial p = {0, 0, 0, 0};
  for (uint32_t i = (uint32_t)lane; i < run.n; i += 64) fold(p, mine[i]);
  wave_fold(p);
  if (lane == 0) write_digest(out + k, p);
}

void launch(const fcpg::Launch &l, const Rec *recs, const uint32_t *prefix, DigestPartial *partials, hipStream_t s) {
  const dim3 grid(l.blocks), block(FCP_BLOCK_THREADS);
  with_one_of<8, 4, 2, 1>(l.align, [&](auto a) {
    with_group(l.group, [&](auto g) {
      constexpr int A = decltype(a)::value, G = decltype(g)::value;
      if (l.by_id)
        hipLaunchKernelGGL((fcp_tables_digest_kernel<A, G, true>), grid, block, 0, s, recs, prefix, l.n_recs, partials);
      else
        hipLaunchKernelGGL((fcp_tables_digest_kernel<A, G, false>), grid, block, 0, s, recs, prefix, l.n_recs, partials);
    });
  });
}

} // namespace

extern "C" int32_t fcp_tables_digest_launches(const fcp_table_digest_entry_t *entries, int32_t n_tables, int32_t *blocks) {
  std::string why;
  const int rc = fcpg::check_entries(entries, n_tables, &why);
  if (rc) return -fail(rc, why);
  if (n_tables == 0) return 0;
  fcpg::LaunchList L;
  fcpg::build_launches(entries, n_tables, &L);
  if (blocks)
    for (int32_t k = 0; k < n_tables; ++k) blocks[k] = (int32_t)L.runs[k].n;
  return 2 + (int32_t)L.launches.size();
}

extern "C" int fcp_tables_digest(const fcp_table_digest_entry_t *entries, int32_t n_tables, fcp_table_digest_t *out, void *workspace,
                                 int32_t device, void *stream_) {
  static StageRings rings;
  std::string why;
  int rc = fcpg::check_call(entries, n_tables, out, workspace, &why);
  if (rc) return fail(rc, why);
  if (n_tables == 0) return FCP_OK;
  fcpg::LaunchList L;
  fcpg::build_launches(entries, n_tables, &L);
  const std::string w = "fcp_tables_digest: ";
  const size_t recs_bytes = L.recs_bytes(), prefix_bytes = L.prefix_bytes(), image_bytes = L.image_bytes();
  const int64_t partials_off = fcpg::partials_offset(n_tables);
  uint32_t n_partials = 0;
  for (const fcpg::Launch &l : L.launches) n_partials += l.blocks;
  if ((int64_t)image_bytes > partials_off || (int64_t)n_partials > fcpg::kDealBlocks + n_tables) // (never: the deal and the class count keep both inside)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`entries` need more records than the workspace holds");

  DeviceGuard guard;
  if ((rc = guard.enter(device))) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char *d_image;
  rc = upload_image("fcp_tables_digest", rings, device, stream, workspace, image_bytes,
                    "stream capture of a call with entries: their records are installed from the host by every call, which a replay would "
                    "not repeat",
                    [&](char *buf) { L.write_image(buf); }, &d_image);
  if (rc) return rc;
  const Rec *d_recs = reinterpret_cast<const Rec *>(d_image);
  const uint32_t *d_prefix = reinterpret_cast<const uint32_t *>(d_image + recs_bytes);
  const Run *d_runs = reinterpret_cast<const Run *>(d_image + recs_bytes + prefix_bytes);
  DigestPartial *d_partials = reinterpret_cast<DigestPartial *>(d_image + partials_off);
  for (const fcpg::Launch &l : L.launches) launch(l, d_recs + l.first_rec, d_prefix + l.prefix_off, d_partials + l.partial_first, stream);
  hipLaunchKernelGGL(fcp_tables_digest_fold_kernel, dim3((n_tables + kFoldWaves - 1) / kFoldWaves), dim3(FCP_BLOCK_THREADS), 0, stream, d_runs,
                     d_partials, n_tables, out);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? FCP_OK : hip_fail((w + "kernel launch").c_str(), le);
}
