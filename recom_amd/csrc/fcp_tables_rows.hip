// fcp_tables_rows.hip — fcp_tables_update_rows / fcp_tables_read_rows: the rows-by-id entries of fcp_table_rows.hip for MANY
// tables in one call.  A model has hundreds to thousands of tables and a trainer's delta names rows in most of them; one
// call per table is one device guard, one round of checks and one launch per table, nearly every launch far too small to fill
// the machine.  Here the number of launches does not grow with the number of tables.  The reference has no counterpart.
//
//   bodies    update_q8_body<V, G>, update_rows_body<V>, read_rows_body<V> of fcp_table_rows_bodies.h: the text the single-table
//             kernels run, with the block index LOCAL to the entry.  Nothing about a row is written here.
//   front     The host sorts the entries with rows into classes (fcp_tables_rows_plan.cc: a q8 update by (V, G), everything
//             else by V) and builds ONE image per call: 64-byte records, one per entry (an entry of more than 2^30 threads:
//             one per piece, cut where the single-table host cuts its launches), and per launch a uint32 table of first
//             blocks, prefix[0] = 0 ... prefix[n_recs] = the grid.  The image goes through a slot of a pinned ring and
//             the upload kernel into the workspace, on the caller's stream; then one launch per class, whose grid is exactly
//             the sum of its entries' blocks — one entry of a million rows among 999 small ones launches no idle block.
//             Block b finds its entry j, prefix[j] <= b < prefix[j + 1], by a binary search of at most 17 steps (n_recs <=
//             65537) from blockIdx.x alone: the table and the records are read through the constant address space, so
//             the search and the record are scalar loads into SGPRs and every lane of the block agrees on the entry by
//             construction.  The streaming kernels take `kind` from the record: the wave-uniform branch it already was.
//
// No faults, no races beyond the single-table entries', by construction.  Every record and prefix value a launch reads was
// written by the upload in front of it on the same stream.  An entry's blocks are exactly ceil(threads / 256), so the body's own
// bounds (row < rows, i < n) hold as they do alone.  No LDS, no scratch, no atomic but the skipped add, no block waits for
// another, every loop is bounded; byte offsets are formed in 64 bits (the bodies').  Contraction is off, as in
// fcp_table_rows.hip.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off)

#include "fcp_table_walk.h"
#include "fcp_table_rows_bodies.h"
#include "fcp_grouped_front.h" // find_piece: the search of a block for its entry, asserted against the launch list's bounds
#include "fcp_tables_rows_plan.h"

static_assert(FCP_TAB_BF16 == FCP_OUT_BF16 && FCP_TAB_F16 == FCP_OUT_F16, "st_out_narrow takes the table kind as its output kind");
static_assert(fcpr::kBlockThreads == FCP_BLOCK_THREADS && fcpr::kMaxLaunchThreads == kMaxLaunchThreads, "the launch list is cut for these kernels");
static_assert(sizeof(fcp_table_rows_t) == 64, "fcp_table_rows_t is 64 bytes");

namespace {

using fcpr::Rec;
template <int V, int G>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_tables_update_q8_kernel(const Rec *recs, const uint32_t *prefix, uint32_t n_recs) {
  uint32_t block;
  const Rec r = find_piece(recs, prefix, n_recs, blockIdx.x, &block);
  update_q8_body<V, G>(static_cast<char *>(r.table), r.ids, r.rows, (int32_t)r.n, r.dim, r.table_rows,
                       reinterpret_cast<unsigned long long *>(r.skipped), block);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_tables_update_rows_kernel(const Rec *recs, const uint32_t *prefix, uint32_t n_recs) {
  uint32_t block;
  const Rec r = find_piece(recs, prefix, n_recs, blockIdx.x, &block);
  update_rows_body<V>(static_cast<char *>(r.table), r.ids, r.rows, r.n, r.spr, r.dim, r.kind, r.table_rows,
                      reinterpret_cast<unsigned long long *>(r.skipped), block);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_tables_read_rows_kernel(const Rec *recs, const uint32_t *prefix, uint32_t n_recs) {
  uint32_t block;
  const Rec r = find_piece(recs, prefix, n_recs, blockIdx.x, &block);
  read_rows_body<V>(r.rows, static_cast<const char *>(r.table), r.ids, r.n, r.spr, r.dim, r.kind, r.table_rows, block);
}

void launch(const fcpr::Launch &l, bool update, const Rec *recs, const uint32_t *prefix, hipStream_t s) {
  const dim3 grid(l.blocks), block(FCP_BLOCK_THREADS);
  with_vec(l.vec, [&](auto v) {
    constexpr int V = decltype(v)::value;
    if (!update)
      hipLaunchKernelGGL(fcp_tables_read_rows_kernel<V>, grid, block, 0, s, recs, prefix, l.n_recs);
    else if (l.group == 0)
      hipLaunchKernelGGL(fcp_tables_update_rows_kernel<V>, grid, block, 0, s, recs, prefix, l.n_recs);
    else
      with_group(l.group, [&](auto g) {
        hipLaunchKernelGGL((fcp_tables_update_q8_kernel<V, decltype(g)::value>), grid, block, 0, s, recs, prefix, l.n_recs);
      });
  });
}

// What both entries do; `rings`: the entry's own pinned staging (StageRings, fcp_host.h).
int run(const char *who, bool update, StageRings &rings, const fcp_table_rows_t *entries, int32_t n_tables, int64_t *skipped,
        void *workspace, int32_t device, void *stream_) {
  std::string why;
  int rc = fcpr::check_call(who, entries, n_tables, skipped, workspace, &why);
  if (rc) return fail(rc, why);
  fcpr::LaunchList L;
  fcpr::build_launches(entries, n_tables, update, skipped, &L);
  if (L.launches.empty()) return FCP_OK;
  const std::string w = std::string(who) + ": ";
  const size_t recs_bytes = L.recs_bytes(), image_bytes = recs_bytes + L.prefix_bytes();
  if ((int64_t)(16 + image_bytes) > fcpr::workspace_bytes(n_tables)) // (never: the element bound of check_call keeps the image inside)
    return fail(FCP_ERR_INVALID_ARGUMENT, w + "`entries` need more pieces than the workspace holds");

  DeviceGuard guard;
  if ((rc = guard.enter(device))) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char *d_image;
  rc = upload_image(who, rings, device, stream, workspace, image_bytes,
                    "stream capture of a call with rows: the entries' records are installed from the host by every call, which a replay "
                    "would not repeat",
                    [&](char *buf) { L.write_image(buf); }, &d_image);
  if (rc) return rc;
  const Rec *d_recs = reinterpret_cast<const Rec *>(d_image);
  const uint32_t *d_prefix = reinterpret_cast<const uint32_t *>(d_image + recs_bytes);
  for (const fcpr::Launch &l : L.launches) launch(l, update, d_recs + l.first_rec, d_prefix + l.prefix_off, stream);
  const hipError_t le = hipGetLastError();
  return le == hipSuccess ? FCP_OK : hip_fail((w + "kernel launch").c_str(), le);
}

} // namespace

extern "C" int32_t fcp_tables_rows_launches(const fcp_table_rows_t *entries, int32_t n_tables) {
  std::string why;
  const int rc = fcpr::check_entries("fcp_tables_rows_launches", entries, n_tables, &why);
  if (rc) return -fail(rc, why);
  fcpr::LaunchList L;
  fcpr::build_launches(entries, n_tables, /*update*/ true, nullptr, &L);
  return L.launches.empty() ? 0 : 1 + (int32_t)L.launches.size();
}

extern "C" int fcp_tables_update_rows(const fcp_table_rows_t *entries, int32_t n_tables, int64_t *skipped, void *workspace, int32_t device,
                                      void *stream) {
  static StageRings rings;
  return run("fcp_tables_update_rows", true, rings, entries, n_tables, skipped, workspace, device, stream);
}

extern "C" int fcp_tables_read_rows(const fcp_table_rows_t *entries, int32_t n_tables, void *workspace, int32_t device, void *stream) {
  static StageRings rings;
  return run("fcp_tables_read_rows", false, rings, entries, n_tables, nullptr, workspace, device, stream);
}
