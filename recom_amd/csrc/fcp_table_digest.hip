// fcp_table_digest.hip — fcp_table_digest / fcp_table_digest_rows / fcp_table_digest_workspace_bytes: an order-free 64-bit sum
// of row hashes over a table in any of the formats the plans read (FCP_TAB_F32 / _BF16 / _F16 / _Q8), computed where the table
// lies.  What fcp_table_convert, fcp_table_update_rows and a loader promise is BYTES; this is how a deployment checks them on
// the table it serves.  The value model is fcp_table_digest.h's (shared with fcp_table_digest_host.cc): a row is its bytes as
// little-endian 64-bit words, the last one zero-padded; H(r) = mix(salt + (r + 1) * G + sum_j mix(w[j] ^ (j + 1) * G)); the
// digest is the sum of H over the rows, modulo 2^64.  The reference reads float32 tables only and has no counterpart.
//
//   fcp_table_digest_kernel<A, G, BY_ID>   (its body, digest_body, lives in fcp_table_digest_bodies.h: fcp_tables_digest.hip runs
//                     the same text for many tables per call, with the block index and the grid local to an entry)  the grid of fcp_table_audit_kernel: kDigestBlocks blocks of FCP_BLOCK_THREADS, fewer
//                     when the rows do not fill it, a 64-bit grid-stride walk, a power-of-two group of G <= 64 lanes per row —
//                     G the largest power of two not above the row's words, so lane l of a group loads words l and l + G (fewer
//                     than 2 G words unless G is 64: words l + 128, l + 192, ... in a loop) and a wave's loads of its rows are
//                     contiguous.  kUnroll rows per step of the walk, their first two loads per lane issued before the first
//                     multiply.  A: what the host knows of the rows' alignment, 8 | 4 | 2 | 1 — the
//                     largest power of two up to 8 that divides the first row's address and the row bytes; words are loaded
//                     through typedefs of that alignment (as ld_q8_raw reads a q8 row's pair), so a q8 row may start at any
//                     byte.  The last word of a row of rb % 8 != 0 bytes is put together from loads of 4, 2 and 1 bytes that
//                     stay inside the row — EVERY row's, not only the last row's — so no load touches a byte outside the rows.
//                     Word terms are added inside the group by __shfl_xor butterflies; the group's first lane forms H and adds
//                     it to its own sum.  Lanes of rows beyond the end take part in the exchanges and touch no memory.
//                     BY_ID (fcp_table_digest_rows): the group's row comes from row_ids — every lane of the group loads the
//                     same id, as in fcp_update_q8_kernel; an id outside [0, table_rows), compared as a whole unsigned 64-bit
//                     value, touches no memory and counts in `skipped`.
//                     At the end a block folds its lanes — butterflies inside a wave, its four waves through LDS — and writes
//                     ONE partial record to the workspace.
//   fcp_table_digest_fold_kernel   one wave: lane l folds records l, l + 64, ..., a butterfly joins the lanes, lane 0 writes
//                     fcp_table_digest_t.  rows == 0 / n == 0 launches it alone: zeros.
// No atomics (same-address atomics from every block: 12.7 ns each, README).  Integer sums are exact in any order: which lane
// adds which row plays no part in the result, and two calls leave the same bytes by construction.
//
// No scratch; LDS only for the 4 wave records of a block's fold.  Integer code only.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"
#include "fcp_table_digest.h"

#pragma clang fp contract(off) // (the header's rule; nothing here is floating point)

#include "fcp_table_walk.h"          // with_group, with_one_of: the host's dispatch
#include "fcp_table_digest_bodies.h" // digest_body, DigestPartial: shared with fcp_tables_digest.hip
#include "fcp_block_fold.h"          // wave_fold, block_fold: the fold of a lane's record into the block's
#include "fcp_tables_digest_plan.h"  // group_of_words, align_of, lone_blocks: the rules the grouped entry classes by

namespace {

constexpr int kDigestBlocks = fcpg::kLoneBlocks; // the fixed grid: 8 blocks of 256 threads on each of 256 CUs; also the records of the workspace

// digest_body with the block's own index and the grid: see fcp_table_digest_bodies.h
template <int A, int G, bool BY_ID>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_table_digest_kernel(const char *base, int64_t count, int32_t rb, uint64_t salt, uint64_t row0, uint64_t row_step,
                            const int64_t *row_ids, uint64_t table_rows, DigestPartial *partials) {
  block_fold(digest_body<A, G, BY_ID>(base, count, rb, salt, row0, row_step, row_ids, table_rows, blockIdx.x, gridDim.x), partials);
}

// one wave; n: records of the workspace the first kernel wrote (0: it was not launched)
__global__ void __launch_bounds__(64) fcp_table_digest_fold_kernel(const DigestPartial *partials, int32_t n, fcp_table_digest_t *out) {
  const int lane = threadIdx.x;
  DigestPartial p = {0, 0, 0, 0};
  for (int i = lane; i < n; i += 64) fold(p, partials[i]);
  wave_fold(p);
  if (lane == 0) write_digest(out, p);
}

struct DigestLaunch {
  const char *base;
  int64_t count;
  int32_t rb;
  uint64_t salt, row0, row_step;
  const int64_t *row_ids; // null: the rows lie back to back from `base`
  uint64_t table_rows;
  DigestPartial *partials;
  int blocks;
};

template <int A, int G> void launch_ag(const DigestLaunch &L, hipStream_t s) {
  if (L.row_ids)
    hipLaunchKernelGGL((fcp_table_digest_kernel<A, G, true>), dim3(L.blocks), dim3(FCP_BLOCK_THREADS), 0, s, L.base, L.count, L.rb, L.salt,
                       L.row0, L.row_step, L.row_ids, L.table_rows, L.partials);
  else
    hipLaunchKernelGGL((fcp_table_digest_kernel<A, G, false>), dim3(L.blocks), dim3(FCP_BLOCK_THREADS), 0, s, L.base, L.count, L.rb, L.salt,
                       L.row0, L.row_step, L.row_ids, L.table_rows, L.partials);
}

// Both entries behind their argument checks.  by_id: row_ids names `count` rows of the table at `base`; else `count` rows
// lie back to back from `base`.
int digest_entry(const char *who, const void *base, int32_t kind, int32_t dim, int64_t count, int64_t row0, int64_t row_step,
                 const int64_t *row_ids, int64_t table_rows, fcp_table_digest_t *out, void *workspace, int32_t device, void *stream) {
  DigestLaunch L;
  L.base = static_cast<const char *>(base);
  L.count = count;
  const int64_t rb = fcpf::row_bytes(kind, dim); // (below 2^31: the argument checks)
  L.rb = (int32_t)rb;
  L.salt = fcpd::salt_of(kind, dim);
  L.row0 = (uint64_t)row0;
  L.row_step = (uint64_t)row_step;
  L.row_ids = row_ids;
  L.table_rows = (uint64_t)table_rows;
  L.partials = static_cast<DigestPartial *>(workspace);
  const int g = fcpg::group_of_words((rb + 7) / 8);
  L.blocks = (int)fcpg::lone_blocks(count, g);
  const int a = fcpg::align_of(base, rb); // what is known of every row's address
  return on_device(who, device, stream, [&](hipStream_t s) {
    if (L.blocks > 0)
      with_one_of<8, 4, 2, 1>(a, [&](auto al) {
        with_group(g, [&](auto gg) { launch_ag<decltype(al)::value, decltype(gg)::value>(L, s); });
      });
    hipLaunchKernelGGL(fcp_table_digest_fold_kernel, dim3(1), dim3(64), 0, s, L.partials, (int32_t)L.blocks, out);
  });
}

} // namespace

extern "C" int64_t fcp_table_digest_workspace_bytes(void) { return (int64_t)kDigestBlocks * (int64_t)sizeof(DigestPartial); }

extern "C" int fcp_table_digest(const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step,
                                fcp_table_digest_t *out, void *workspace, int32_t device, void *stream) {
  std::string why;
  const int rc = fcpd::check_digest(first_row, kind, rows, dim, row0, row_step, out, workspace, &why);
  if (rc) return fail(rc, why);
  return digest_entry("fcp_table_digest", first_row, kind, dim, rows, row0, row_step, nullptr, 0, out, workspace, device, stream);
}

extern "C" int fcp_table_digest_rows(const void *table, int32_t kind, int64_t table_rows, int32_t dim, int64_t row0, int64_t row_step,
                                     const int64_t *row_ids, int64_t n, fcp_table_digest_t *out, void *workspace, int32_t device,
                                     void *stream) {
  std::string why;
  const int rc = fcpd::check_digest_rows(table, kind, table_rows, dim, row0, row_step, row_ids, n, out, workspace, &why);
  if (rc) return fail(rc, why);
  // (n > 0: row_ids is not null, which is what selects the by-id kernels)
  return digest_entry("fcp_table_digest_rows", table, kind, dim, n, row0, row_step, row_ids, table_rows, out, workspace, device, stream);
}
