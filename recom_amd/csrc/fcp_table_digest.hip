// fcp_table_digest.hip — fcp_table_digest / fcp_table_digest_rows / fcp_table_digest_workspace_bytes: an order-free 64-bit sum
// of row hashes over a table in any of the formats the plans read (FCP_TAB_F32 / _BF16 / _F16 / _Q8), computed where the table
// lies.  What fcp_table_convert, fcp_table_update_rows and a loader promise is BYTES; this is how a deployment checks them on
// the table it serves.  The value model is fcp_table_digest.h's (shared with fcp_table_digest_host.cc): a row is its bytes as
// little-endian 64-bit words, the last one zero-padded; H(r) = mix(salt + (r + 1) * G + sum_j mix(w[j] ^ (j + 1) * G)); the
// digest is the sum of H over the rows, modulo 2^64.  The reference reads float32 tables only and has no counterpart.
//
//   fcp_table_digest_kernel<A, G, BY_ID>   the grid of fcp_table_audit_kernel: kDigestBlocks blocks of FCP_BLOCK_THREADS, fewer
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

#include "fcp_table_walk.h" // with_group, with_one_of: the host's dispatch
#include "fcp_block_fold.h" // wave_fold, block_fold: the fold of a lane's record into the block's

namespace {

using fcpd::row_hash;
using fcpd::word_term;

constexpr int kDigestBlocks = 2048; // the fixed grid: 8 blocks of 256 threads on each of 256 CUs; also the records of the workspace
constexpr int kUnroll = 4;          // rows of a group per step of the walk

// What a lane, a wave, a block and the whole call have summed.  32 bytes, 8-byte aligned.
struct DigestPartial {
  uint64_t sum;
  int64_t rows, skipped, pad;
};
static_assert(sizeof(DigestPartial) == 32, "the workspace is kDigestBlocks records of 32 bytes");
static_assert(sizeof(fcp_table_digest_t) == 32, "fcp_table_digest_t is 32 bytes");

// loads of 8, 4 and 2 bytes from an address that is A-byte aligned (A-aligned for the narrower ones as far as they need it)
template <int A> struct Loads;
template <> struct Loads<8> {
  typedef uint64_t U64;
  typedef uint32_t U32;
  typedef uint16_t U16;
};
template <> struct Loads<4> {
  typedef uint64_t U64 __attribute__((aligned(4)));
  typedef uint32_t U32;
  typedef uint16_t U16;
};
template <> struct Loads<2> {
  typedef uint64_t U64 __attribute__((aligned(2)));
  typedef uint32_t U32 __attribute__((aligned(2)));
  typedef uint16_t U16;
};
template <> struct Loads<1> {
  typedef uint64_t U64 __attribute__((aligned(1)));
  typedef uint32_t U32 __attribute__((aligned(1)));
  typedef uint16_t U16 __attribute__((aligned(1)));
};

// word j of the row at `row`: a whole word for j < full, else the row's last rem = 1 .. 7 bytes, zero-padded.  The tail
// starts 8 * full bytes into the row, as aligned as the row; its pieces lie at offsets 0, 4 and 6 at the most.
template <int A> __device__ __forceinline__ uint64_t ld_row_word(const char *row, int j, int full, int rem) {
  const char *p = row + 8 * (int64_t)j;
  if (j < full) return *(const FCP_GLOBAL typename Loads<A>::U64 *)(p);
  uint64_t w = 0;
  int at = 0;
  if (rem & 4) {
    w = *(const FCP_GLOBAL typename Loads<A>::U32 *)(p);
    at = 4;
  }
  if (rem & 2) {
    w |= (uint64_t) * (const FCP_GLOBAL typename Loads<A>::U16 *)(p + at) << (8 * at);
    at += 2;
  }
  if (rem & 1) w |= (uint64_t) * (const FCP_GLOBAL uint8_t *)(p + at) << (8 * at);
  return w;
}

__device__ __forceinline__ void fold(DigestPartial &a, const DigestPartial &b) {
  a.sum += b.sum;
  a.rows += b.rows;
  a.skipped += b.skipped;
}

// base: the first row (BY_ID: the table's base); count: rows (BY_ID: ids), < 2^32 - 3; rb: bytes of a row.  Block =
// 256 / G rows per step; a group never straddles a wave, and it is live or not as a whole.  Every thread of a block takes
// the same number of steps.  The instantiations without BY_ID never read row_ids or table_rows.
template <int A, int G, bool BY_ID>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_table_digest_kernel(const char *base, int64_t count, int32_t rb, uint64_t salt, uint64_t row0, uint64_t row_step,
                            const int64_t *row_ids, uint64_t table_rows, DigestPartial *partials) {
  constexpr int kRowsPerBlock = FCP_BLOCK_THREADS / G;
  const int tid = threadIdx.x;
  const int lane = tid & (G - 1);
  const int full = rb >> 3, rem = rb & 7;
  const int nw = full + (rem != 0);
  const int64_t stride = (int64_t)gridDim.x * kRowsPerBlock;
  uint64_t sum = 0;
  int64_t nrows = 0, nskipped = 0;
  for (int64_t first = (int64_t)blockIdx.x * kRowsPerBlock; first < count; first += stride * kUnroll) {
    uint64_t id[kUnroll], w[kUnroll], w2[kUnroll];
    bool have[kUnroll], live[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = first + u * stride + tid / G;
      have[u] = i < count;
      if constexpr (BY_ID) {
        id[u] = have[u] ? (uint64_t) * as_global(row_ids + i) : ~0ull; // the whole group: one address
        live[u] = have[u] && id[u] < table_rows;
      } else {
        id[u] = (uint64_t)i;
        live[u] = have[u];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      w[u] = w2[u] = 0;
      if (live[u] && lane < nw) w[u] = ld_row_word<A>(base + id[u] * (uint64_t)rb, lane, full, rem);
      if (live[u] && lane + G < nw) w2[u] = ld_row_word<A>(base + id[u] * (uint64_t)rb, lane + G, full, rem);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      uint64_t t = (live[u] && lane < nw) ? word_term(w[u], (uint64_t)lane) : 0;
      if (live[u] && lane + G < nw) t += word_term(w2[u], (uint64_t)(lane + G));
      if constexpr (G == 64) {
        if (live[u])
          for (int j = lane + 128; j < nw; j += 64) t += word_term(ld_row_word<A>(base + id[u] * (uint64_t)rb, j, full, rem), (uint64_t)j);
      }
#pragma unroll
      for (int m = G / 2; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
      if (lane == 0) {
        if (live[u]) {
          sum += row_hash(salt, row0 + id[u] * row_step, t);
          ++nrows;
        } else if (have[u]) {
          ++nskipped;
        }
      }
    }
  }

  block_fold(DigestPartial{sum, nrows, nskipped, 0}, partials);
}

// one wave; n: records of the workspace the first kernel wrote (0: it was not launched)
__global__ void __launch_bounds__(64) fcp_table_digest_fold_kernel(const DigestPartial *partials, int32_t n, fcp_table_digest_t *out) {
  const int lane = threadIdx.x;
  DigestPartial p = {0, 0, 0, 0};
  for (int i = lane; i < n; i += 64) fold(p, partials[i]);
  wave_fold(p);
  if (lane != 0) return;
  fcp_table_digest_t r;
  r.sum = p.sum;
  r.rows = p.rows;
  r.skipped = p.skipped;
  r.reserved = 0;
  *out = r;
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

// G, the lanes that share a row: the largest power of two that is not above the row's words, at most 64 — a row of 9 words
// (q8, dim 64) takes 8 lanes and two words in its first lane, not 16 lanes of which 7 idle
int group_of_words(int64_t nw) {
  int g = 1;
  while (2 * g <= nw && g < 64) g <<= 1;
  return g;
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
  const int g = group_of_words((rb + 7) / 8);
  const int64_t rows_per_block = FCP_BLOCK_THREADS / g;
  L.blocks = (int)std::min<int64_t>(kDigestBlocks, (count + rows_per_block - 1) / rows_per_block);
  // what is known of every row's address: the base's low bits and the row bytes' (a q8 table of dim % 8 == 0 at an
  // allocation's start takes the aligned loads)
  const uintptr_t bits = (uintptr_t)base | (uintptr_t)rb | 8u;
  const int a = (int)(bits & (~bits + 1));
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
