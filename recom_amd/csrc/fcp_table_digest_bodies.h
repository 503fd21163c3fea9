// fcp_table_digest_bodies.h — the body of the digest kernels, written ONCE for the two units that launch it:
// fcp_table_digest.hip (one table per call: the block index is blockIdx.x and the walk's stride the grid) and
// fcp_tables_digest.hip (many tables per call: both are LOCAL to the entry the block found).  `block` and `blocks` are the only
// things the two fronts hand over differently; every other argument is what the single-table kernel took.  The record a lane,
// a block and a call sum into (DigestPartial), its fold and the fold kernel's last step (write_digest) live here too.  The
// includer includes fcp_block_fold.h behind this header: block_fold and wave_fold find fold(DigestPartial &, ...) through the
// record's type.  Unnamed namespace, as in fcp_table_walk.h.  Integer code only.
#pragma once
#include "fcp_fused_bodies.h"
#include "fcp_table_digest.h"

namespace {

using fcpd::row_hash;
using fcpd::word_term;

constexpr int kUnroll = 4; // rows of a group per step of the walk

// What a lane, a wave, a block and the whole call have summed.  32 bytes, 8-byte aligned.
struct DigestPartial {
  uint64_t sum;
  int64_t rows, skipped, pad;
};
static_assert(sizeof(DigestPartial) == 32, "a workspace record is 32 bytes");
static_assert(sizeof(fcp_table_digest_t) == 32, "fcp_table_digest_t is 32 bytes");

__device__ __forceinline__ void fold(DigestPartial &a, const DigestPartial &b) {
  a.sum += b.sum;
  a.rows += b.rows;
  a.skipped += b.skipped;
}

// what a call leaves for one table: the folded record as fcp_table_digest_t
__device__ __forceinline__ void write_digest(fcp_table_digest_t *out, const DigestPartial &p) {
  fcp_table_digest_t r;
  r.sum = p.sum;
  r.rows = p.rows;
  r.skipped = p.skipped;
  r.reserved = 0;
  *out = r;
}

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

// What ONE lane of block `block` of the `blocks` blocks that share a table sums.  base: the first row (BY_ID: the table's
// base); count: rows (BY_ID: ids), < 2^32 - 3; rb: bytes of a row.  Block = 256 / G rows per step, the walk's stride is
// blocks * 256 / G rows; a group never straddles a wave, and it is live or not as a whole.  Every thread of a block takes the
// same number of steps.  The instantiations without BY_ID never read row_ids or table_rows.  EVERY thread of the block calls it
// (the butterflies), and hands the result to block_fold.
template <int A, int G, bool BY_ID>
__device__ __forceinline__ DigestPartial digest_body(const char *base, int64_t count, int32_t rb, uint64_t salt, uint64_t row0,
                                                     uint64_t row_step, const int64_t *row_ids, uint64_t table_rows, uint32_t block,
                                                     uint32_t blocks) {
  constexpr int kRowsPerBlock = FCP_BLOCK_THREADS / G;
  const int tid = threadIdx.x;
  const int lane = tid & (G - 1);
  const int full = rb >> 3, rem = rb & 7;
  const int nw = full + (rem != 0);
  const int64_t stride = (int64_t)blocks * kRowsPerBlock;
  uint64_t sum = 0;
  int64_t nrows = 0, nskipped = 0;
  for (int64_t first = (int64_t)block * kRowsPerBlock; first < count; first += stride * kUnroll) {
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
  return DigestPartial{sum, nrows, nskipped, 0};
}

} // namespace
