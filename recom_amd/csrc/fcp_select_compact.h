// fcp_select_compact.h — what the selecting units share: fcp_table_delta.hip and fcp_table_diff.hip end in "the positions that
// satisfy X, ascending, padded with -1", found by the same three phases over a fixed grid, and that tail is written here ONCE.
//   classify   the unit's own kernel(s): select_grid(n) blocks, block b owns the contiguous chunk [b * chunk, (b + 1) * chunk)
//              of positions.  One flag byte per position (1: selected), ONE record per block by block_fold (fcp_block_fold.h).
//   fold       the unit's own one-wave kernel: its lanes sum their records' fields, select_offsets turns the selected counts
//              into exclusive offsets; the unit then writes the totals record at partials[Blocks] and its report.
//   compact    the unit's own kernel <V, G> around select_compact, the classify grid again: selected position number k of the
//              call, in ascending position, goes to the unit's emit, every i >= m (the indices no selected position has) to
//              its tail; V > 0: the selected float32 rows are copied as bits, rows[i_k] -> rows_out[k].
// Launch boundaries order the phases; no block ever waits for another.  The units keep their __global__ kernels and argument
// structs, their records and what they count, what an output index receives, the report.  Unnamed namespace, as fcp_block_fold.h.
// A RECORD IS 32 BYTES, THE SELECTED COUNT ITS FIRST FIELD AND `offset` ITS LAST, both int64_t; the workspace holds Blocks + 1.
#pragma once
#include "fcp_fused_bodies.h"
#include "fcp_table_walk.h" // group_of, with_vec, with_group

#include <cstddef>
#include <type_traits>

namespace {

constexpr int kSelectTile = FCP_BLOCK_THREADS; // positions of one step of a compact block; a chunk is whole tiles
static_assert(kSelectTile == 256, "four waves per block: the compact body's scan of wave counts");

// The classify / compact grid of n positions: chunks of whole tiles, at least min_tiles of them, at most max_blocks chunks.
struct SelectGrid { int64_t chunk; int nblocks; };
inline SelectGrid select_grid(int64_t n, int max_blocks, int min_tiles) {
  const int64_t tiles = (n + kSelectTile - 1) / kSelectTile;
  const int64_t chunk = std::max<int64_t>(min_tiles, (tiles + max_blocks - 1) / max_blocks) * kSelectTile;
  return SelectGrid{chunk, (int)((n + chunk - 1) / chunk)};
}

template <class P> __device__ __forceinline__ int64_t selected_of(const P &p) {
  static_assert(std::is_standard_layout<P>::value && sizeof(P) == 32 && offsetof(P, offset) == 24, "a record: the count first, offset last");
  return *reinterpret_cast<const int64_t *>(&p);
}

// The fold kernel's wave: lane l owns the records [l * per, (l + 1) * per) of the nblocks the classify phase wrote and has
// summed their selected counts into `mine`; offset of record b = the selected counts of the records before it.
template <int Blocks, class P> __device__ __forceinline__ void select_offsets(P *partials, int nblocks, int64_t mine) {
  static_assert(Blocks % 64 == 0, "the fold's lanes own equal runs of records");
  constexpr int per = Blocks / 64;
  const int lane = threadIdx.x;
  const int b0 = lane * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  int64_t before = mine; // inclusive scan of the lanes' counts, then made exclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t up = __shfl_up(before, d, 64);
    if (lane >= d) before += up;
  }
  before -= mine;
  for (int b = b0; b < b1; ++b) {
    partials[b].offset = before;
    before += selected_of(partials[b]);
  }
}

// The run-time form, for a fold whose wave serves an entry of a grouped call (fcp_tables_delta.hip): `per` records per lane, any
// per with 64 * per >= nblocks, where the template form takes Blocks / 64.
template <class P> __device__ __forceinline__ void select_offsets_n(P *partials, int nblocks, int per, int64_t mine) {
  const int lane = threadIdx.x & 63;
  const int b0 = lane * per < nblocks ? lane * per : nblocks, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  int64_t before = mine; // inclusive scan of the lanes' counts, then made exclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t up = __shfl_up(before, d, 64);
    if (lane >= d) before += up;
  }
  before -= mine;
  for (int b = b0; b < b1; ++b) {
    partials[b].offset = before;
    before += selected_of(partials[b]);
  }
}

// V 32-bit words as one load / store at the rows' alignment 4 * V
template <int V> struct Words;
template <> struct Words<4> { typedef uint32_t __attribute__((ext_vector_type(4))) T; };
template <> struct Words<2> { typedef uint32_t __attribute__((ext_vector_type(2))) T; };
template <> struct Words<1> { typedef uint32_t T; };

// One block of the grid; EVERY thread of a block of kSelectTile calls it and reaches its three barriers per tile (two without
// rows).  n, chunk: the grid's; partials: behind the fold.  V == 0: rows and rows_out are never read; else groups of G lanes
// copy a row, V words per load and store (integer vectors).  LDS: 1 KiB + 16 bytes.  The unit's hook h:
//   h.prepare(i, have)   what position i brings along (have: it lies in the chunk), asked for BEFORE the ballot: a load it
//                        issues is in flight across the first barrier
//   h.emit(k, i, p)      selected position i is number k of the call; p: what prepare returned.  h.tail(i): i >= m
template <int V, int G, int Blocks, class P, class H>
__device__ __forceinline__ void select_compact(const uint8_t *flags, const P *partials, int64_t n, int64_t chunk, const float *rows,
                                               float *rows_out, int32_t dim, const H &h) {
  __shared__ uint32_t s_list[kSelectTile]; // the tile's selected positions, by rank: their thread
  __shared__ uint32_t s_count[kSelectTile / 64];
  const int tid = threadIdx.x;
  const int wave = tid / 64;
  const int64_t c0 = (int64_t)blockIdx.x * chunk;
  const int64_t c1 = c0 + chunk < n ? c0 + chunk : n;
  const int64_t m = selected_of(partials[Blocks]);
  int64_t k0 = partials[blockIdx.x].offset; // the output index of the tile's first selected position
  for (int64_t t0 = c0; t0 < c1; t0 += kSelectTile) {
    const int64_t i = t0 + tid;
    const bool have = i < c1;
    const bool hit = have && *as_global(flags + i) != 0;
    const auto brought = h.prepare(i, have);
    const unsigned long long ballot = __ballot(hit);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
    if ((tid & 63) == 0) s_count[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t rank = below, total = 0;
#pragma unroll
    for (int w = 0; w < kSelectTile / 64; ++w) {
      const uint32_t c = s_count[w];
      if (w < wave) rank += c;
      total += c;
    }
    if (hit) {
      h.emit(k0 + rank, i, brought);
      if constexpr (V > 0) s_list[rank] = (uint32_t)tid;
    }
    if (have && i >= m) h.tail(i);
    __syncthreads(); // s_list is whole; s_count may be written again
    if constexpr (V > 0) {
      typedef typename Words<V>::T W;
      const int lane = tid & (G - 1);
      const int nslots = dim / V;
      for (uint32_t j = (uint32_t)(tid / G); j < total; j += kSelectTile / G) {
        const FCP_GLOBAL W *src = as_global(reinterpret_cast<const W *>(rows + (t0 + (int64_t)s_list[j]) * dim));
        FCP_GLOBAL W *dst = as_global(reinterpret_cast<W *>(rows_out + (k0 + (int64_t)j) * dim));
        for (int slot = lane; slot < nslots; slot += G) dst[slot] = src[slot];
      }
      __syncthreads(); // the copies have read s_list
    }
    k0 += total;
  }
}

// The run-time form, for a block that serves an entry of a grouped call (fcp_tables_delta.hip): `block` of the entry's own
// `nblocks`, its records partials[0 .. nblocks) and its totals partials[nblocks], where the template form takes blockIdx.x and
// Blocks.  The same steps, barriers and LDS.
template <int V, int G, class P, class H>
__device__ __forceinline__ void select_compact_at(const uint8_t *flags, const P *partials, uint32_t block, uint32_t nblocks, int64_t n, int64_t chunk,
                                                  const float *rows, float *rows_out, int32_t dim, const H &h) {
  __shared__ uint32_t s_list[kSelectTile]; // the tile's selected positions, by rank: their thread
  __shared__ uint32_t s_count[kSelectTile / 64];
  const int tid = threadIdx.x;
  const int wave = tid / 64;
  const int64_t c0 = (int64_t)block * chunk;
  const int64_t c1 = c0 + chunk < n ? c0 + chunk : n;
  const int64_t m = selected_of(partials[nblocks]);
  int64_t k0 = partials[block].offset; // the output index of the tile's first selected position
  for (int64_t t0 = c0; t0 < c1; t0 += kSelectTile) {
    const int64_t i = t0 + tid;
    const bool have = i < c1;
    const bool hit = have && *as_global(flags + i) != 0;
    const auto brought = h.prepare(i, have);
    const unsigned long long ballot = __ballot(hit);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
    if ((tid & 63) == 0) s_count[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t rank = below, total = 0;
#pragma unroll
    for (int w = 0; w < kSelectTile / 64; ++w) {
      const uint32_t c = s_count[w];
      if (w < wave) rank += c;
      total += c;
    }
    if (hit) {
      h.emit(k0 + rank, i, brought);
      if constexpr (V > 0) s_list[rank] = (uint32_t)tid;
    }
    if (have && i >= m) h.tail(i);
    __syncthreads(); // s_list is whole; s_count may be written again
    if constexpr (V > 0) {
      typedef typename Words<V>::T W;
      const int lane = tid & (G - 1);
      const int nslots = dim / V;
      for (uint32_t j = (uint32_t)(tid / G); j < total; j += kSelectTile / G) {
        const FCP_GLOBAL W *src = as_global(reinterpret_cast<const W *>(rows + (t0 + (int64_t)s_list[j]) * dim));
        FCP_GLOBAL W *dst = as_global(reinterpret_cast<W *>(rows_out + (k0 + (int64_t)j) * dim));
        for (int slot = lane; slot < nslots; slot += G) dst[slot] = src[slot];
      }
      __syncthreads(); // the copies have read s_list
    }
    k0 += total;
  }
}

// The host's choice of the compact kernel: launch(V, G) as std::integral_constants, <0, 1> without rows, else the rows' V and G
template <class L> void with_compact_shape(bool with_rows, int dim, int vec, L launch) {
  if (!with_rows) return launch(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
  with_vec(vec, [&](auto v) { with_group(group_of(dim, vec), [&](auto g) { launch(v, g); }); });
}

} // namespace
