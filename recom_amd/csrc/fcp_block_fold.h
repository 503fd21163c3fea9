// fcp_block_fold.h — what the judging units share on the device: fcp_table_audit.hip, fcp_outputs_compare.hip,
// fcp_table_digest.hip and fcp_table_delta.hip end a block by folding one partial record per lane into ONE record per block,
// and a one-wave kernel folds those; fcp_table_traffic.hip and fcp_table_delta.hip put a block-level LDS table of {row, value}
// cells in front of a global one.  The fold (record_shuffled, wave_fold, block_fold, kNoSuchRow) and the table (lds_rows_clear /
// _claim / _flush, kEmptyCell, kLdsRowProbes, LdsU32) are written here ONCE.  The units keep what differs: their record
// structs with a fold(a, b) beside them (found through the record's type), nothing_seen, the final-record writers, the
// operation on a claimed cell's value and where a row goes that found no cell.  Everything lives in an unnamed namespace, as in
// fcp_table_walk.h: each translation unit gets its own copy.
//
// THE ORDER OF THE FOLD IS A CONTRACT — audit and compare sum float64 with it, and their bytes do not change while it holds:
//   wave_fold    steps m = 32, 16, 8, 4, 2, 1, each fold(p, the record of lane ^ m): every lane ends with the same record;
//   block_fold   wave_fold, one record per wave in LDS, a barrier, then thread 0 folds the records of waves 1, 2, ... in
//                ascending order ONTO ITS OWN (wave 0's) and stores the result at partials[blockIdx.x].
#pragma once
#include "fcp_fused_bodies.h"

#include <type_traits>

namespace {

constexpr uint32_t kNoSuchRow = 0xFFFFFFFFu; // rows < 2^32 - 3: a row index fits 32 bits, and this is none

// what lane ^ m holds of p, moved as 32-bit words (a field fold() never reads, padding say, costs nothing: its moves are dead)
template <class R> __device__ __forceinline__ R record_shuffled(const R &p, int m) {
  static_assert(std::is_trivially_copyable<R>::value && sizeof(R) % 4 == 0, "a record is moved as 32-bit words");
  uint32_t w[sizeof(R) / 4];
  __builtin_memcpy(w, &p, sizeof(R));
#pragma unroll
  for (size_t i = 0; i < sizeof(R) / 4; ++i) w[i] = __shfl_xor(w[i], m, 64);
  R o;
  __builtin_memcpy(&o, w, sizeof(R));
  return o;
}

// the 64 lanes of a wave into every lane
template <class R> __device__ __forceinline__ void wave_fold(R &p) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) fold(p, record_shuffled(p, m));
}

// EVERY thread of a block of FCP_BLOCK_THREADS calls it with its own record; P: what a workspace record is (R converts to it)
template <class R, class P> __device__ __forceinline__ void block_fold(R p, P *partials) {
  wave_fold(p);
  __shared__ R s_wave[FCP_BLOCK_THREADS / 64];
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) s_wave[tid / 64] = p;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < FCP_BLOCK_THREADS / 64; ++w) fold(p, s_wave[w]);
    partials[blockIdx.x] = p;
  }
}

// ... and with the record's place given: a block of a grouped launch owns a record of its ENTRY's run, not number blockIdx.x
template <class R, class P> __device__ __forceinline__ void block_fold_to(R p, P *mine) {
  wave_fold(p);
  __shared__ R s_wave[FCP_BLOCK_THREADS / 64];
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) s_wave[tid / 64] = p;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < FCP_BLOCK_THREADS / 64; ++w) fold(p, s_wave[w]);
    *mine = p;
  }
}

// ---- a block's LDS table of SLOTS {row, value} cells, SLOTS a power of two, for a block of THREADS threads.  The kernel owns
// the two __shared__ arrays.  A row's home is row mod SLOTS; it looks at kLdsRowProbes cells from there on.  A cell is claimed
// by an LDS compare-and-swap on its key; the key of a claimed cell never changes while the block runs, so a key that is read as
// another row's is another row's for good, and a relaxed load that sees a stale EMPTY only costs the compare-and-swap that
// tells the truth.  (Explicit address spaces: with generic pointers the compiler merges the LDS atomic on a claimed cell and
// the global atomic of a row without one into ONE flat atomic on either address.)
typedef __attribute__((address_space(3))) uint32_t LdsU32;
constexpr uint32_t kEmptyCell = 0xFFFFFFFFu; // a table's rows < 2^32 - 3: a row index fits 32 bits, and this is none
constexpr int kLdsRowProbes = 4;

// every cell {kEmptyCell, 0}, then the block's barrier
template <int SLOTS, int THREADS> __device__ __forceinline__ void lds_rows_clear(uint32_t *s_key, uint32_t *s_val, int tid) {
  static_assert(SLOTS > 0 && (SLOTS & (SLOTS - 1)) == 0 && SLOTS % THREADS == 0, "slot masks and the clear / flush loops");
  for (int i = tid; i < SLOTS; i += THREADS) {
    s_key[i] = kEmptyCell;
    s_val[i] = 0;
  }
  __syncthreads();
}

// the cell of row r, claimed now if r had none; -1: no cell within the probes.  The caller's own LDS atomic on the value follows
// (every claim is followed by one that leaves the value non-zero), or its own way out.
template <int SLOTS> __device__ __forceinline__ int lds_rows_claim(LdsU32 *s_key, uint32_t r) {
#pragma unroll
  for (int p = 0; p < kLdsRowProbes; ++p) {
    const uint32_t slot = (r + p) & (SLOTS - 1);
    uint32_t k = __hip_atomic_load(&s_key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == kEmptyCell) {
      uint32_t seen = kEmptyCell; // what the cell held: still empty = claimed for r
      __hip_atomic_compare_exchange_strong(&s_key[slot], &seen, r, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      k = seen == kEmptyCell ? r : seen;
    }
    if (k == r) return (int)slot;
  }
  return -1;
}

// the block's barrier, then f(row, value) per occupied cell (value != 0: the cell was claimed, its key is a row)
template <int SLOTS, int THREADS, class F> __device__ __forceinline__ void lds_rows_flush(const uint32_t *s_key, const uint32_t *s_val, int tid, F f) {
  __syncthreads();
  for (int i = tid; i < SLOTS; i += THREADS) {
    const uint32_t v = s_val[i];
    if (v != 0) f(s_key[i], v);
  }
}

} // namespace
