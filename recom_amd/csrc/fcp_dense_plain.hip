// fcp_dense_plain.hip — the dense kernel of PLAIN dense plans (fcp_plan::plain_dense): float32 concat output, one group,
// unsharded, V = 4, every column a gather by int32 ids, int64 ids or float32 values bucketized by reproducible boundaries,
// no id transform, no table of 2^32 - 3 slots or more — BASELINE.json's S2.  At least 64 rows per request (R = 4).
//
// A translation unit of its own, for the reason fcp_weighted.hip and fcp_narrow.hip are: the tuned instantiations of
// fcp_kernels.hip stay the code they are, and a plan that does not qualify never sees this file.
//
// Geometry, grid, block mapping and phase 2 are the generic dense kernel's (dense_body, fcp_fused_bodies.h): a block owns
// one 64-slot span for 16 rows.  What differs is the block's front, which the generic body pays for every form, id
// source, bucketize tier, id transform, shard and 64-bit row path:
//   * ONE coalesced read of the span's record of the per-span image (FcpPlainSpan + FcpPlainCol[], fcp_internal.h) into
//     LDS instead of kernarg -> slot map -> static + dynamic column records;
//   * the kernel arguments are 16 separate dwords (FcpPlainLaunch), the first 14 preloaded into SGPRs where the loader
//     supports it (the last two are bad_ids, wanted on a bad id only);
//   * the partial last group of eight spans is dealt evenly over the XCDs (fcp_plain_map.h); the grid is unchanged;
//   * the ids of the (column, row) pairs asked for BEFORE the record has arrived: all a pair thread needs first is its
//     column's id fact (one dword: where the id stream starts, 4 or 8 bytes per id), and the four facts of a wave's
//     columns are one 16-byte scalar load; the record goes to LDS, and the block meets its first barrier, behind the
//     id loads; a loop of as many passes as the span has pairs;
//   * the conversion for the three id kinds only: a range check on the whole 64-bit id, bucketize_arith, pre-scaled
//     32-bit slot offsets parked in LDS.
// Phase 2 has one store form more than st_out's three: write-through without the streaming hint (st_through_alloc below),
// which store_policy_for hands to this kernel for large outputs into a reused arena (S2 25.57 -> 24.35 us).
// Same bits out as the generic kernel, same bad-id counts (a column that straddles two spans is counted by the block that
// holds its first slot).
#include "fcp_fused_bodies.h"
#include "fcp_plain_map.h"

namespace {

template <int R> struct PlainLds {
  static constexpr int RB = FCP_WAVES_PER_BLOCK * R; // rows per block
  static constexpr int IDS = RB + 1;                 // padded row of the offset tile (LDS banks)
  static constexpr int REC = FCP_PLAIN_FACTS_OFF + fcp_plain_facts_bytes(FCP_WAVE) + FCP_WAVE * sizeof(FcpPlainCol);
  alignas(16) char rec[REC];
  uint32_t off[FCP_WAVE * IDS];
};
static_assert(sizeof(FcpPlainCol) == 48 && sizeof(FcpPlainSpan) == FCP_PLAIN_FACTS_OFF && FCP_PLAIN_FACTS_OFF % 16 == 0 &&
                  fcp_plain_facts_bytes(1) == 64 && fcp_plain_facts_bytes(FCP_WAVE) == 256,
              "span records: 80-byte head, id facts in whole passes of 16 dwords, 48-byte columns");
static_assert(FCP_BLOCK_THREADS / (FCP_WAVES_PER_BLOCK * 4) == FCP_PLAIN_FACTS_PER_PASS && FCP_WAVE / (FCP_WAVES_PER_BLOCK * 4) == 4,
              "R = 4: a pass of the pair loop covers 16 columns, a wave four");
static_assert(PlainLds<4>::REC / 16 <= FCP_BLOCK_THREADS, "one 16-byte piece of the record per thread");

// an int64 id of the blob: 4-byte aligned only (ConcatInputs packs tensors back to back), read with one 8-byte load
typedef uint32_t __attribute__((ext_vector_type(2))) U2;
typedef U2 __attribute__((aligned(4))) Id64;

// Fourth output-store form, this kernel's alone: write-through WITHOUT the streaming hint (`sc1`: the line leaves the XCD's
// L2 at once, as under `sc1 nt`, and allocates as a plain store does).  FcpPlainLaunch::store_policy bit 3
// (FCP_ST_THROUGH_ALLOC); the other three forms are st_out's (fcp_fused_bodies.h), untouched.  Inline asm ending in
// s_nop 1, for st_through's reasons.  Measured in profiles/dense_plain_store_sc1_ab.txt.
__device__ __forceinline__ void st_through_alloc(FCP_GLOBAL VecType<4>::T *p, VecType<4>::T t) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_out_plain(float *p, const VF<4> &v, int policy) {
  if (policy & FCP_ST_THROUGH_ALLOC) {
    VecType<4>::T t;
    __builtin_memcpy(&t, &v, sizeof(t));
    st_through_alloc(as_global(reinterpret_cast<VecType<4>::T *>(p)), t);
    return;
  }
  st_out<4>(p, v, policy);
}

template <int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
fcp_dense_kernel_plain(const char *img, const char *blob, float *out, int rows, int nslots, int nsp8, int nlist, int img_stride,
                       int deal_tiles, int out_stride, int policy, unsigned long long *bad_ids) {
  constexpr int V = 4, RB = PlainLds<R>::RB, IDS = PlainLds<R>::IDS;
  __shared__ PlainLds<R> S;
  const int tid = threadIdx.x;
  const int lane = tid & (FCP_WAVE - 1);
  const int wave = tid >> 6;

  // the block mapping (fcp_plain_map.h): locate_block's, but for the partial last group of eight spans, whose (span, row
  // tile) pairs are dealt evenly over the eight XCDs when deal_tiles is the grid's number of row tiles (0: locate_block's)
  int idx, tile;
  if (!fcp_plain_locate(blockIdx.x, nsp8, nlist, deal_tiles, idx, tile)) return; // uniform: whole block leaves
  const int q0 = idx * FCP_WAVE, row_blk = tile * RB;
  if (q0 >= nslots || row_blk >= rows) return;

  // ---- the front: id facts by a scalar load, the record by a vector load, the id loads of the first pass behind the facts ----
  // A wave's 64 pair threads cover four consecutive columns of the span (RB = 16): their id facts are one aligned 16-byte
  // group at a wave-uniform address, asked for through the scalar cache while the record is still in flight.
  typedef uint32_t __attribute__((ext_vector_type(4))) U4;
  const char *rec = img + (int64_t)idx * img_stride;
  const FCP_CONST U4 *facts = (const FCP_CONST U4 *)(rec + FCP_PLAIN_FACTS_OFF) + __builtin_amdgcn_readfirstlane(wave);
  const U4 f0 = *facts;
  const bool rec_thread = tid < (img_stride >> 4);
  U4 rec_regs = {0, 0, 0, 0};
  if (rec_thread) rec_regs = as_global(reinterpret_cast<const U4 *>(rec))[tid];

  const int r = tid % RB, b = row_blk + r; // the thread's row, the same in every pass
  const int sub = lane / RB;               // which of the wave's four columns
  const int bc = b < rows ? b : rows - 1;  // (a row past the request reads the last row's id and parks kNoRow)
  // The id of pair (column of `fact`, row b), asked for in straight-line code: two dword loads by every lane, the second
  // one of the id's high half (int64) or of the same dword again.  A load under a branch on the id kind would make the
  // wait for the record, which was asked for earlier, a wait for every load in flight.  A padding fact reads the blob's
  // first stream (offset 0: at least `rows` dwords) and parks nothing.
  auto load_id = [&](U4 f, uint32_t &kind) -> U2 {
    const uint32_t lo2 = (sub & 1) ? f.y : f.x, hi2 = (sub & 1) ? f.w : f.z;
    const uint32_t fact = (sub & 2) ? hi2 : lo2;
    kind = b < rows ? fact >> 30 : FCP_PLAIN_FACT_NONE;
    const bool wide = (fact >> 30) == FCP_PLAIN_FACT_I64;
    const FCP_GLOBAL uint32_t *a = as_global(reinterpret_cast<const uint32_t *>(blob + ((uint64_t)(fact & 0x3FFFFFFFu) << 2))) + (wide ? 2 * bc : bc);
    U2 w;
    w.x = a[0];
    w.y = a[wide ? 1 : 0];
    return w;
  };
  uint32_t kind;
  U2 w = load_id(f0, kind);
  if (rec_thread) reinterpret_cast<U4 *>(S.rec)[tid] = rec_regs;
  __syncthreads();
  const FcpPlainSpan &H = *reinterpret_cast<const FcpPlainSpan *>(S.rec);
  const FcpPlainCol *cols = reinterpret_cast<const FcpPlainCol *>(S.rec + H.cols_off);

  // ---- phase 1: one thread per (column, row) pair: id -> table slot offset in LDS --------------------------------------
  // consecutive threads take consecutive rows of one column: every id cache line is requested once
  const int ncols = H.ncols;
  for (int j = tid / RB;;) {
    if (j < ncols) {
      uint32_t off = kNoRow;
      if (kind != FCP_PLAIN_FACT_NONE) {
        const FcpPlainCol &c = cols[j];
        int64_t id;
        if (kind == FCP_PLAIN_FACT_I64)
          id = (int64_t)(((uint64_t)w.y << 32) | w.x);
        else
          id = kind == FCP_PLAIN_FACT_F32 ? (int64_t)bucketize_arith(c.n_boundaries, c.bnd_b0, c.bnd_inv, c.bnd_step, __uint_as_float(w.x))
                                          : (int64_t)(int32_t)w.x;
        // ids outside [0, vocab) read as zeros: the whole 64-bit id is compared (2^32 + 5 is not row 5)
        const bool bad = (uint64_t)id >= (uint64_t)c.vocab;
        off = bad ? kBadRow : (uint32_t)id * c.spr; // every table of the plan has < 2^32 - 3 slots: pre-scaled
        // a column that straddles two spans is staged by two blocks: the one holding its first slot counts
        if (bad && bad_ids && c.out_off >= q0 * V) atomicAdd(bad_ids, 1ull);
      }
      S.off[j * IDS + r] = off;
    }
    // further passes (spans of more than 16 columns): the wave's next four facts, then its ids
    j += FCP_PLAIN_FACTS_PER_PASS;
    if (j - sub >= ncols) break; // wave-uniform: j - sub is the wave's first column of the pass
    facts += FCP_BLOCK_THREADS / FCP_WAVE;
    w = load_id(*facts, kind);
  }
  __syncthreads();
  const int q = q0 + lane;
  if (q >= nslots) return;

  // ---- phase 2: R table reads in flight per lane, then R coalesced stores (dense_body's, and a fourth store form) -----
  const int j = H.lane_col[lane];
  const float *tb = cols[j].table + (q * V - cols[j].out_off);
  float *outp = out + q * V;
  const int r0 = wave * R;
  uint32_t off[R];
#pragma unroll
  for (int r = 0; r < R; ++r) off[r] = S.off[j * IDS + r0 + r];
  VF<V> v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    v[r] = vzero<V>();
    if (is_row(off[r])) v[r] = ld_slot32<V>(tb, off[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int b = row_blk + r0 + r;
    if (b < rows) st_out_plain(outp + (int64_t)b * out_stride, v[r], policy);
  }
}

} // namespace

// the request's stop event / any-order flag, as the other fused launches take them
int fcp_launch_dense_plain(const FcpPlainLaunch &P, int grid_blocks, ihipStream_t *s) {
  if (grid_blocks <= 0) return 0;
  // (a record has the head, at least one pass of id facts and one column: every wave's first scalar load stays inside it)
  if (P.img_stride < FCP_PLAIN_FACTS_OFF + fcp_plain_facts_bytes(1) + (int)sizeof(FcpPlainCol) || (P.img_stride & 15) ||
      P.img_stride > PlainLds<4>::REC)
    return (int)hipErrorInvalidValue;
  void *stop = nullptr;
  int flags = 0;
  fcp_take_launch_extras(&stop, &flags);
  const dim3 grid(grid_blocks), block(FCP_BLOCK_THREADS);
  if (stop || flags)
    hipExtLaunchKernelGGL(fcp_dense_kernel_plain<4>, grid, block, 0, s, nullptr, static_cast<hipEvent_t>(stop), flags, P.img, P.blob,
                          P.out, P.rows, P.nslots, P.nsp8, P.nlist, P.img_stride, P.deal_tiles, P.out_stride, P.store_policy, P.bad_ids);
  else
    hipLaunchKernelGGL(fcp_dense_kernel_plain<4>, grid, block, 0, s, P.img, P.blob, P.out, P.rows, P.nslots, P.nsp8, P.nlist,
                       P.img_stride, P.deal_tiles, P.out_stride, P.store_policy, P.bad_ids);
  return (int)hipGetLastError();
}
