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
//   * the kernel arguments are 15 separate dwords (FcpPlainLaunch), preloaded into SGPRs where the loader supports it;
//   * one id load per (column, row) pair, 4 or 8 bytes, in a loop of as many passes as the span has pairs;
//   * the conversion for the three id kinds only: a range check on the whole 64-bit id, bucketize_arith, pre-scaled
//     32-bit slot offsets parked in LDS.
// Same bits out as the generic kernel, same bad-id counts (a column that straddles two spans is counted by the block that
// holds its first slot).
#include "fcp_fused_bodies.h"

namespace {

template <int R> struct PlainLds {
  static constexpr int RB = FCP_WAVES_PER_BLOCK * R; // rows per block
  static constexpr int IDS = RB + 1;                 // padded row of the offset tile (LDS banks)
  static constexpr int REC = sizeof(FcpPlainSpan) + FCP_WAVE * sizeof(FcpPlainCol);
  alignas(16) char rec[REC];
  uint32_t off[FCP_WAVE * IDS];
};
static_assert(sizeof(FcpPlainCol) == 48 && sizeof(FcpPlainSpan) == 80, "span records: 80-byte head, 48-byte columns");

// an int64 id of the blob: 4-byte aligned only (ConcatInputs packs tensors back to back), read with one 8-byte load
typedef uint32_t __attribute__((ext_vector_type(2))) U2;
typedef U2 __attribute__((aligned(4))) Id64;

template <int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
fcp_dense_kernel_plain(const char *img, const char *blob, float *out, unsigned long long *bad_ids, int rows, int nslots,
                       int nsp8, int nlist, int img_stride, int out_stride, int policy) {
  constexpr int V = 4, RB = PlainLds<R>::RB, IDS = PlainLds<R>::IDS;
  __shared__ PlainLds<R> S;
  const int tid = threadIdx.x;
  const int lane = tid & (FCP_WAVE - 1);
  const int wave = tid >> 6;

  // the block mapping of locate_block (one group, every span listed in order): blocks with equal (bid & 7) share an XCD
  // and are given the same spans
  const int bid = blockIdx.x;
  int idx, tile;
  if (nsp8 > 0) {
    const int xcd = bid & 7, j8 = bid >> 3;
    idx = (j8 % nsp8) * 8 + xcd;
    tile = j8 / nsp8;
  } else {
    idx = bid % (-nsp8);
    tile = bid / (-nsp8);
  }
  if (idx >= nlist) return; // uniform: whole block leaves
  const int q0 = idx * FCP_WAVE, row_blk = tile * RB;
  if (q0 >= nslots || row_blk >= rows) return;

  // ---- phase 0: the span's record -> LDS, 16 bytes per thread ----------------------------------------------------------
  typedef uint32_t __attribute__((ext_vector_type(4))) U4;
  {
    const FCP_GLOBAL U4 *g = as_global(reinterpret_cast<const U4 *>(img + (int64_t)idx * img_stride));
    if (tid < (img_stride >> 4)) reinterpret_cast<U4 *>(S.rec)[tid] = g[tid];
  }
  __syncthreads();
  const FcpPlainSpan &H = *reinterpret_cast<const FcpPlainSpan *>(S.rec);
  const FcpPlainCol *cols = reinterpret_cast<const FcpPlainCol *>(S.rec + sizeof(FcpPlainSpan));

  // ---- phase 1: one thread per (column, row) pair: id -> table slot offset in LDS --------------------------------------
  // consecutive threads take consecutive rows of one column: every id cache line is requested once
  const int npairs = H.ncols * RB;
  for (int p = tid; p < npairs; p += FCP_BLOCK_THREADS) {
    const int j = p / RB, r = p % RB;
    const int b = row_blk + r;
    uint32_t off = kNoRow;
    if (b < rows) {
      const FcpPlainCol &c = cols[j];
      const char *a = blob + c.ids_off;
      const uint32_t kind = c.kind;
      int64_t id;
      if (kind == FCP_IDS_I64) {
        const Id64 w = ((const FCP_GLOBAL Id64 *)a)[b];
        id = (int64_t)(((uint64_t)w.y << 32) | w.x);
      } else {
        const uint32_t w = *as_global(reinterpret_cast<const uint32_t *>(a) + b);
        id = kind == FCP_IDS_F32_BUCKETIZE ? (int64_t)bucketize_arith(c.n_boundaries, c.bnd_b0, c.bnd_inv, c.bnd_step, __uint_as_float(w))
                                           : (int64_t)(int32_t)w;
      }
      // ids outside [0, vocab) read as zeros: the whole 64-bit id is compared (2^32 + 5 is not row 5)
      const bool bad = (uint64_t)id >= (uint64_t)c.vocab;
      off = bad ? kBadRow : (uint32_t)id * c.spr; // every table of the plan has < 2^32 - 3 slots: pre-scaled
      // a column that straddles two spans is staged by two blocks: the one holding its first slot counts
      if (bad && bad_ids && c.out_off >= q0 * V) atomicAdd(bad_ids, 1ull);
    }
    S.off[j * IDS + r] = off;
  }
  __syncthreads();
  const int q = q0 + lane;
  if (q >= nslots) return;

  // ---- phase 2: R table reads in flight per lane, then R coalesced stores (dense_body's) ------------------------------
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
    if (b < rows) st_out<V>(outp + (int64_t)b * out_stride, v[r], policy);
  }
}

} // namespace

// the request's stop event / any-order flag, as the other fused launches take them
int fcp_launch_dense_plain(const FcpPlainLaunch &P, int grid_blocks, ihipStream_t *s) {
  if (grid_blocks <= 0) return 0;
  if (P.img_stride <= 0 || (P.img_stride & 15) || P.img_stride > PlainLds<4>::REC) return (int)hipErrorInvalidValue;
  void *stop = nullptr;
  int flags = 0;
  fcp_take_launch_extras(&stop, &flags);
  const dim3 grid(grid_blocks), block(FCP_BLOCK_THREADS);
  if (stop || flags)
    hipExtLaunchKernelGGL(fcp_dense_kernel_plain<4>, grid, block, 0, s, nullptr, static_cast<hipEvent_t>(stop), flags, P.img, P.blob,
                          P.out, P.bad_ids, P.rows, P.nslots, P.nsp8, P.nlist, P.img_stride, P.out_stride, P.store_policy);
  else
    hipLaunchKernelGGL(fcp_dense_kernel_plain<4>, grid, block, 0, s, P.img, P.blob, P.out, P.bad_ids, P.rows, P.nslots, P.nsp8,
                       P.nlist, P.img_stride, P.out_stride, P.store_policy);
  return (int)hipGetLastError();
}
