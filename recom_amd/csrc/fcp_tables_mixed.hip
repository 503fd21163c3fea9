// fcp_tables_mixed.hip — the fused kernels for plans whose embedding tables have MORE THAN ONE format
// (FCP_FLAG_TABLES_PER_INPUT with tables that really differ): float32, bf16, fp16 and 8-bit row-quantised tables side by side
// in one plan — big tables at 8 bits, small or quality-sensitive ones at 16 or 32, a dim-1 "wide" column never as a 9-byte q8
// row.  Plans whose tables all share one format take that format's plan-wide kernels (fcp_kernels.hip, fcp_tables16.hip,
// fcp_tables_q8.hip), never these.
//
// A translation unit of its own, for the reason the other table units are: the tuned instantiations stay the code they are.
// These are the SAME bodies (dense_body / ragged_body<..., FCP_VAR_TABMIX>, fcp_fused_bodies.h) with the same slot map, span
// lists, rows per wave, LDS layout and grids.  A span is 64 slots of the concat row, so one wave routinely holds columns of
// different formats: the kind is a fact of each COLUMN — bits 16..17 of its record's flags (FCP_F_TABKIND), staged with the
// record, no record or LDS structure grows — and a lane picks its table address, row stride and loader by it.  Where one
// ballot shows that the whole wave holds one kind, the choice is a scalar branch; the three exec-masked sections are paid
// only by waves that really mix.  9 + 3 + 9 = 21 kernels.  Unsharded, float32 output.
#include "fcp_fused_launch.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_tabmix_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, FCP_VAR_TABMIX>(L, blockIdx.x, smem);
}

// Eight waves per SIMD where the body fits 64 VGPRs.  At V = 4 it does not: fcp_ragged_kernel<4> sits at exactly 64, and the
// lane's kind next to the q8 walk's tail does not fit beside a 10-wide batch without scratch — that instantiation (and the
// hybrid ones that contain it) is left to the allocator: more registers, fewer waves, no scratch.
template <int V> constexpr int kMixMinWaves = V == 4 ? 1 : 8;

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(kMixMinWaves<V>, 8)))
fcp_ragged_tabmix_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, FCP_VAR_TABMIX>(L, blockIdx.x, smem);
}

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(kMixMinWaves<V>, 8)))
fcp_hybrid_tabmix_kernel(const FcpHybridLaunch H) {
  __shared__ __attribute__((aligned(16))) char smem[kHybridLds<R>];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, FCP_VAR_TABMIX>(H.ragged, bid, smem); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, FCP_VAR_TABMIX>(H.dense, bid - H.ragged_blocks, smem);
  }
}

} // namespace

int fcp_launch_tabmix(const FcpFusedWork &W, ihipStream_t *s) {
  if (W.dense_blocks <= 0 && W.ragged_blocks <= 0) return 0;
  if (fcp_work_sharded(W)) return (int)hipErrorInvalidValue;
  return fcp_launch_work(
      W, s, [](auto V, auto R) { return fcp_dense_tabmix_kernel<V, R>; }, [](auto V) { return fcp_ragged_tabmix_kernel<V>; },
      [](auto V, auto R) { return fcp_hybrid_tabmix_kernel<V, R>; });
}
