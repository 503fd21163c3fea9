// fcp_narrow.hip — the fused kernels for plans whose concat output is bf16 or fp16 (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16):
// the network behind the embedding layer runs in one of the two on an MI355X, and the output stores are the one part of a
// request whose cost still scales with bytes.  The reference writes float32 only.
//
// A translation unit of its own, for the reason fcp_weighted.hip is one: the 42 tuned instantiations of fcp_kernels.hip
// stay the code they are.  These are the SAME bodies (dense_body / ragged_body<..., FCP_VAR_NARROW>, fcp_fused_bodies.h) with
// the same slot map, span lists, rows per wave, LDS layout and grids: a slot is still V elements, a span 64 slots.  What
// differs is the output address (2 bytes per element) and the store: the float32 value the plan would have written is
// rounded once, to nearest-even, and the lane stores 2 * V bytes — global_store_dwordx2 | _dword | _short, in the same
// three cache policies.  The element type is launch-uniform: `out_kind` (FCP_OUT_BF16 | FCP_OUT_F16) is a kernel argument
// and a wave-uniform branch at the store, so the matrix is 9 + 3 + 9 = 21 kernels, not 42.  Unsharded plans only.
#include "fcp_fused_launch.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_narrow_kernel(const FcpLaunch L, int out_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, FCP_VAR_NARROW>(L, blockIdx.x, smem, out_kind);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_ragged_narrow_kernel(const FcpLaunch L, int out_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, FCP_VAR_NARROW>(L, blockIdx.x, smem, nullptr, out_kind);
}

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_hybrid_narrow_kernel(const FcpHybridLaunch H, int out_kind) {
  __shared__ __attribute__((aligned(16))) char smem[kHybridLds<R>];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, FCP_VAR_NARROW>(H.ragged, bid, smem, nullptr, out_kind); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, FCP_VAR_NARROW>(H.dense, bid - H.ragged_blocks, smem, out_kind);
  }
}

} // namespace

int fcp_launch_narrow(const FcpFusedWork &W, ihipStream_t *s) {
  if (W.dense_blocks <= 0 && W.ragged_blocks <= 0) return 0;
  if (fcp_work_sharded(W) || (W.kind != FCP_OUT_BF16 && W.kind != FCP_OUT_F16)) return (int)hipErrorInvalidValue;
  return fcp_launch_work(
      W, s, [](auto V, auto R) { return fcp_dense_narrow_kernel<V, R>; }, [](auto V) { return fcp_ragged_narrow_kernel<V>; },
      [](auto V, auto R) { return fcp_hybrid_narrow_kernel<V, R>; }, W.kind);
}
