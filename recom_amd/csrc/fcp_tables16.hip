// fcp_tables16.hip — the fused kernels for plans whose embedding tables are bf16 or fp16 (FCP_FLAG_TABLES_BF16 /
// FCP_FLAG_TABLES_F16): the tables are all but the whole of a model's footprint, and checkpoints are kept in one of the two.
// The reference reads float32 tables only.
//
// A translation unit of its own, for the reason fcp_narrow.hip is one: the tuned instantiations of fcp_kernels.hip stay
// the code they are.  These are the SAME bodies (dense_body / ragged_body<..., FCP_VAR_TAB16>, fcp_fused_bodies.h) with the
// same slot map, span lists, rows per wave, LDS layout, grids and parked 32-bit slot offsets: a slot is still V elements, a
// span 64 slots.  What differs is the table address (2 bytes per element, formed in 64 bits) and the load: a lane reads
// 2 * V bytes — global_load_dwordx2 | _dword | _ushort — and widens them to the float32 values the float32 plan would
// have read; the widening is exact, so everything behind it (sums in id order, means, copies, stores) is the float32
// plan's.  The element type is launch-uniform: `tab_kind` (FCP_TAB_BF16 | FCP_TAB_F16) is a kernel argument and a
// wave-uniform branch behind the load, so the matrix is 9 + 3 + 9 = 21 kernels, not 42.  Unsharded, float32 output.
#include "fcp_fused_launch.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_tab16_kernel(const FcpLaunch L, int tab_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, FCP_VAR_TAB16>(L, blockIdx.x, smem, tab_kind);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_ragged_tab16_kernel(const FcpLaunch L, int tab_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, FCP_VAR_TAB16>(L, blockIdx.x, smem, nullptr, tab_kind);
}

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_hybrid_tab16_kernel(const FcpHybridLaunch H, int tab_kind) {
  __shared__ __attribute__((aligned(16))) char smem[kHybridLds<R>];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, FCP_VAR_TAB16>(H.ragged, bid, smem, nullptr, tab_kind); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, FCP_VAR_TAB16>(H.dense, bid - H.ragged_blocks, smem, tab_kind);
  }
}

} // namespace

int fcp_launch_tab16(const FcpFusedWork &W, ihipStream_t *s) {
  if (W.dense_blocks <= 0 && W.ragged_blocks <= 0) return 0;
  if (fcp_work_sharded(W) || (W.kind != FCP_TAB_BF16 && W.kind != FCP_TAB_F16)) return (int)hipErrorInvalidValue;
  return fcp_launch_work(
      W, s, [](auto V, auto R) { return fcp_dense_tab16_kernel<V, R>; }, [](auto V) { return fcp_ragged_tab16_kernel<V>; },
      [](auto V, auto R) { return fcp_hybrid_tab16_kernel<V, R>; }, W.kind);
}
