// fcp_tables_q8.hip — the fused kernels for plans whose embedding tables are 8-bit row-quantised (FCP_FLAG_TABLES_Q8): the
// "fused 8-bit rowwise" serving format — dim uint8 codes, a float32 scale and a float32 bias per row, dim + 8 bytes, rows
// back to back.  A quarter of the float32 footprint decides whether a model needs more than one GPU.  The reference reads
// float32 tables only.
//
// A translation unit of its own, for the reason fcp_narrow.hip and fcp_tables16.hip are: the tuned instantiations of
// fcp_kernels.hip stay the code they are.  These are the SAME bodies (dense_body / ragged_body<..., FCP_VAR_TABQ8>,
// fcp_fused_bodies.h) with the same slot map, span lists, rows per wave, LDS layout, grids and parked 32-bit slot offsets: a
// slot is still V elements, a span 64 slots.  What differs is the table address — a row index is scaled by the row STRIDE in
// slots, (dim + 8) / V, so that a slot offset x V is the row's byte offset — and the load: a lane reads its V code bytes
// (global_load_dword | _ushort | _ubyte) and the row's scale and bias, and dequantises with one v_fma_f32 per element to the
// float32 values the float32 plan would have read from the dequantised table; everything behind that (sums in id order,
// means, copies, stores) is the float32 plan's.  9 + 3 + 9 = 21 kernels.  Unsharded, float32 output.
#include "fcp_fused_launch.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_tabq8_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, FCP_VAR_TABQ8>(L, blockIdx.x, smem);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_ragged_tabq8_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, FCP_VAR_TABQ8>(L, blockIdx.x, smem);
}

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_hybrid_tabq8_kernel(const FcpHybridLaunch H) {
  __shared__ __attribute__((aligned(16))) char smem[kHybridLds<R>];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, FCP_VAR_TABQ8>(H.ragged, bid, smem); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, FCP_VAR_TABQ8>(H.dense, bid - H.ragged_blocks, smem);
  }
}

} // namespace

int fcp_launch_tabq8(const FcpFusedWork &W, ihipStream_t *s) {
  if (W.dense_blocks <= 0 && W.ragged_blocks <= 0) return 0;
  if (fcp_work_sharded(W)) return (int)hipErrorInvalidValue;
  return fcp_launch_work(
      W, s, [](auto V, auto R) { return fcp_dense_tabq8_kernel<V, R>; }, [](auto V) { return fcp_ragged_tabq8_kernel<V>; },
      [](auto V, auto R) { return fcp_hybrid_tabq8_kernel<V, R>; });
}
