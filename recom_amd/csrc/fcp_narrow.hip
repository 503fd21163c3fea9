// fcp_narrow.hip — the fused kernels for plans whose concat output is bf16 or fp16 (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16):
// the network behind the embedding layer runs in one of the two on an MI355X, and the output stores are the one part of a
// request whose cost still scales with bytes.  The reference writes float32 only.
//
// A translation unit of its own, for the reason fcp_weighted.hip is one: the 42 tuned instantiations of fcp_kernels.hip
// stay the code they are.  These are the SAME bodies (dense_body / ragged_body<..., NARROW = true>, fcp_fused_bodies.h) with
// the same slot map, span lists, rows per wave, LDS layout and grids: a slot is still V elements, a span 64 slots.  What
// differs is the output address (2 bytes per element) and the store: the float32 value the plan would have written is
// rounded once, to nearest-even, and the lane stores 2 * V bytes — global_store_dwordx2 | _dword | _short, in the same
// three cache policies.  The element type is launch-uniform: `out_kind` (FCP_OUT_BF16 | FCP_OUT_F16) is a kernel argument
// and a wave-uniform branch at the store, so the matrix is 9 + 3 + 9 = 21 kernels, not 42.  Unsharded plans only.
#include "fcp_fused_bodies.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_narrow_kernel(const FcpLaunch L, int out_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, true>(L, blockIdx.x, smem, out_kind);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_ragged_narrow_kernel(const FcpLaunch L, int out_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, false, true>(L, blockIdx.x, smem, nullptr, out_kind);
}

// (the argument block of fcp_hybrid_kernel, fcp_kernels.hip)
struct FcpHybridNarrowLaunch {
  FcpLaunch ragged; // blocks [0, ragged_blocks)
  FcpLaunch dense;  // blocks [ragged_blocks, grid)
  int32_t ragged_blocks;
};

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_hybrid_narrow_kernel(const FcpHybridNarrowLaunch H, int out_kind) {
  constexpr size_t kSmem = sizeof(RaggedLds) > sizeof(DenseLds<R>) ? sizeof(RaggedLds) : sizeof(DenseLds<R>);
  __shared__ __attribute__((aligned(16))) char smem[kSmem];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, false, true>(H.ragged, bid, smem, nullptr, out_kind); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, true>(H.dense, bid - H.ragged_blocks, smem, out_kind);
  }
}

// the request's stop event / any-order flag, as the other fused launches take them
template <typename K, typename... A> void launch(K kernel, int grid_blocks, ihipStream_t *s, A... args) {
  void *stop = nullptr;
  int flags = 0;
  fcp_take_launch_extras(&stop, &flags);
  const dim3 grid(grid_blocks), block(FCP_BLOCK_THREADS);
  if (stop || flags)
    hipExtLaunchKernelGGL(kernel, grid, block, 0, s, nullptr, static_cast<hipEvent_t>(stop), flags, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

template <int V> void launch_dense(const FcpLaunch &L, int out_kind, int grid_blocks, ihipStream_t *s) {
  if (L.rows_per_wave == 4)
    launch(fcp_dense_narrow_kernel<V, 4>, grid_blocks, s, L, out_kind);
  else if (L.rows_per_wave == 2)
    launch(fcp_dense_narrow_kernel<V, 2>, grid_blocks, s, L, out_kind);
  else
    launch(fcp_dense_narrow_kernel<V, 1>, grid_blocks, s, L, out_kind);
}

template <int V> void launch_hybrid(const FcpHybridNarrowLaunch &H, int out_kind, int grid_blocks, ihipStream_t *s) {
  if (H.dense.rows_per_wave == 4)
    launch(fcp_hybrid_narrow_kernel<V, 4>, grid_blocks, s, H, out_kind);
  else if (H.dense.rows_per_wave == 2)
    launch(fcp_hybrid_narrow_kernel<V, 2>, grid_blocks, s, H, out_kind);
  else
    launch(fcp_hybrid_narrow_kernel<V, 1>, grid_blocks, s, H, out_kind);
}

} // namespace

// vec: 4 | 2 | 1; rows per wave (dense) from L.rows_per_wave; out_kind: FCP_OUT_BF16 | FCP_OUT_F16
int fcp_launch_narrow(const FcpLaunch &L, int vec, bool dense_kernel, int out_kind, int grid_blocks, ihipStream_t *s) {
  if (grid_blocks <= 0) return 0;
  if (L.shard_world > 1 || (out_kind != FCP_OUT_BF16 && out_kind != FCP_OUT_F16)) return (int)hipErrorInvalidValue;
  if (dense_kernel) {
    if (vec == 4)
      launch_dense<4>(L, out_kind, grid_blocks, s);
    else if (vec == 2)
      launch_dense<2>(L, out_kind, grid_blocks, s);
    else
      launch_dense<1>(L, out_kind, grid_blocks, s);
  } else {
    if (vec == 4)
      launch(fcp_ragged_narrow_kernel<4>, grid_blocks, s, L, out_kind);
    else if (vec == 2)
      launch(fcp_ragged_narrow_kernel<2>, grid_blocks, s, L, out_kind);
    else
      launch(fcp_ragged_narrow_kernel<1>, grid_blocks, s, L, out_kind);
  }
  return (int)hipGetLastError();
}

int fcp_launch_narrow_hybrid(const FcpLaunch &Ldense, int dense_blocks, const FcpLaunch &Lragged, int ragged_blocks, int vec,
                             int out_kind, ihipStream_t *s) {
  if (Ldense.shard_world > 1 || (out_kind != FCP_OUT_BF16 && out_kind != FCP_OUT_F16)) return (int)hipErrorInvalidValue;
  FcpHybridNarrowLaunch H;
  H.ragged = Lragged;
  H.dense = Ldense;
  H.ragged_blocks = ragged_blocks;
  const int grid_blocks = dense_blocks + ragged_blocks;
  if (vec == 4)
    launch_hybrid<4>(H, out_kind, grid_blocks, s);
  else if (vec == 2)
    launch_hybrid<2>(H, out_kind, grid_blocks, s);
  else
    launch_hybrid<1>(H, out_kind, grid_blocks, s);
  return (int)hipGetLastError();
}
