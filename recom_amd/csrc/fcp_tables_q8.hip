// fcp_tables_q8.hip — the fused kernels for plans whose embedding tables are 8-bit row-quantised (FCP_FLAG_TABLES_Q8): the
// "fused 8-bit rowwise" serving format — dim uint8 codes, a float32 scale and a float32 bias per row, dim + 8 bytes, rows
// back to back.  A quarter of the float32 footprint decides whether a model needs more than one GPU.  The reference reads
// float32 tables only.
//
// A translation unit of its own, for the reason fcp_narrow.hip and fcp_tables16.hip are: the tuned instantiations of
// fcp_kernels.hip stay the code they are.  These are the SAME bodies (dense_body / ragged_body<..., TABQ8 = true>,
// fcp_fused_bodies.h) with the same slot map, span lists, rows per wave, LDS layout, grids and parked 32-bit slot offsets: a
// slot is still V elements, a span 64 slots.  What differs is the table address — a row index is scaled by the row STRIDE in
// slots, (dim + 8) / V, so that a slot offset x V is the row's byte offset — and the load: a lane reads its V code bytes
// (global_load_dword | _ushort | _ubyte) and the row's scale and bias, and dequantises with one v_fma_f32 per element to the
// float32 values the float32 plan would have read from the dequantised table; everything behind that (sums in id order,
// means, copies, stores) is the float32 plan's.  9 + 3 + 9 = 21 kernels.  Unsharded, float32 output.
#include "fcp_fused_bodies.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_tabq8_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, false, false, true>(L, blockIdx.x, smem);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_ragged_tabq8_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, false, false, false, true>(L, blockIdx.x, smem);
}

// (the argument block of fcp_hybrid_kernel, fcp_kernels.hip)
struct FcpHybridTabQ8Launch {
  FcpLaunch ragged; // blocks [0, ragged_blocks)
  FcpLaunch dense;  // blocks [ragged_blocks, grid)
  int32_t ragged_blocks;
};

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_hybrid_tabq8_kernel(const FcpHybridTabQ8Launch H) {
  constexpr size_t kSmem = sizeof(RaggedLds) > sizeof(DenseLds<R>) ? sizeof(RaggedLds) : sizeof(DenseLds<R>);
  __shared__ __attribute__((aligned(16))) char smem[kSmem];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, false, false, false, true>(H.ragged, bid, smem); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, false, false, true>(H.dense, bid - H.ragged_blocks, smem);
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

template <int V> void launch_dense(const FcpLaunch &L, int grid_blocks, ihipStream_t *s) {
  if (L.rows_per_wave == 4)
    launch(fcp_dense_tabq8_kernel<V, 4>, grid_blocks, s, L);
  else if (L.rows_per_wave == 2)
    launch(fcp_dense_tabq8_kernel<V, 2>, grid_blocks, s, L);
  else
    launch(fcp_dense_tabq8_kernel<V, 1>, grid_blocks, s, L);
}

template <int V> void launch_hybrid(const FcpHybridTabQ8Launch &H, int grid_blocks, ihipStream_t *s) {
  if (H.dense.rows_per_wave == 4)
    launch(fcp_hybrid_tabq8_kernel<V, 4>, grid_blocks, s, H);
  else if (H.dense.rows_per_wave == 2)
    launch(fcp_hybrid_tabq8_kernel<V, 2>, grid_blocks, s, H);
  else
    launch(fcp_hybrid_tabq8_kernel<V, 1>, grid_blocks, s, H);
}

} // namespace

// vec: 4 | 2 | 1; rows per wave (dense) from L.rows_per_wave
int fcp_launch_tabq8(const FcpLaunch &L, int vec, bool dense_kernel, int grid_blocks, ihipStream_t *s) {
  if (grid_blocks <= 0) return 0;
  if (L.shard_world > 1) return (int)hipErrorInvalidValue;
  if (dense_kernel) {
    if (vec == 4)
      launch_dense<4>(L, grid_blocks, s);
    else if (vec == 2)
      launch_dense<2>(L, grid_blocks, s);
    else
      launch_dense<1>(L, grid_blocks, s);
  } else {
    if (vec == 4)
      launch(fcp_ragged_tabq8_kernel<4>, grid_blocks, s, L);
    else if (vec == 2)
      launch(fcp_ragged_tabq8_kernel<2>, grid_blocks, s, L);
    else
      launch(fcp_ragged_tabq8_kernel<1>, grid_blocks, s, L);
  }
  return (int)hipGetLastError();
}

int fcp_launch_tabq8_hybrid(const FcpLaunch &Ldense, int dense_blocks, const FcpLaunch &Lragged, int ragged_blocks, int vec,
                            ihipStream_t *s) {
  if (Ldense.shard_world > 1) return (int)hipErrorInvalidValue;
  FcpHybridTabQ8Launch H;
  H.ragged = Lragged;
  H.dense = Ldense;
  H.ragged_blocks = ragged_blocks;
  const int grid_blocks = dense_blocks + ragged_blocks;
  if (vec == 4)
    launch_hybrid<4>(H, grid_blocks, s);
  else if (vec == 2)
    launch_hybrid<2>(H, grid_blocks, s);
  else
    launch_hybrid<1>(H, grid_blocks, s);
  return (int)hipGetLastError();
}
