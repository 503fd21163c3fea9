// fcp_tables16.hip — the fused kernels for plans whose embedding tables are bf16 or fp16 (FCP_FLAG_TABLES_BF16 /
// FCP_FLAG_TABLES_F16): the tables are all but the whole of a model's footprint, and checkpoints are kept in one of the two.
// The reference reads float32 tables only.
//
// A translation unit of its own, for the reason fcp_narrow.hip is one: the tuned instantiations of fcp_kernels.hip stay
// the code they are.  These are the SAME bodies (dense_body / ragged_body<..., TAB16 = true>, fcp_fused_bodies.h) with the
// same slot map, span lists, rows per wave, LDS layout, grids and parked 32-bit slot offsets: a slot is still V elements, a
// span 64 slots.  What differs is the table address (2 bytes per element, formed in 64 bits) and the load: a lane reads
// 2 * V bytes — global_load_dwordx2 | _dword | _ushort — and widens them to the float32 values the float32 plan would
// have read; the widening is exact, so everything behind it (sums in id order, means, copies, stores) is the float32
// plan's.  The element type is launch-uniform: `tab_kind` (FCP_TAB_BF16 | FCP_TAB_F16) is a kernel argument and a
// wave-uniform branch behind the load, so the matrix is 9 + 3 + 9 = 21 kernels, not 42.  Unsharded, float32 output.
#include "fcp_fused_bodies.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_tab16_kernel(const FcpLaunch L, int tab_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, false, true>(L, blockIdx.x, smem, 0, tab_kind);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_ragged_tab16_kernel(const FcpLaunch L, int tab_kind) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, false, false, true>(L, blockIdx.x, smem, nullptr, 0, tab_kind);
}

// (the argument block of fcp_hybrid_kernel, fcp_kernels.hip)
struct FcpHybridTab16Launch {
  FcpLaunch ragged; // blocks [0, ragged_blocks)
  FcpLaunch dense;  // blocks [ragged_blocks, grid)
  int32_t ragged_blocks;
};

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_hybrid_tab16_kernel(const FcpHybridTab16Launch H, int tab_kind) {
  constexpr size_t kSmem = sizeof(RaggedLds) > sizeof(DenseLds<R>) ? sizeof(RaggedLds) : sizeof(DenseLds<R>);
  __shared__ __attribute__((aligned(16))) char smem[kSmem];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, false, false, true>(H.ragged, bid, smem, nullptr, 0, tab_kind); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, false, true>(H.dense, bid - H.ragged_blocks, smem, 0, tab_kind);
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

template <int V> void launch_dense(const FcpLaunch &L, int tab_kind, int grid_blocks, ihipStream_t *s) {
  if (L.rows_per_wave == 4)
    launch(fcp_dense_tab16_kernel<V, 4>, grid_blocks, s, L, tab_kind);
  else if (L.rows_per_wave == 2)
    launch(fcp_dense_tab16_kernel<V, 2>, grid_blocks, s, L, tab_kind);
  else
    launch(fcp_dense_tab16_kernel<V, 1>, grid_blocks, s, L, tab_kind);
}

template <int V> void launch_hybrid(const FcpHybridTab16Launch &H, int tab_kind, int grid_blocks, ihipStream_t *s) {
  if (H.dense.rows_per_wave == 4)
    launch(fcp_hybrid_tab16_kernel<V, 4>, grid_blocks, s, H, tab_kind);
  else if (H.dense.rows_per_wave == 2)
    launch(fcp_hybrid_tab16_kernel<V, 2>, grid_blocks, s, H, tab_kind);
  else
    launch(fcp_hybrid_tab16_kernel<V, 1>, grid_blocks, s, H, tab_kind);
}

} // namespace

// vec: 4 | 2 | 1; rows per wave (dense) from L.rows_per_wave; tab_kind: FCP_TAB_BF16 | FCP_TAB_F16
int fcp_launch_tab16(const FcpLaunch &L, int vec, bool dense_kernel, int tab_kind, int grid_blocks, ihipStream_t *s) {
  if (grid_blocks <= 0) return 0;
  if (L.shard_world > 1 || (tab_kind != FCP_TAB_BF16 && tab_kind != FCP_TAB_F16)) return (int)hipErrorInvalidValue;
  if (dense_kernel) {
    if (vec == 4)
      launch_dense<4>(L, tab_kind, grid_blocks, s);
    else if (vec == 2)
      launch_dense<2>(L, tab_kind, grid_blocks, s);
    else
      launch_dense<1>(L, tab_kind, grid_blocks, s);
  } else {
    if (vec == 4)
      launch(fcp_ragged_tab16_kernel<4>, grid_blocks, s, L, tab_kind);
    else if (vec == 2)
      launch(fcp_ragged_tab16_kernel<2>, grid_blocks, s, L, tab_kind);
    else
      launch(fcp_ragged_tab16_kernel<1>, grid_blocks, s, L, tab_kind);
  }
  return (int)hipGetLastError();
}

int fcp_launch_tab16_hybrid(const FcpLaunch &Ldense, int dense_blocks, const FcpLaunch &Lragged, int ragged_blocks, int vec,
                             int tab_kind, ihipStream_t *s) {
  if (Ldense.shard_world > 1 || (tab_kind != FCP_TAB_BF16 && tab_kind != FCP_TAB_F16)) return (int)hipErrorInvalidValue;
  FcpHybridTab16Launch H;
  H.ragged = Lragged;
  H.dense = Ldense;
  H.ragged_blocks = ragged_blocks;
  const int grid_blocks = dense_blocks + ragged_blocks;
  if (vec == 4)
    launch_hybrid<4>(H, tab_kind, grid_blocks, s);
  else if (vec == 2)
    launch_hybrid<2>(H, tab_kind, grid_blocks, s);
  else
    launch_hybrid<1>(H, tab_kind, grid_blocks, s);
  return (int)hipGetLastError();
}
