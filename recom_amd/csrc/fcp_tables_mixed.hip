// fcp_tables_mixed.hip — the fused kernels for plans whose embedding tables have MORE THAN ONE format
// (FCP_FLAG_TABLES_PER_INPUT with tables that really differ): float32, bf16, fp16 and 8-bit row-quantised tables side by side
// in one plan — big tables at 8 bits, small or quality-sensitive ones at 16 or 32, a dim-1 "wide" column never as a 9-byte q8
// row.  Plans whose tables all share one format take that format's plan-wide kernels (fcp_kernels.hip, fcp_tables16.hip,
// fcp_tables_q8.hip), never these.
//
// A translation unit of its own, for the reason the other table units are: the tuned instantiations stay the code they are.
// These are the SAME bodies (dense_body / ragged_body<..., TABMIX = true>, fcp_fused_bodies.h) with the same slot map, span
// lists, rows per wave, LDS layout and grids.  A span is 64 slots of the concat row, so one wave routinely holds columns of
// different formats: the kind is a fact of each COLUMN — bits 16..17 of its record's flags (FCP_F_TABKIND), staged with the
// record, no record or LDS structure grows — and a lane picks its table address, row stride and loader by it.  Where one
// ballot shows that the whole wave holds one kind, the choice is a scalar branch; the three exec-masked sections are paid
// only by waves that really mix.  9 + 3 + 9 = 21 kernels.  Unsharded, float32 output.
#include "fcp_fused_bodies.h"

namespace {

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_tabmix_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, false, false, false, false, true>(L, blockIdx.x, smem);
}

// Eight waves per SIMD where the body fits 64 VGPRs.  At V = 4 it does not: fcp_ragged_kernel<4> sits at exactly 64, and the
// lane's kind next to the q8 walk's tail does not fit beside a 10-wide batch without scratch — that instantiation (and the
// hybrid ones that contain it) is left to the allocator: more registers, fewer waves, no scratch.
template <int V> constexpr int kMixMinWaves = V == 4 ? 1 : 8;

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(kMixMinWaves<V>, 8)))
fcp_ragged_tabmix_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, false, false, false, false, false, true>(L, blockIdx.x, smem);
}

// (the argument block of fcp_hybrid_kernel, fcp_kernels.hip)
struct FcpHybridTabMixLaunch {
  FcpLaunch ragged; // blocks [0, ragged_blocks)
  FcpLaunch dense;  // blocks [ragged_blocks, grid)
  int32_t ragged_blocks;
};

template <int V, int R>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(kMixMinWaves<V>, 8)))
fcp_hybrid_tabmix_kernel(const FcpHybridTabMixLaunch H) {
  constexpr size_t kSmem = sizeof(RaggedLds) > sizeof(DenseLds<R>) ? sizeof(RaggedLds) : sizeof(DenseLds<R>);
  __shared__ __attribute__((aligned(16))) char smem[kSmem];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, false, false, false, false, false, true>(H.ragged, bid, smem); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, false, false, false, false, true>(H.dense, bid - H.ragged_blocks, smem);
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
    launch(fcp_dense_tabmix_kernel<V, 4>, grid_blocks, s, L);
  else if (L.rows_per_wave == 2)
    launch(fcp_dense_tabmix_kernel<V, 2>, grid_blocks, s, L);
  else
    launch(fcp_dense_tabmix_kernel<V, 1>, grid_blocks, s, L);
}

template <int V> void launch_hybrid(const FcpHybridTabMixLaunch &H, int grid_blocks, ihipStream_t *s) {
  if (H.dense.rows_per_wave == 4)
    launch(fcp_hybrid_tabmix_kernel<V, 4>, grid_blocks, s, H);
  else if (H.dense.rows_per_wave == 2)
    launch(fcp_hybrid_tabmix_kernel<V, 2>, grid_blocks, s, H);
  else
    launch(fcp_hybrid_tabmix_kernel<V, 1>, grid_blocks, s, H);
}

} // namespace

// vec: 4 | 2 | 1; rows per wave (dense) from L.rows_per_wave
int fcp_launch_tabmix(const FcpLaunch &L, int vec, bool dense_kernel, int grid_blocks, ihipStream_t *s) {
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
      launch(fcp_ragged_tabmix_kernel<4>, grid_blocks, s, L);
    else if (vec == 2)
      launch(fcp_ragged_tabmix_kernel<2>, grid_blocks, s, L);
    else
      launch(fcp_ragged_tabmix_kernel<1>, grid_blocks, s, L);
  }
  return (int)hipGetLastError();
}

int fcp_launch_tabmix_hybrid(const FcpLaunch &Ldense, int dense_blocks, const FcpLaunch &Lragged, int ragged_blocks, int vec,
                            ihipStream_t *s) {
  if (Ldense.shard_world > 1) return (int)hipErrorInvalidValue;
  FcpHybridTabMixLaunch H;
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
