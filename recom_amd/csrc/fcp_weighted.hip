// fcp_weighted.hip — the ragged kernel for plans with per-id weights or the sqrtn combiner: TensorFlow's
// weighted_categorical_column / embedding_lookup_sparse(sp_ids, sp_weights, combiner) — `embeddings *= weights`, a segment
// sum, then a division by the sum of the weights (mean) or by the square root of the sum of their squares (sqrtn).  The
// reference has neither.
//
// A translation unit of its own: fcp_ragged_kernel<4, *> and the hybrid kernels sit at exactly 64 VGPRs, so the weight
// path has no room in them; this instantiation of the same body (ragged_body<V, SHARDED, true>, fcp_fused_bodies.h) is
// launched only for plans that need it and serves ALL their spans — one-hot, passthrough and unweighted pooled columns
// behave in it exactly as in the unweighted kernels.  Same block shape, same LDS, same launch geometry as the ragged kernel.
#include "fcp_fused_bodies.h"

namespace {

template <int V, bool SHARDED>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_weighted_bag_kernel(const FcpLaunch L, const int64_t *wts) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, SHARDED, true>(L, blockIdx.x, smem, wts);
}

template <int V, bool SHARDED>
void launch(const FcpLaunch &L, const int64_t *wts, int grid_blocks, ihipStream_t *s) {
  void *stop = nullptr;
  int flags = 0;
  fcp_take_launch_extras(&stop, &flags); // the request's stop event / any-order flag, as the other fused launches take them
  const dim3 grid(grid_blocks), block(FCP_BLOCK_THREADS);
  if (stop || flags)
    hipExtLaunchKernelGGL((fcp_weighted_bag_kernel<V, SHARDED>), grid, block, 0, s, nullptr, static_cast<hipEvent_t>(stop), flags, L, wts);
  else
    hipLaunchKernelGGL((fcp_weighted_bag_kernel<V, SHARDED>), grid, block, 0, s, L, wts);
}

} // namespace

// vec: 4 | 2 | 1; one row per wave, as the ragged kernel
int fcp_launch_weighted(const FcpLaunch &L, const int64_t *wts, int vec, int grid_blocks, ihipStream_t *s) {
  if (grid_blocks <= 0) return 0;
  const bool sharded = L.shard_world > 1;
  if (vec == 4)
    sharded ? launch<4, true>(L, wts, grid_blocks, s) : launch<4, false>(L, wts, grid_blocks, s);
  else if (vec == 2)
    sharded ? launch<2, true>(L, wts, grid_blocks, s) : launch<2, false>(L, wts, grid_blocks, s);
  else
    sharded ? launch<1, true>(L, wts, grid_blocks, s) : launch<1, false>(L, wts, grid_blocks, s);
  return (int)hipGetLastError();
}
