// fcp_weighted.hip — the ragged kernel for plans with per-id weights or the sqrtn combiner: TensorFlow's
// weighted_categorical_column / embedding_lookup_sparse(sp_ids, sp_weights, combiner) — `embeddings *= weights`, a segment
// sum, then a division by the sum of the weights (mean) or by the square root of the sum of their squares (sqrtn).  The
// reference has neither.
//
// A translation unit of its own: fcp_ragged_kernel<4, *> and the hybrid kernels sit at exactly 64 VGPRs, so the weight
// path has no room in them; this instantiation of the same body (ragged_body<V, SHARDED, FCP_VAR_WEIGHTED>, fcp_fused_bodies.h) is
// launched only for plans that need it and serves ALL their spans — one-hot, passthrough and unweighted pooled columns
// behave in it exactly as in the unweighted kernels.  Same block shape, same LDS, same launch geometry as the ragged kernel.
#include "fcp_fused_launch.h"

namespace {

template <int V, bool SHARDED>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8)))
fcp_weighted_bag_kernel(const FcpLaunch L, const int64_t *wts) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, SHARDED, FCP_VAR_WEIGHTED>(L, blockIdx.x, smem, wts);
}

} // namespace

// one row per wave, as the ragged kernel; W.dense is not read
int fcp_launch_weighted(const FcpFusedWork &W, ihipStream_t *s) {
  if (W.ragged_blocks <= 0) return 0;
  with_int<4, 2, 1>(W.vec, [&](auto V) {
    with_bool(W.ragged->shard_world > 1,
              [&](auto SHARDED) { fcp_klaunch(fcp_weighted_bag_kernel<V, SHARDED>, W.ragged_blocks, s, *W.ragged, W.wts); });
  });
  return (int)hipGetLastError();
}
