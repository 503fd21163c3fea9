// fcp_fused_launch.h — what the translation units of the fused kernels share on top of the bodies (fcp_fused_bodies.h): the
// argument block and the LDS size of a hybrid kernel, the launch that carries a request's stop event and any-order flag, and
// the dispatch from a request's fused work (FcpFusedWork, fcp_internal.h) to one kernel instantiation.  The `__global__`
// templates themselves stay in their units — fcp_kernels.hip, fcp_weighted.hip, fcp_narrow.hip, fcp_tables16.hip,
// fcp_tables_q8.hip, fcp_tables_mixed.hip — with their names, launch bounds and occupancy attributes.
#pragma once
#include <type_traits>

#include "fcp_fused_bodies.h"

namespace {

// ---------------------------------------------------------------------------
// Hybrid launch: plans that mix one-hot and pooled columns (the reference's models
// E / F: ~98 % bucketize / hash one-hot columns plus a few multi-hot ones).  Spans
// whose columns are all GATHER / PASSTHROUGH run the dense body, the other spans
// the ragged body — in ONE launch (block-uniform branch, one LDS buffer carved by
// either body), because these models are launch-latency bound: as separate
// dependent launches they cost 27.6 us per request, see DESIGN.md.
// ---------------------------------------------------------------------------
struct FcpHybridLaunch {
  FcpLaunch ragged; // blocks [0, ragged_blocks)
  FcpLaunch dense;  // blocks [ragged_blocks, grid)
  int32_t ragged_blocks;
};

// LDS bytes of a hybrid kernel.  (The split itself — `blockIdx.x < H.ragged_blocks` ? ragged body : dense body — is written
// out in each hybrid kernel: behind a shared inline function the compiler orders the front's scalar loads differently.)
template <int R> constexpr size_t kHybridLds = sizeof(RaggedLds) > sizeof(DenseLds<R>) ? sizeof(RaggedLds) : sizeof(DenseLds<R>);

// The launch of a fused kernel: it takes the request's stop event and any-order flag (fcp_set_stop_event,
// fcp_set_any_order) and goes through the extended launch only when there is either.
template <typename K, typename... A> void fcp_klaunch(K kernel, int grid_blocks, ihipStream_t *s, const A &...args) {
  void *stop = nullptr;
  int flags = 0;
  fcp_take_launch_extras(&stop, &flags);
  const dim3 grid(grid_blocks), block(FCP_BLOCK_THREADS);
  if (stop || flags)
    hipExtLaunchKernelGGL(kernel, grid, block, 0, s, nullptr, static_cast<hipEvent_t>(stop), flags, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

// A run-time value as a template argument: f(std::integral_constant<int, N>()) for the first N of the list equal to v,
// for the last one when none is.
template <int N, int... Rest, typename F> void with_int(int v, F &&f) {
  if constexpr (sizeof...(Rest) == 0)
    f(std::integral_constant<int, N>());
  else if (v == N)
    f(std::integral_constant<int, N>());
  else
    with_int<Rest...>(v, f);
}
template <typename F> void with_bool(bool v, F &&f) {
  if (v)
    f(std::true_type());
  else
    f(std::false_type());
}

inline bool fcp_work_sharded(const FcpFusedWork &W) { return (W.dense_blocks > 0 ? W.dense : W.ragged)->shard_world > 1; }

// The dispatch of a unit with a dense, a ragged and a hybrid kernel template: hybrid when both sides of W have blocks, else
// ragged, else dense; nothing when neither has.  dense(V, R), ragged(V) and hybrid(V, R) return the unit's instantiation for
// those (integral-constant) arguments; `extra` follows the FcpLaunch / FcpHybridLaunch in the kernel's arguments.
template <typename D, typename G, typename H, typename... A>
int fcp_launch_work(const FcpFusedWork &W, ihipStream_t *s, D dense, G ragged, H hybrid, const A &...extra) {
  if (W.dense_blocks <= 0 && W.ragged_blocks <= 0) return 0;
  with_int<4, 2, 1>(W.vec, [&](auto V) {
    if (W.dense_blocks <= 0) {
      fcp_klaunch(ragged(V), W.ragged_blocks, s, *W.ragged, extra...);
      return;
    }
    with_int<4, 2, 1>(W.dense->rows_per_wave, [&](auto R) {
      if (W.ragged_blocks <= 0) {
        fcp_klaunch(dense(V, R), W.dense_blocks, s, *W.dense, extra...);
        return;
      }
      FcpHybridLaunch Hy;
      Hy.ragged = *W.ragged;
      Hy.dense = *W.dense;
      Hy.ragged_blocks = W.ragged_blocks;
      fcp_klaunch(hybrid(V, R), W.dense_blocks + W.ragged_blocks, s, Hy, extra...);
    });
  });
  return (int)hipGetLastError();
}

} // namespace
