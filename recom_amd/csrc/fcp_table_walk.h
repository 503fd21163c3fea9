// fcp_table_walk.h — what the units that walk float32 table rows share: fcp_convert.hip (fcp_quantize_q8_kernel), fcp_table_rows.hip
// (fcp_update_q8_kernel) and fcp_table_audit.hip (fcp_table_audit_kernel) handle a row by the same power-of-two lane group, with
// the same V-element slots and the same in-register cap, and form q8 codes by the same arithmetic.  The walk itself (RowSlots),
// the row quantiser (quantize_row), the constants, the slot loads / stores, the group rule and the host's dispatch on G and V
// (with_group, with_vec) are written here ONCE; the kernels keep what differs between them.  Everything lives in an unnamed
// namespace, as in fcp_fused_bodies.h: each translation unit gets its own copy.  The includer switches contraction off (#pragma
// clang fp contract(off)) BEFORE it includes this header, and includes fcp_fused_bodies.h ahead of the pragma: q8_code rounds
// every operation once, and the bodies keep the mode they have in every other unit.
#pragma once
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#include <type_traits>

namespace {

constexpr int kQSlots = 4;                          // slots of a row a lane of a 64-lane group keeps in registers
constexpr int64_t kMaxLaunchThreads = 1ll << 30;    // per launch: in-launch indices fit 32 bits, grid x block < 2^32

template <int V> __device__ __forceinline__ VF<V> ld_f32(const float *p) {
  typedef typename VecType<V>::T T;
  const T t = *as_global(reinterpret_cast<const T *>(p));
  VF<V> r;
  __builtin_memcpy(&r, &t, sizeof(T));
  return r;
}
template <int V> __device__ __forceinline__ void st_f32(float *p, const VF<V> &v) {
  typedef typename VecType<V>::T T;
  T t;
  __builtin_memcpy(&t, &v, sizeof(T));
  *as_global(reinterpret_cast<T *>(p)) = t;
}

template <int V> __device__ __forceinline__ void minmax(const VF<V> &x, float &mn, float &mx) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    mn = fminf(mn, x.v[i]);
    mx = fmaxf(mx, x.v[i]);
  }
}

// the q8 code of one element: rint((x - mn) * inv), round-half-even (v_rndne_f32), each operation rounded once, its low 8 bits
__device__ __forceinline__ uint32_t q8_code(float x, float mn, float inv) {
  const float d = x - mn;
  const float q = __builtin_rintf(d * inv);
  return (uint32_t)(int32_t)q & 0xFFu;
}

// the V codes of a slot as one store of V bytes; element i in byte i
template <int V> __device__ __forceinline__ void st_codes(char *p, const VF<V> &x, float mn, float inv) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < V; ++i) c |= q8_code(x.v[i], mn, inv) << (8 * i);
  *as_global(reinterpret_cast<typename Q8Codes<V>::T *>(p)) = (typename Q8Codes<V>::T)c;
}

// slots of a row a lane keeps in registers, by its group: G == 1 holds dims <= 4, dim 3 being three one-element slots of one lane
template <int G> constexpr int slots_in_registers() { return G == 64 ? kQSlots : (G == 1 ? 3 : 1); }

// The slots of a float32 row that ONE lane of the row's G-lane group owns: slot lane + k * G, k = 0, 1, ...  The first
// slots_in_registers<G>() of them stay in registers between the passes; what lies beyond (only a 64-lane group has any) is read
// again by every pass.
template <int V, int G> struct RowSlots {
  static constexpr int S = slots_in_registers<G>();
  VF<V> x[S];

  // pass one: f(value) per slot, in increasing k, then the tail in increasing slot.  A row that is not live touches no memory.
  template <class F> __device__ __forceinline__ void load(const float *srow, int nslots, int lane, bool live, F f) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      x[k] = vzero<V>();
      const int slot = lane + k * G;
      if (live && slot < nslots) {
        x[k] = ld_f32<V>(srow + (int64_t)slot * V);
        f(x[k]);
      }
    }
    if constexpr (G == 64) {
      if (live)
        for (int slot = lane + S * G; slot < nslots; slot += G) f(ld_f32<V>(srow + (int64_t)slot * V));
    }
  }

  // a later pass of a LIVE row: f(slot, value) in the order of pass one, the kept slots from registers
  template <class F> __device__ __forceinline__ void again(const float *srow, int nslots, int lane, F f) const {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int slot = lane + k * G;
      if (slot < nslots) f(slot, x[k]);
    }
    if constexpr (G == 64) {
      for (int slot = lane + S * G; slot < nslots; slot += G) // beyond the register cap: the row's tail is read again
        f(slot, ld_f32<V>(srow + (int64_t)slot * V));
    }
  }
};

// One float32 row at srow -> one q8 row at drow (dim codes, then scale and bias), by the row's G-lane group; bit for bit what
// quantized::embedding_bag_byte_prepack writes (fcp_hip.h spells the arithmetic out).  EVERY lane of a wave calls it: lanes
// of a group that is not live take part in the exchanges and touch no memory.  Codes leave V bytes at a time, scale and
// bias as one pair at the alignment the format allows (Q8Pair<V>), from the group's first lane.
template <int V, int G> __device__ __forceinline__ void quantize_row(char *drow, const float *srow, int dim, int lane, bool live) {
  const int nslots = dim / V;
  RowSlots<V, G> r;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  r.load(srow, nslots, lane, live, [&](const VF<V> &x) { minmax<V>(x, mn, mx); });
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1) { // the group's min and max in every lane: order-free, no LDS
    mn = fminf(mn, __shfl_xor(mn, m, 64));
    mx = fmaxf(mx, __shfl_xor(mx, m, 64));
  }
  const float range = mx - mn;
  const float scale = range / 255.0f;
  const float inv = 255.0f / (range + 1e-8f);
  if (!live) return;
  r.again(srow, nslots, lane, [&](int slot, const VF<V> &x) { st_codes<V>(drow + (int64_t)slot * V, x, mn, inv); });
  if (lane == 0) {
    const uint64_t pair = (uint64_t)__float_as_uint(scale) | ((uint64_t)__float_as_uint(mn) << 32);
    *(FCP_GLOBAL typename Q8Pair<V>::T *)(drow + dim) = pair;
  }
}

inline dim3 blocks_for(int64_t threads) { return dim3((uint32_t)((threads + FCP_BLOCK_THREADS - 1) / FCP_BLOCK_THREADS)); }

// V and G of a dim: fcp_formats.h has the two rules (the host-only units read them too)
using fcpf::group_of;
using fcpf::vec_of;

// The host's dispatch on a template argument: f(std::integral_constant<int, N>{}) for the N of Ns... that n equals — the caller
// writes [&](auto N) { ... decltype(N)::value ... }.  n is one of them by construction (group_of, vec_of).
template <int... Ns, class F> void with_one_of(int n, F f) { (void)((n == Ns && (f(std::integral_constant<int, Ns>{}), true)) || ...); }
template <class F> void with_group(int g, F f) { with_one_of<1, 2, 4, 8, 16, 32, 64>(g, f); }
template <class F> void with_vec(int vec, F f) { with_one_of<4, 2, 1>(vec, f); }

using fcpf::kind_name;

} // namespace
