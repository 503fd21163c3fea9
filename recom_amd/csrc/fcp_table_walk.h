// fcp_table_walk.h — what the units that walk float32 table rows share: fcp_convert.hip (fcp_quantize_q8_kernel), fcp_table_rows.hip
// (fcp_update_q8_kernel) and fcp_table_audit.hip (fcp_table_audit_kernel) handle a row by the same power-of-two lane group, with
// the same V-element slots and the same in-register cap, and form q8 codes by the same arithmetic.  One place for the constants,
// the slot loads / stores and the group rule, so the three cannot drift apart.  Everything lives in an unnamed namespace, as in
// fcp_fused_bodies.h: each translation unit gets its own copy.  The includer switches contraction off (#pragma clang fp
// contract(off)) BEFORE it includes this header, and includes fcp_fused_bodies.h ahead of the pragma: q8_code rounds every
// operation once, and the bodies keep the mode they have in every other unit.
#pragma once
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

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

inline dim3 blocks_for(int64_t threads) { return dim3((uint32_t)((threads + FCP_BLOCK_THREADS - 1) / FCP_BLOCK_THREADS)); }

// V: the largest of 4 | 2 | 1 that divides dim
inline int vec_of(int32_t dim) { return dim % 4 == 0 ? 4 : dim % 2 == 0 ? 2 : 1; }
// G, the lanes that share a row: 1 for dims <= 4, else the power of two that holds the row's dim / V slots, at most 64
inline int group_of(int dim, int vec) {
  int g = 1;
  if (dim > 4)
    while (g < dim / vec && g < 64) g <<= 1;
  return g;
}
inline const char *kind_name(int32_t k) { return k == FCP_TAB_F32 ? "float32" : k == FCP_TAB_BF16 ? "bf16" : k == FCP_TAB_F16 ? "fp16" : "q8"; }

} // namespace
