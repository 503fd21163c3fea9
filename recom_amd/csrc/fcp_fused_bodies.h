// fcp_fused_bodies.h — the device code the fused kernels are made of: loads / stores, the id path, the dense body and the
// ragged body, each a template over the variant it is instantiated for (FcpVariant, fcp_internal.h).  Shared by the
// translation units that instantiate kernels from it, one per variant: fcp_kernels.hip (the float32 matrix: dense, ragged,
// hybrid), fcp_weighted.hip (the weighted ragged kernels, which do not fit the 64-VGPR budget of the tuned instantiations and
// are launched only for plans that need them), fcp_narrow.hip, fcp_tables16.hip, fcp_tables_q8.hip and fcp_tables_mixed.hip;
// what their kernels and launchers share on top of the bodies is fcp_fused_launch.h.  Everything lives in an unnamed
// namespace: each translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/fcp_hip.h"
#include <hip/hip_ext.h>
#include "fcp_internal.h"

namespace {

// Pointers that travel through LDS records (or are computed from them) lose their
// address space: hipcc then emits FLAT loads, which probe the LDS aperture as well
// and complete out of order.  Every such access is cast back to the global address
// space so that it becomes a plain global_load / global_store.
#define FCP_GLOBAL __attribute__((address_space(1)))
template <typename T> __device__ __forceinline__ const FCP_GLOBAL T *as_global(const T *p) {
  return (const FCP_GLOBAL T *)(p);
}
template <typename T> __device__ __forceinline__ FCP_GLOBAL T *as_global(T *p) { return (FCP_GLOBAL T *)(p); }
// Plan data and the request's descriptors are read-only for the lifetime of a launch: the constant
// address space lets the compiler use scalar loads for wave-uniform addresses (slot map, span list).
#define FCP_CONST __attribute__((address_space(4)))
template <typename T> __device__ __forceinline__ const FCP_CONST T *as_const(const T *p) { return (const FCP_CONST T *)(p); }

template <int V> struct VecType;
template <> struct VecType<4> { typedef float __attribute__((ext_vector_type(4))) T; };
template <> struct VecType<2> { typedef float __attribute__((ext_vector_type(2))) T; };
template <> struct VecType<1> { typedef float T; };

template <int V> struct alignas(4 * V) VF { float v[V]; };
template <int V> struct alignas(4 * V) VU { uint32_t v[V]; }; // the same slot as bit patterns

template <int V> __device__ __forceinline__ VF<V> vzero() {
  VF<V> r;
#pragma unroll
  for (int i = 0; i < V; ++i) r.v[i] = 0.0f;
  return r;
}

// Output rows are written once and consumed by a later kernel: non-temporal stores
// (measured on S2: 34.3 -> 30.5 us per request).  Table rows are read with the DEFAULT
// cache policy: streaming them (non-temporal loads) changes nothing on S2 (1M-row tables,
// uniform ids) but costs the reference's models E / F 4.5 us per request — their ~1000
// bucketize / hash tables of ~100 rows are re-read by every row and belong in L2.
// (r6) A per-column choice — non-temporal reads for tables far beyond an XCD's L2, default policy for the small hot ones —
// was built and measured too, because a bare gather probe reads 11 % faster with `nt` at every row size (53.7 against 48.5
// G rows/s): inside the fused kernels it moved nothing (S2 27.39 against 27.35 us, model F 12.9 / 12.9, RAGGED -0.5 us in
// one encoding, +0 in the other: profiles/r06_streamed_table_reads_negative.txt) and was taken out again.
// Write-through form (`sc1 nt`: the line leaves the XCD's L2 at once instead of at the kernel boundary) for
// outputs larger than the L2s can hold — S2's 61 MB: 28.4 vs 29.0 us per request; outputs that FIT the
// caches (DLRM 3.5 MB, models E / F 16 MB) lose with it (DLRM 4.7 -> 5.9 us, F 14.7 -> 17.7 us): the host
// picks per launch (FcpLaunch::store_through, profiles/r02_store_policy.txt).  Inline asm: the compiler has
// no builtin for the sc1 bit; the s_nop covers the hazard "VMEM store of more than 64 bits followed by a
// VALU write of its data registers", which the hazard recogniser cannot see inside asm.
__device__ __forceinline__ void st_through(FCP_GLOBAL VecType<4>::T *p, VecType<4>::T t) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_through(FCP_GLOBAL VecType<2>::T *p, VecType<2>::T t) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1 nt" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_through(FCP_GLOBAL VecType<1>::T *p, VecType<1>::T t) {
  asm volatile("global_store_dword %0, %1, off sc1 nt" ::"v"(p), "v"(t) : "memory");
}

// (r6) Third policy, PLAIN stores (default cache policy), for an arena that is the one the plan's previous request (or the
// one before it) wrote: TF's allocate_output(2) hands a serving loop the block it just freed
// (feature_column_process_op_gpu.cu.cc:107-111), so an output line is rewritten one request later — 61 MB of output + 86 MB
// of table lines in between stay within the 256-MiB Infinity Cache, and rewriting a resident line is cheaper than streaming
// it past the caches: S2 27.2 us against 27.9 (nt) / 28.0 (sc1 nt) with one arena, 28.0 / 28.2 / 28.2 with two; with three
// or more arenas plain stores LOSE (31.1 against 28.1): profiles/r06_arena_reuse_store_policy.txt.  The host decides per
// request (FcpLaunch::store_through bit 2, fill_launch).
#define FCP_ST_THROUGH 1
#define FCP_ST_PLAIN 4
// The non-temporal form in inline asm as well: written as `if (plain) *p = t; else __builtin_nontemporal_store(t, p);` the
// compiler MERGED the two stores into one and dropped the nontemporal hint with it (the first build of the three-policy
// st_out had exactly two store instructions per row: `sc1 nt` and plain — every "nt" request wrote with plain stores,
// RAGGED with six arenas 27.5 -> 29.3 us, profiles/r06_arena_reuse_kernel_traces.txt).
__device__ __forceinline__ void st_nt(FCP_GLOBAL VecType<4>::T *p, VecType<4>::T t) {
  asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_nt(FCP_GLOBAL VecType<2>::T *p, VecType<2>::T t) {
  asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_nt(FCP_GLOBAL VecType<1>::T *p, VecType<1>::T t) {
  asm volatile("global_store_dword %0, %1, off nt" ::"v"(p), "v"(t) : "memory");
}

template <int V> __device__ __forceinline__ void st_out(float *p, const VF<V> &v, int policy) {
  typedef typename VecType<V>::T T;
  T t;
  __builtin_memcpy(&t, &v, sizeof(T));
  if (policy & FCP_ST_THROUGH) {
    st_through(as_global(reinterpret_cast<T *>(p)), t);
    return;
  }
  if (!(policy & FCP_ST_PLAIN)) {
    st_nt(as_global(reinterpret_cast<T *>(p)), t);
    return;
  }
  *as_global(reinterpret_cast<T *>(p)) = t;
}

// ---- narrow output (fcp_narrow.hip: FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16 plans) ------------------------------------------
// A narrow element is fl16(x) of the float32 value x the float32 plan stores: ONE rounding to nearest-even, at the store.
// bf16 in integers (the high half of the pattern plus the carry of the rounding: ties to even, overflow into the exponent
// gives +-inf, float32 subnormals round like every other value, -0.0 stays -0.0; a NaN keeps its sign and becomes quiet so
// that no payload can round to inf); fp16 is the hardware conversion v_cvt_f16_f32 in the kernel's mode (round-to-nearest-
// even, denormals kept: |x| >= 65520 -> inf, gradual underflow, float32 subnormals -> +-0).
__device__ __forceinline__ uint32_t narrow_bf16(float x) {
  const uint32_t u = __float_as_uint(x);
  const uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
  return (u & 0x7FFFFFFFu) > 0x7F800000u ? ((u >> 16) | 0x40u) : r;
}
__device__ __forceinline__ uint32_t narrow_f16(float x) {
  const _Float16 h = (_Float16)x;
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  return b;
}

// The V narrow elements of a slot as one store of 2 * V bytes: dwordx2 | dword | short.
template <int V> struct NarrowType;
template <> struct NarrowType<4> { typedef uint32_t __attribute__((ext_vector_type(2))) T; };
template <> struct NarrowType<2> { typedef uint32_t T; };
template <> struct NarrowType<1> { typedef uint16_t T; };

// the same three cache policies as st_out, the hinted forms in inline asm for the same reason (st_nt above)
__device__ __forceinline__ void st_through16(FCP_GLOBAL NarrowType<4>::T *p, NarrowType<4>::T t) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1 nt" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_through16(FCP_GLOBAL NarrowType<2>::T *p, NarrowType<2>::T t) {
  asm volatile("global_store_dword %0, %1, off sc1 nt" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_through16(FCP_GLOBAL NarrowType<1>::T *p, NarrowType<1>::T t) {
  asm volatile("global_store_short %0, %1, off sc1 nt" ::"v"(p), "v"((uint32_t)t) : "memory");
}
__device__ __forceinline__ void st_nt16(FCP_GLOBAL NarrowType<4>::T *p, NarrowType<4>::T t) {
  asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_nt16(FCP_GLOBAL NarrowType<2>::T *p, NarrowType<2>::T t) {
  asm volatile("global_store_dword %0, %1, off nt" ::"v"(p), "v"(t) : "memory");
}
__device__ __forceinline__ void st_nt16(FCP_GLOBAL NarrowType<1>::T *p, NarrowType<1>::T t) {
  asm volatile("global_store_short %0, %1, off nt" ::"v"(p), "v"((uint32_t)t) : "memory");
}

// p: BYTE address of the slot's first narrow element (2 * V-byte aligned); out_kind: FCP_OUT_BF16 | FCP_OUT_F16, the same
// for every wave of the launch (a kernel argument)
template <int V> __device__ __forceinline__ void st_out_narrow(char *p, const VF<V> &v, int policy, int out_kind) {
  typedef typename NarrowType<V>::T T;
  uint32_t h[V];
  if (out_kind == FCP_OUT_BF16) {
#pragma unroll
    for (int i = 0; i < V; ++i) h[i] = narrow_bf16(v.v[i]);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) h[i] = narrow_f16(v.v[i]);
  }
  T t;
  if constexpr (V == 4) {
    t.x = h[0] | (h[1] << 16);
    t.y = h[2] | (h[3] << 16);
  } else if constexpr (V == 2) {
    t = h[0] | (h[1] << 16);
  } else {
    t = (uint16_t)h[0];
  }
  FCP_GLOBAL T *g = as_global(reinterpret_cast<T *>(p));
  if (policy & FCP_ST_THROUGH) {
    st_through16(g, t);
    return;
  }
  if (!(policy & FCP_ST_PLAIN)) {
    st_nt16(g, t);
    return;
  }
  *g = t;
}

// Row `off` of a table of `spr` slots (of V floats) per row whose lane-specific base is `tb`: one v_mad_u64_u32
// (row x slots per row, 64-bit: a table may be of any size, rows < 2^32 - 3) + one global_load.
template <int V> __device__ __forceinline__ VF<V> ld_slot32(const float *tb, uint32_t off);
template <int V> __device__ __forceinline__ VF<V> ld_slot(const float *tb, uint32_t off, uint32_t spr) {
  typedef typename VecType<V>::T T;
  const FCP_GLOBAL T *g = as_global(reinterpret_cast<const T *>(tb)) + (uint64_t)off * spr;
  T t = *g;
  VF<V> r;
  __builtin_memcpy(&r, &t, sizeof(T));
  return r;
}
// The same for a PRE-SCALED slot offset (row x slots per row < 2^32 - 3, known for the whole plan: FcpLaunch::store_through
// bit 1 clear): one v_lshl_add_u64 + one global_load — what the dense kernel uses whenever every table allows it
// (S2: 0.15-0.25 us per request against the 64-bit multiply-add, profiles/r03_row_index_ab.txt).
template <int V> __device__ __forceinline__ VF<V> ld_slot32(const float *tb, uint32_t off) {
  typedef typename VecType<V>::T T;
  const FCP_GLOBAL T *g = as_global(reinterpret_cast<const T *>(tb)) + off;
  T t = *g;
  VF<V> r;
  __builtin_memcpy(&r, &t, sizeof(T));
  return r;
}

// ---- 16-bit tables (fcp_tables16.hip: FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16 plans) -----------------------------------
// A table element is 2 bytes and widens to float32 EXACTLY, so the plan computes what the float32 plan computes on the
// widened tables.  bf16 in integers (the pattern moves to the high half: a NaN keeps sign and payload through a copy);
// fp16 is the hardware conversion v_cvt_f32_f16 in the kernel's mode (16-bit denormals kept: subnormals widen exactly, a
// NaN becomes some NaN).  A slot is still V elements: one load of 2 * V bytes — dwordx2 | dword | ushort (NarrowType<V>).
// `tab_kind` (FCP_TAB_BF16 | FCP_TAB_F16) is the same for every wave of the launch (a kernel argument).
template <int V> __device__ __forceinline__ VF<V> widen16(typename NarrowType<V>::T t, int tab_kind) {
  uint32_t w[(V + 1) / 2];
  if constexpr (V == 4) {
    w[0] = t.x;
    w[1] = t.y;
  } else {
    w[0] = t;
  }
  VF<V> r;
  if (tab_kind == FCP_TAB_BF16) {
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = __uint_as_float((i & 1) ? (w[i / 2] & 0xFFFF0000u) : (w[i / 2] << 16));
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const uint16_t b = (uint16_t)((i & 1) ? (w[i / 2] >> 16) : w[i / 2]);
      _Float16 h;
      __builtin_memcpy(&h, &b, 2);
      r.v[i] = (float)h;
    }
  }
  return r;
}
// The three loaders in their 16-bit forms.  `tb`: the lane-specific base as a BYTE address (table + 2 * element offset);
// the slot offset is scaled by the slot's 2 * V bytes in 64 bits, as the float32 forms scale by 4 * V.
template <int V> __device__ __forceinline__ VF<V> ld_slot16(const char *tb, uint32_t off, uint32_t spr, int tab_kind) {
  typedef typename NarrowType<V>::T T;
  const FCP_GLOBAL T *g = as_global(reinterpret_cast<const T *>(tb)) + (uint64_t)off * spr;
  return widen16<V>(*g, tab_kind);
}
template <int V> __device__ __forceinline__ VF<V> ld_slot32_16(const char *tb, uint32_t off, int tab_kind) {
  typedef typename NarrowType<V>::T T;
  const FCP_GLOBAL T *g = as_global(reinterpret_cast<const T *>(tb)) + off;
  return widen16<V>(*g, tab_kind);
}

// ---- 8-bit row-quantised tables (fcp_tables_q8.hip: FCP_FLAG_TABLES_Q8 plans) -----------------------------------------------
// A table row is dim uint8 codes, then a float32 scale, then a float32 bias, rows back to back: dim + 8 bytes.  An element is
// the float32 value fma(float(code), scale, bias) — the product exact (8 x 24 bits), the sum rounded once: one v_fma_f32,
// written out, not left to contraction.  A slot is still V elements: one load of V code bytes —
// dword | ushort | ubyte — plus the row's scale and bias, which lie at a multiple of V bytes (V divides dim and 8) and of no
// more: the pair is declared with that alignment and the compiler forms the loads this target allows for it.
template <int V> struct Q8Pair;
template <> struct Q8Pair<4> { typedef uint64_t T __attribute__((aligned(4))); };
template <> struct Q8Pair<2> { typedef uint64_t T __attribute__((aligned(2))); };
template <> struct Q8Pair<1> { typedef uint64_t T __attribute__((aligned(1))); };
template <int V> struct Q8Codes;
template <> struct Q8Codes<4> { typedef uint32_t T; };
template <> struct Q8Codes<2> { typedef uint16_t T; };
template <> struct Q8Codes<1> { typedef uint8_t T; };
struct Q8Raw {
  uint32_t codes; // V code bytes, element i in byte i
  uint64_t pair;  // scale in the low dword, bias in the high one
};
// codes: BYTE address of the lane's V codes (row base + element offset); sb: byte address of the row's scale (row base + dim)
template <int V> __device__ __forceinline__ Q8Raw ld_q8_raw(const char *codes, const char *sb) {
  typedef typename Q8Codes<V>::T T;
  Q8Raw r;
  r.codes = *as_global(reinterpret_cast<const T *>(codes));
  r.pair = *(const FCP_GLOBAL typename Q8Pair<V>::T *)(sb);
  return r;
}
// element i: one v_fma_f32, by name — neither contraction nor the vectoriser has a say in how this value is rounded.
// What that costs: the compiler may not pair two elements into a v_pk_fma_f32 (as fused, half the issue slots), and it
// schedules the statement without seeing inside it.  These kernels wait on table reads, not on the VALU.
__device__ __forceinline__ float dequant_q8(const Q8Raw &w, int i) {
  const float code = (float)((w.codes >> (8 * i)) & 0xFFu);
  float x;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(x) : "v"(code), "v"(__uint_as_float((uint32_t)w.pair)), "v"(__uint_as_float((uint32_t)(w.pair >> 32))));
  return x;
}
template <int V> __device__ __forceinline__ VF<V> ld_q8(const char *codes, const char *sb) {
  const Q8Raw w = ld_q8_raw<V>(codes, sb);
  VF<V> r;
#pragma unroll
  for (int i = 0; i < V; ++i) r.v[i] = dequant_q8(w, i);
  return r;
}
// The loaders in their 8-bit forms.  `tb`: the lane-specific base as a BYTE address (table + element offset e); `tail`:
// dim - e, the distance from the lane's codes to the row's scale; `row_bytes`: dim + 8 (one v_mad_u64_u32 forms the row's
// byte offset from a parked row index).  A PRE-SCALED offset is row x the row stride in slots, (dim + 8) / V: offset x V
// is the row's byte offset, as in the float32 forms a slot offset x 4 * V is.
template <int V> __device__ __forceinline__ VF<V> ld_slot_q8(const char *tb, int tail, uint32_t off, uint32_t row_bytes) {
  const char *codes = tb + (uint64_t)off * row_bytes;
  return ld_q8<V>(codes, codes + tail);
}
template <int V> __device__ __forceinline__ VF<V> ld_slot32_q8(const char *tb, int tail, uint32_t off) {
  const char *codes = tb + (uint64_t)off * V;
  return ld_q8<V>(codes, codes + tail);
}
// Blob tensors are only guaranteed 4-byte aligned (ConcatInputs packs bytes
// back to back, concat_inputs_ops.cc:52-60): payloads are read dword by dword,
// 8-byte ids as two dwords.
template <int V> __device__ __forceinline__ VF<V> ld_blob_f32(const char *p) {
  VF<V> r;
  const FCP_GLOBAL float *q = as_global(reinterpret_cast<const float *>(p));
#pragma unroll
  for (int i = 0; i < V; ++i) r.v[i] = q[i];
  return r;
}

__device__ __forceinline__ int64_t ld_i64_a4(const char *p) {
  const FCP_GLOBAL uint32_t *q = as_global(reinterpret_cast<const uint32_t *>(p));
  const uint32_t lo = q[0], hi = q[1];
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// cuda_emitter.cc:233-247 — r+1 = number of boundaries <= value.
template <typename P> __device__ __forceinline__ int bucketize(P b, int n, float value) {
  int l = 0, r = n - 1;
  while (l <= r) {
    const int mid = (l + r) >> 1;
    if (value < b[mid]) {
      r = mid - 1;
    } else {
      l = mid + 1;
    }
  }
  return r + 1;
}

// The same count for (nearly) evenly spaced boundaries — the reference's bucketized columns use
// 0, 5, ..., 495 (examples/python/microbenchmark.py:46): guess the bucket from the spacing, read the two
// boundaries that bracket it (independent reads, one round trip) and accept the guess only if
// b[g-1] <= value < b[g]; anything else (rounding at a boundary, NaN, uneven spacing) runs the search.
// Exact for every input by construction; ~2 reads instead of log2(n) dependent ones.
template <typename P> __device__ __forceinline__ int bucketize_fast(P b, int n, float b0, float inv, float value) {
  float t = (value - b0) * inv;
  t = fminf(fmaxf(t, -1.0f), (float)n); // NaN -> -1
  const int g = min(max((int)floorf(t) + 1, 0), n);
  const float below = b[max(g - 1, 0)], above = b[min(g, n - 1)];
  const bool ok = (g == 0 || !(value < below)) && (g == n || value < above);
  if (ok) return g;
  return bucketize(b, n, value);
}

// Boundaries that are REPRODUCIBLE as fma(i, step, b0) (checked bit for bit when the plan is created):
// the same guess-and-verify, and the fallback search, on computed boundaries — the array is never read.
// (Reading it made every block of a launch hit the same few cache lines at once: 2.3 us of queueing on
// one L2 channel at the head of an S2 launch.)
__device__ __forceinline__ int bucketize_arith(int n, float b0, float inv, float step, float value) {
  float t = (value - b0) * inv;
  t = fminf(fmaxf(t, -1.0f), (float)n); // NaN -> -1
  const int g = min(max((int)floorf(t) + 1, 0), n);
  const float below = __builtin_fmaf((float)(g - 1), step, b0), above = __builtin_fmaf((float)g, step, b0);
  if ((g == 0 || !(value < below)) && (g == n || value < above)) return g;
  int l = 0, r = n - 1;
  while (l <= r) {
    const int mid = (l + r) >> 1;
    if (value < __builtin_fmaf((float)mid, step, b0)) {
      r = mid - 1;
    } else {
      l = mid + 1;
    }
  }
  return r + 1;
}

constexpr uint32_t kNoRow = 0xFFFFFFFFu;    // "this id contributes nothing" (another rank's row, or past the end of a bag)
constexpr uint32_t kFiltered = 0xFFFFFFFEu; // dropped by the column's id filter: contributes nothing AND does not count in a mean
constexpr uint32_t kBadRow = 0xFFFFFFFDu;   // an id outside [0, vocab): reads as zeros (and can be told from kNoRow when it is counted late)
__device__ __forceinline__ bool is_row(uint32_t off) { return off < kBadRow; }

// One column of the span, staged in LDS by the block: the static record VERBATIM (its six 16-byte words go
// from the load straight to LDS: nothing is re-packed, few registers live) plus what the request's dynamic
// record turns into.
struct alignas(16) LdsCol : FcpColStatic { // 64 + 32 = 96 bytes
  const char *ids;            // id / value stream of this request
  const int32_t *csr;         // CSR offsets of this request (blob or arena scratch), or — L.seg_search — the segment ids
  int64_t out_base;           // byte offset in the arena of element (0,0)
  int32_t out_stride;
  union {
    int32_t nnz;              // lookup forms: number of ids
    int32_t inner;            // BatchColReduction: rows reduced per output row
  };
};
static_assert(sizeof(LdsCol) == 96 && sizeof(FcpColStatic) == 64, "column records: 64 static + 32 derived bytes");

// The scalars of the argument block a body uses, fetched up front in ONE batch of scalar loads and
// pinned there (the empty asm keeps the compiler from sinking each load next to its first use, which
// made a string of separate scalar-cache round trips at the head of every block).
struct Hot {
  const FCP_CONST uint32_t *slot_map, *span_list;
  const FCP_CONST FcpColStatic *cols;
  const FCP_CONST FcpColDyn *dyn;
  const char *blob;
  char *arena;
  unsigned long long *bad_ids;
  const float *zeros;
  int64_t csr_arena_off;
  int32_t n_groups, rank, world, seg_search, store_through;
  FcpGroupLaunch g0;
};

__device__ __forceinline__ Hot load_hot(const FcpLaunch &L) {
  Hot h;
  h.slot_map = as_const(L.slot_map);
  h.span_list = as_const(L.span_list);
  h.cols = as_const(L.cols);
  h.dyn = as_const(L.dyn);
  h.blob = L.blob;
  h.arena = L.arena;
  h.bad_ids = L.bad_ids;
  h.zeros = L.zeros;
  h.csr_arena_off = L.csr_arena_off;
  h.n_groups = L.n_groups;
  h.rank = L.shard_rank;
  h.world = L.shard_world;
  h.seg_search = L.seg_search;
  h.store_through = L.store_through;
  h.g0 = L.groups[0];
  asm volatile("" : "+s"(h.slot_map), "+s"(h.span_list), "+s"(h.cols), "+s"(h.dyn), "+s"(h.blob), "+s"(h.arena),
               "+s"(h.bad_ids), "+s"(h.csr_arena_off), "+s"(h.zeros));
  asm volatile("" : "+s"(h.n_groups), "+s"(h.rank), "+s"(h.world), "+s"(h.seg_search), "+s"(h.store_through), "+s"(h.g0.rows), "+s"(h.g0.nslots),
               "+s"(h.g0.nsp8), "+s"(h.g0.block_begin), "+s"(h.g0.slot_map_off), "+s"(h.g0.span_list_off), "+s"(h.g0.nlist));
  return h;
}

// A column record as unconditional 16-byte loads (field-by-field access let the compiler wait
// for `flags` before it asked for the rest: two or three dependent round trips in phase 0).
template <typename T> __device__ __forceinline__ T ld_rec(const FCP_CONST T *p) {
  static_assert(sizeof(T) % 16 == 0, "column records are whole 16-byte words");
  typedef uint32_t __attribute__((ext_vector_type(4))) U4;
  const FCP_CONST U4 *g = reinterpret_cast<const FCP_CONST U4 *>(p);
  U4 w[sizeof(T) / 16];
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 16; ++i) w[i] = g[i];
  T r;
  __builtin_memcpy(&r, w, sizeof(T));
  return r;
}

// Phase 0 of both bodies for one column: static record -> LDS word by word, then the derived part.
// (For a PASSTHROUGH column the "table" is its payload in the blob.)
__device__ __forceinline__ void stage_col(const Hot &L, LdsCol *dst, const FCP_CONST FcpColStatic *gs,
                                          const FCP_CONST FcpColDyn *gd) {
  typedef uint32_t __attribute__((ext_vector_type(4))) U4;
  const FCP_CONST U4 *ws = reinterpret_cast<const FCP_CONST U4 *>(gs);
  const FCP_CONST U4 *wd = reinterpret_cast<const FCP_CONST U4 *>(gd);
  U4 s0 = ws[0], s1 = ws[1], s2 = ws[2], s3 = ws[3];
  const U4 d0 = wd[0], d1 = wd[1], d2 = wd[2];
  FcpColDyn cd;
  {
    U4 w[3] = {d0, d1, d2};
    __builtin_memcpy(&cd, w, sizeof(cd));
  }
  const uint32_t flags = s2.x; // word 2: flags, n_boundaries, seg_stride, bnd_b0 (offset 32)
  const char *ids = L.blob + cd.ids_off;
  if (FCP_F_FORM(flags) == FCP_FORM_PASSTHROUGH) { // word 0: table, boundaries
    const uint64_t t = (uint64_t)reinterpret_cast<uintptr_t>(ids);
    s0.x = (uint32_t)t;
    s0.y = (uint32_t)(t >> 32);
  }
  U4 *out = reinterpret_cast<U4 *>(dst);
  out[0] = s0;
  out[1] = s1;
  out[2] = s2;
  out[3] = s3;
  const unsigned segkind = FCP_F_SEGKIND(flags);
  dst->ids = ids;
  dst->csr = (segkind == FCP_SEG_CSR_I32 || (segkind != FCP_SEG_NONE && L.seg_search))
                 ? reinterpret_cast<const int32_t *>(L.blob + cd.seg_off)
             : segkind != FCP_SEG_NONE ? reinterpret_cast<const int32_t *>(L.arena + L.csr_arena_off) + cd.csr_base
                                       : nullptr;
  dst->out_base = cd.out_base;
  dst->out_stride = cd.out_stride;
  dst->nnz = FCP_F_FORM(flags) == FCP_FORM_BATCH_COL_REDUCTION ? cd.inner : cd.nnz;
}
static_assert(offsetof(FcpColStatic, flags) == 32 && offsetof(FcpColStatic, table) == 0, "stage_col reads the record by word");

// the interval test of Addons>SelectValue / Addons>GatherIndiceValue /
// Addons>GatherValueGenIndice (select_value_ops.cc:33-56 and siblings), fused: closed intervals,
// `lo <= id && id <= hi` (the reference's `||` accepts everything).  Returns the id the
// lookup sees and, next to it, whether the filter removed it — a flag of its own, not a reserved id: every
// int64 is a legal id, interval end and substitute (INT64_MIN inside a filter's interval is kept, reaches the
// lookup, reads zeros and counts in a mean).  Out of line and fed from the per-column side table
// (FcpLaunch::xforms) on purpose: columns without a transform — nearly all — pay one compare, no registers
// and no record bytes for it (inlined with the intervals in the column record it cost S2 2 us of 29: 76 VGPRs).
// The pair comes back in registers (three VGPRs), nothing goes through memory.
struct XformedId {
  int64_t id;
  uint32_t dropped;
};

// ---- Fingerprint64 of a short byte string (FarmHash farmhashna::Hash64, lengths 1..32; TensorFlow's
// StringToHashBucketFast, core/kernels/string_to_hash_bucket_fast_op.h) -----------------------------------
// The string is the decimal form of an int64 (at most 20 bytes), kept in three little-endian 64-bit words
// held in registers (no arrays: nothing may end up in scratch memory).
struct Str24 {
  uint64_t w0, w1, w2;
};
__device__ __forceinline__ uint64_t fetch64(const Str24 &s, int o) { // unaligned little-endian read at byte o (o <= 15)
  const int i = o >> 3, sh = (o & 7) * 8;
  const uint64_t lo = (i == 0 ? s.w0 : s.w1) >> sh;
  return sh ? lo | ((i == 0 ? s.w1 : s.w2) << (64 - sh)) : lo;
}
__device__ __forceinline__ uint64_t rot64(uint64_t v, int sh) { return sh ? (v >> sh) | (v << (64 - sh)) : v; }
__device__ __forceinline__ uint64_t hash_len16(uint64_t u, uint64_t v, uint64_t mul) {
  uint64_t a = (u ^ v) * mul;
  a ^= a >> 47;
  uint64_t b = (v ^ a) * mul;
  b ^= b >> 47;
  return b * mul;
}
__device__ uint64_t fingerprint64_decimal(int64_t value) {
  constexpr uint64_t k0 = 0xc3a5c85c97cb3127ull, k1 = 0xb492b66fbe98f273ull, k2 = 0x9ae16a3b2f90404full;
  // AsString of an integer: decimal digits, most significant first, '-' for negatives, no padding
  const uint64_t mag = value < 0 ? 0ull - (uint64_t)value : (uint64_t)value;
  int n = 1;
  for (uint64_t p = 10; n < 20 && mag >= p; p *= 10) ++n; // 10^19 < 2^64: p never overflows before n reaches 20
  const int neg = value < 0 ? 1 : 0;
  Str24 s = {neg ? (uint64_t)'-' : 0ull, 0ull, 0ull};
  uint64_t m = mag;
  for (int k = 0; k < n; ++k) { // least significant digit first, written at its final position
    const int pos = neg + n - 1 - k;
    const uint64_t v = (uint64_t)('0' + (int)(m % 10)) << ((pos & 7) * 8);
    m /= 10;
    if (pos < 8) s.w0 |= v;
    else if (pos < 16) s.w1 |= v;
    else s.w2 |= v;
  }
  n += neg;
  const uint64_t len = (uint64_t)n;
  if (n <= 16) {
    if (n >= 8) {
      const uint64_t mul = k2 + len * 2, a = fetch64(s, 0) + k2, b = fetch64(s, n - 8);
      return hash_len16(rot64(b, 37) * mul + a, (rot64(a, 25) + b) * mul, mul);
    }
    if (n >= 4) {
      const uint64_t mul = k2 + len * 2, a = (uint32_t)s.w0;
      return hash_len16(len + (a << 3), (uint32_t)(s.w0 >> ((n - 4) * 8)), mul);
    }
    const uint8_t a = (uint8_t)s.w0, b = (uint8_t)(s.w0 >> ((n >> 1) * 8)), c = (uint8_t)(s.w0 >> ((n - 1) * 8));
    const uint32_t y = (uint32_t)a + ((uint32_t)b << 8), z = (uint32_t)n + ((uint32_t)c << 2);
    uint64_t h = (uint64_t)y * k2 ^ (uint64_t)z * k0;
    h ^= h >> 47;
    return h * k2;
  }
  const uint64_t mul = k2 + len * 2, a = fetch64(s, 0) * k1, b = fetch64(s, 8), c = fetch64(s, n - 8) * mul,
                 e = fetch64(s, n - 16) * k2;
  return hash_len16(rot64(a + b, 43) + rot64(c, 30) + e, a + rot64(b + k2, 18) + c, mul);
}

__device__ __attribute__((noinline)) XformedId apply_xform(uint32_t xform, const FcpXform *xf, int64_t id) {
  const FCP_GLOBAL FcpXform *x = as_global(xf);
  if (xform & FCP_XFORM_HASH_BIT) id = (int64_t)(fingerprint64_decimal(id) % (uint64_t)x->hash_buckets);
  const unsigned mode = xform & 3u;
  if (mode == FCP_XFORM_NONE) return {id, 0u};
  bool in = id >= x->lo0 && id <= x->hi0;
  const int n = (int)((xform & ~FCP_XFORM_HASH_BIT) >> 2);
  for (int i = 1; i < n && !in; ++i) {
    const FCP_GLOBAL int64_t *e = as_global(x->extra) + 2 * (i - 1);
    in = id >= e[0] && id <= e[1];
  }
  if (in) return {id, 0u};
  if (mode == FCP_XFORM_FILTER) return {id, 1u};
  return {x->sub, 0u};
}

// The index expression the reference inlines per column (EmitInputInline,
// cuda_emitter.cc:1769-1949: raw int32 / int64 ids, or Bucketize(float value)),
// the range check and the row shard, folded into ONE number per id: the (local) row
// of the table (< 2^32 - 3 rows per table or shard is checked when the plan is created;
// the byte offset is formed in 64 bits where the row is read), or kNoRow.  Ids outside [0, vocab) read as zeros (the
// reference reads out of bounds, TF-GPU GatherV2 returns zeros); under row
// sharding an id owned by another rank contributes nothing here.
template <int V, bool SHARDED>
__device__ __forceinline__ uint32_t slot_offset_from_raw(const LdsCol &c, const FcpXform *xf, uint32_t lo, uint32_t hi,
                                                         const float *lds_bnd, int rank, int world, bool &bad) {
  const unsigned idsrc = FCP_F_IDSRC(c.flags);
  int64_t id;
  if (idsrc == FCP_IDS_F32_BUCKETIZE) {
    const float x = __uint_as_float(lo);
    if (c.bnd_step != 0.0f) // reproducible boundaries: no reads at all
      id = bucketize_arith(c.n_boundaries, c.bnd_b0, c.bnd_inv, c.bnd_step, x);
    else if (lds_bnd)       // staged in LDS by the block; evenly spaced ones start from the guess
      id = c.bnd_inv != 0.0f ? bucketize_fast(lds_bnd, c.n_boundaries, c.bnd_b0, c.bnd_inv, x)
                             : bucketize(lds_bnd, c.n_boundaries, x);
    else
      id = c.bnd_inv != 0.0f ? bucketize_fast(as_global(c.boundaries), c.n_boundaries, c.bnd_b0, c.bnd_inv, x)
                             : bucketize(as_global(c.boundaries), c.n_boundaries, x);
  } else {
    id = idsrc == FCP_IDS_I64 ? (int64_t)(((uint64_t)hi << 32) | lo) : (int64_t)(int32_t)lo;
  }
  bad = false;
  if (c.xform) { // rare
    const XformedId x = apply_xform(c.xform, xf, id);
    if (x.dropped) return kFiltered;
    id = x.id;
  }
  bad = (uint64_t)id >= (uint64_t)c.vocab;
  if (bad) return kBadRow;
  if (SHARDED) {
    const int64_t q = id < 0x7fffffffLL ? (int64_t)((uint32_t)id / (uint32_t)world) : id / world;
    if (id - q * world != rank) return kNoRow;
    id = q;
  }
  return (uint32_t)id;
}

template <int V, bool SHARDED>
__device__ __forceinline__ uint32_t fetch_slot_offset(const LdsCol &c, const FcpXform *xf, int64_t pos, const float *lds_bnd,
                                                      int rank, int world, bool &bad) {
  const bool is64 = FCP_F_IDSRC(c.flags) == FCP_IDS_I64;
  // branch-free fetch: one code path for every id source
  const char *a = c.ids + (is64 ? 8 : 4) * pos;
  const uint32_t lo = *as_global(reinterpret_cast<const uint32_t *>(a));
  const uint32_t hi = *as_global(reinterpret_cast<const uint32_t *>(a + (is64 ? 4 : 0)));
  return slot_offset_from_raw<V, SHARDED>(c, xf, lo, hi, lds_bnd, rank, world, bad);
}

// ---- per-input table formats (fcp_tables_mixed.hip: FCP_FLAG_TABLES_PER_INPUT plans whose tables really differ) ------------
// The R reads of one lane of the dense body by the kind of its column's table (FCP_TAB_*): the three loader families above,
// each with all its R reads in flight.  `table`: the table's base; `e`: the lane's element offset in the row.  Called with a
// scalar `kind` where the wave holds one kind (the branches are then scalar), with the lane's own otherwise (three
// exec-masked sections, each skipped when no lane takes it).
template <int V, int R>
__device__ __forceinline__ void ld_rows_mixed(VF<V> (&v)[R], const uint32_t (&off)[R], int kind, const char *table, int e, int dim, bool wide) {
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = vzero<V>();
  if (kind == FCP_TAB_F32) {
    const float *tb = reinterpret_cast<const float *>(table) + e;
    const uint32_t spr = (uint32_t)(dim / V);
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (is_row(off[r])) v[r] = wide ? ld_slot<V>(tb, off[r], spr) : ld_slot32<V>(tb, off[r]);
  } else if (kind == FCP_TAB_Q8) {
    const char *tb8 = table + e; // the lane's codes in row 0; the scale dim - e behind
    const int tail = dim - e;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (is_row(off[r])) v[r] = wide ? ld_slot_q8<V>(tb8, tail, off[r], (uint32_t)dim + 8u) : ld_slot32_q8<V>(tb8, tail, off[r]);
  } else {
    const char *tb16 = table + 2 * (int64_t)e; // element offset x 2, in 64 bits
    const uint32_t spr = (uint32_t)(dim / V);
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (is_row(off[r])) v[r] = wide ? ld_slot16<V>(tb16, off[r], spr, kind) : ld_slot32_16<V>(tb16, off[r], kind);
  }
}

// Common block header: which group / span / row tile this block owns.
struct BlockPos {
  int rows, nslots, q0, row_blk, ncols;
  uint32_t first_col;
  const FCP_CONST uint32_t *map;
};

template <int RB> __device__ __forceinline__ bool locate_block(const FcpLaunch &L, const Hot &H, int bid, BlockPos &B) {
  // Every scalar a block of a one-group plan needs sits at a FIXED offset of the argument block: the
  // loads are issued together and waited for once.  (Indexing groups[g] with a searched g made a chain
  // of five dependent scalar loads, each a scalar-cache miss at launch start: 1.9 us before the first
  // column record was requested, profiles/r01_s2_block_timeline_stamps.txt "desc".)
  FcpGroupLaunch G = H.g0;
  if (H.n_groups > 1) {
    for (int k = 1; k < H.n_groups; ++k)
      if (bid >= L.groups[k].block_begin) G = L.groups[k];
  }
  B.rows = G.rows;
  B.nslots = G.nslots;
  const int nsp8 = G.nsp8;
  B.map = H.slot_map + G.slot_map_off;
  bid -= G.block_begin;
  // XCD-aware mapping: blocks with equal (bid & 7) share an XCD under the
  // round-robin dispatch; give them the same spans (same columns / tables).
  int idx, tile; // idx: position in the list of spans this launch covers
  if (nsp8 > 0) {
    const int xcd = bid & 7, j8 = bid >> 3;
    idx = (j8 % nsp8) * 8 + xcd;
    tile = j8 / nsp8;
  } else { // fewer than 8 spans: no padding to 8 (nsp8 = -nlist)
    idx = bid % (-nsp8);
    tile = bid / (-nsp8);
  }
  if (idx >= G.nlist) return false; // uniform: whole block leaves
  const int lo = G.span_list_off;
  const int span = lo >= 0 ? (int)H.span_list[lo + idx] : idx;
  B.q0 = span * FCP_WAVE;
  B.row_blk = tile * RB;
  if (B.q0 >= B.nslots || B.row_blk >= B.rows) return false;
  B.first_col = B.map[B.q0];
  B.ncols = (int)(B.map[min(B.q0 + FCP_WAVE - 1, B.nslots - 1)] - B.first_col) + 1;
  return true;
}

// ---------------------------------------------------------------------------
// Dense kernel: every column of the plan is GATHER or PASSTHROUGH (exactly one
// source row per output row) — BASELINE.json's S2 and DLRM shapes.
//
// A block owns one span (64 slots = 1 KiB of the output row) for RB = 4*R rows.
//   phase 0  the span's column records (static + dynamic, contiguous because
//            the device arrays are kept in concat order) are copied to LDS,
//            one thread per column;
//   phase 0b bucketize boundaries -> LDS (the reference stages them per block
//            too, cuda_emitter.cc:1818-1825); wave 0 assigns LDS offsets with a
//            shuffle prefix sum, columns that do not fit keep searching in L2;
//   phase 1  the block's (column, row) id pairs are fetched with one thread
//            per pair — consecutive threads take consecutive rows of one
//            column, so every id cache line is requested exactly once — turned
//            into table slot offsets and parked in LDS;
//   phase 2  every lane reads its column record and its R slot offsets from
//            LDS (broadcast reads), issues its R 16-byte table reads back to
//            back, then its R stores: 1 KiB contiguous per wave instruction,
//            straight into the concat layout.
// Without the LDS staging every lane fetched its own copy of the id and of the
// 96-byte column record: ~80 vector-memory instructions per wave and — measured
// with rocprofv3 — about half of the kernel time queueing on the same in-flight
// cache lines (profiles/r01_s2_pmc_before_lds_staging.txt).
// ---------------------------------------------------------------------------
template <int R> struct DenseLds {
  static constexpr int RB = FCP_WAVES_PER_BLOCK * R; // rows per block
  static constexpr int IDS = RB + 1;                 // padded row of the offset tile (LDS banks)
  static constexpr int BND = 1024;                   // floats of bucketize boundaries staged per block
  LdsCol col[FCP_WAVE];
  uint32_t off[FCP_WAVE * IDS];
  float bnd[BND];
};

// NARROW: the instantiation for bf16 / fp16 output plans (fcp_narrow.hip); `out_kind` (FCP_OUT_*) is launch-uniform.  Only the
// output address (2 bytes per element) and the store differ, and both sit behind `if constexpr (NARROW)`: the float32
// instantiations are the code they were.
// TAB16: the instantiation for bf16 / fp16 table plans (fcp_tables16.hip); `tab_kind` (FCP_TAB_*) is launch-uniform.  Only the
// table address (2 bytes per element) and the load differ, both behind `if constexpr (TAB16)`.  A PASSTHROUGH column's
// "table" is its float32 payload in the blob and is read as such.
// TABQ8: the instantiation for 8-bit row-quantised table plans (fcp_tables_q8.hip).  The table address and the load differ,
// and a row index is scaled by the row stride in slots, (dim + 8) / V, where the float32 plan scales by dim / V; all behind
// `if constexpr (TABQ8)`.
// TABMIX: the instantiation for plans whose tables have more than one format (fcp_tables_mixed.hip).  The kind is a fact of each
// COLUMN (FCP_F_TABKIND of its record's flags: a 64-slot span routinely holds columns of different formats), so the row stride
// that scales a row index and the loader are chosen per lane — wave-uniformly where one ballot shows that the whole wave
// holds one kind; all behind `if constexpr (TABMIX)`.
// `kind`: what NARROW and TAB16 call out_kind / tab_kind; the other variants do not read it.
template <int V, int R, bool SHARDED, FcpVariant X = FCP_VAR_F32>
__device__ __forceinline__ void dense_body(const FcpLaunch &L, int bid, char *smem, int kind = 0) {
  constexpr bool NARROW = X == FCP_VAR_NARROW, TAB16 = X == FCP_VAR_TAB16, TABQ8 = X == FCP_VAR_TABQ8, TABMIX = X == FCP_VAR_TABMIX;
  static_assert(X != FCP_VAR_WEIGHTED, "the weighted kernel is a ragged one");
  const int out_kind = kind, tab_kind = kind;
  constexpr int RB = DenseLds<R>::RB, IDS = DenseLds<R>::IDS, BND = DenseLds<R>::BND;
  DenseLds<R> &S = *reinterpret_cast<DenseLds<R> *>(smem);
  LdsCol *s_col = S.col;
  uint32_t *s_off = S.off;
  float *s_bnd = S.bnd;

  BlockPos B;
  const Hot H = load_hot(L);
  if (!locate_block<RB>(L, H, bid, B)) return;
  const int tid = threadIdx.x;
  const int lane = tid & (FCP_WAVE - 1);
  const int wave = tid >> 6;
  const int q = B.q0 + lane;
  const uint32_t my_col = B.map[min(q, B.nslots - 1)];
  const int world = H.world, rank = H.rank;
  const bool wide = (H.store_through & 2) != 0; // some table has 2^32 - 3 slots or more: rows are parked, not slot offsets

  // ---- phase 0 ----------------------------------------------------------------------
  if (tid < B.ncols) stage_col(H, &s_col[tid], H.cols + B.first_col + tid, H.dyn + B.first_col + tid);
  __syncthreads();

  // ---- phase 1a: raw id words of this thread's (column, row) pairs ------------------------
  // issued before the boundary staging so that the two memory round trips overlap.  The column facts of
  // all the thread's pairs are read from LDS in one batch (unconditional reads, one wait), then the id
  // loads are issued back to back: interleaving "LDS read, wait, load" per pair put ~0.3 us of LDS
  // round trips in front of the last id load.
  constexpr int PT = (FCP_WAVE * RB + FCP_BLOCK_THREADS - 1) / FCP_BLOCK_THREADS; // pairs per thread, at most
  uint32_t raw_lo[PT], raw_hi[PT], pflags[PT];
  const char *pids[PT];
  const int npairs = B.ncols * RB;
#pragma unroll
  for (int h = 0; h < PT; ++h) {
    const int p = tid + h * FCP_BLOCK_THREADS;
    const int j = min(p / RB, B.ncols - 1);
    pflags[h] = s_col[j].flags;
    pids[h] = s_col[j].ids;
  }
#pragma unroll
  for (int h = 0; h < PT; ++h) {
    const int p = tid + h * FCP_BLOCK_THREADS;
    const int b = B.row_blk + p % RB;
    const unsigned form = FCP_F_FORM(pflags[h]);
    raw_lo[h] = raw_hi[h] = 0;
    if (p < npairs && b < B.rows && form == FCP_FORM_GATHER) {
      const bool is64 = FCP_F_IDSRC(pflags[h]) == FCP_IDS_I64;
      const char *a = pids[h] + (is64 ? 8 : 4) * (int64_t)b;
      raw_lo[h] = *as_global(reinterpret_cast<const uint32_t *>(a));
      raw_hi[h] = *as_global(reinterpret_cast<const uint32_t *>(a + (is64 ? 4 : 0)));
    }
  }

  // ---- phase 0b: bucketize boundaries -> LDS (skipped when the span has none) --------------
  // Every wave derives the same staging plan from the column records (lane l looks at column
  // l): which columns bucketize, which of them lead a run of neighbours sharing one boundary
  // array (deduplicated at plan creation), and where each run's copy goes (wave-shuffle prefix
  // sum).  No block-wide vote, no per-column LDS round trips: the leaders' (pointer, length,
  // offset) triples travel by lane broadcast, all 256 threads copy, one barrier publishes.
  // (arrays reproducible as fma(i, step, b0) are not staged: their boundaries are computed, never read)
  const bool my_bkt = lane < B.ncols && FCP_F_IDSRC(s_col[lane].flags) == FCP_IDS_F32_BUCKETIZE &&
                      FCP_F_FORM(s_col[lane].flags) == FCP_FORM_GATHER && s_col[lane].bnd_step == 0.0f;
  const unsigned long long any_bkt = __ballot(my_bkt);
  if (any_bkt) {
    const float *mine = my_bkt ? s_col[lane].boundaries : nullptr;
    const float *prev = reinterpret_cast<const float *>(__shfl_up((unsigned long long)mine, 1));
    const bool leader = my_bkt && (lane == 0 || prev != mine);
    const int nb_all = my_bkt ? s_col[lane].n_boundaries : 0;
    const int nb = leader ? nb_all : 0;
    int incl = nb;
#pragma unroll
    for (int d = 1; d < FCP_WAVE; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    // followers take their leader's slice; arrays that do not fit stay in global memory (-1)
    const int boff = (nb_all > 0 && incl <= BND && incl >= nb_all) ? incl - nb_all : -1;
    if (wave == 0 && boff >= 0) s_col[lane].bnd_off = boff;
    unsigned long long todo = __ballot(leader && boff >= 0);
    while (todo) {
      const int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const FCP_GLOBAL float *src = as_global(reinterpret_cast<const float *>(__shfl((unsigned long long)mine, j)));
      const int n = __shfl(nb_all, j), off = __shfl(boff, j);
      for (int i = tid; i < n; i += FCP_BLOCK_THREADS) s_bnd[off + i] = src[i];
    }
    __syncthreads();
  }

  // ---- phase 1b: raw ids -> table slot offsets in LDS -----------------------------------------
#pragma unroll
  for (int h = 0; h < PT; ++h) {
    const int p = tid + h * FCP_BLOCK_THREADS;
    if (p >= npairs) break;
    const int j = p / RB, r = p % RB;
    const int b = B.row_blk + r;
    uint32_t off = kNoRow;
    if (b < B.rows) {
      const LdsCol &c = s_col[j];
      const unsigned form = FCP_F_FORM(pflags[h]);
      if (form == FCP_FORM_PASSTHROUGH) {
        // a tensor of the blob copied into its concat slot; table-free columns
        // belong to shard rank 0
        if (rank == 0) off = wide ? (uint32_t)b : (uint32_t)b * (uint32_t)(c.dim / V);
      } else if (form == FCP_FORM_GATHER) {
        bool bad;
        off = slot_offset_from_raw<V, SHARDED>(c, L.xforms + B.first_col + j, raw_lo[h], raw_hi[h],
                                               c.bnd_off >= 0 ? s_bnd + c.bnd_off : nullptr,
                                               rank, world, bad);
        if constexpr (TABMIX) { // the stride of THIS column's format: (dim + 8) / V for a q8 table, dim / V for the others
          if (!wide && is_row(off)) off *= (uint32_t)((c.dim + (FCP_F_TABKIND(pflags[h]) == FCP_TAB_Q8 ? 8 : 0)) / V);
        } else if constexpr (TABQ8) {
          if (!wide && is_row(off)) off *= (uint32_t)((c.dim + 8) / V); // the row STRIDE in slots: offset x V = the row's byte offset
        } else {
          if (!wide && is_row(off)) off *= (uint32_t)(c.dim / V); // every table of the plan has < 2^32 - 3 slots: pre-scaled
        }
        // a column that straddles two spans is staged by two blocks: the one holding its first slot counts
        if (bad && H.bad_ids && c.out_off >= B.q0 * V) atomicAdd(H.bad_ids, 1ull);
      } // FCP_FORM_EXTERNAL: nothing to fetch, nothing to write
    }
    s_off[j * IDS + r] = off;
  }
  __syncthreads();
  if (q >= B.nslots) return;

  // ---- phase 2: R table reads in flight per lane, then R coalesced stores -------------------
  const int j = (int)(my_col - B.first_col);
  const int e = q * V - s_col[j].out_off;
  const float *tb = s_col[j].table + e;
  const int64_t ostride = s_col[j].out_stride;
  if (FCP_F_FORM(s_col[j].flags) == FCP_FORM_EXTERNAL) return; // somebody else's slot (ConcatOutputs host input)
  float *outp = reinterpret_cast<float *>(H.arena + s_col[j].out_base) + e;
  char *outp16 = nullptr; // narrow output: the same element, 2 bytes each
  if constexpr (NARROW) outp16 = H.arena + s_col[j].out_base + 2 * (int64_t)e;
  const int r0 = wave * R;
  const uint32_t spr = (uint32_t)(s_col[j].dim / V); // slots per table row
  uint32_t off[R];
#pragma unroll
  for (int r = 0; r < R; ++r) off[r] = s_off[j * IDS + r0 + r];
  VF<V> v[R];
  if constexpr (TABMIX) {
    // (a PASSTHROUGH column carries kind 0 and its "table" is its float32 payload: the float32 path)
    const int kind = (int)FCP_F_TABKIND(s_col[j].flags), k0 = __builtin_amdgcn_readfirstlane(kind);
    const char *table = reinterpret_cast<const char *>(s_col[j].table);
    if (__ballot(kind != k0) == 0ull)
      ld_rows_mixed<V, R>(v, off, k0, table, e, s_col[j].dim, wide); // one kind in the whole wave: scalar branches
    else
      ld_rows_mixed<V, R>(v, off, kind, table, e, s_col[j].dim, wide);
  }
#pragma unroll
  for (int r = 0; r < (TABMIX ? 0 : R); ++r) { // (TABMIX: read above, by kind)
    v[r] = vzero<V>();
    if constexpr (TAB16) {
      if (FCP_F_FORM(s_col[j].flags) != FCP_FORM_PASSTHROUGH) {
        const char *tb16 = reinterpret_cast<const char *>(s_col[j].table) + 2 * (int64_t)e; // element offset x 2, in 64 bits
        if (is_row(off[r])) v[r] = wide ? ld_slot16<V>(tb16, off[r], spr, tab_kind) : ld_slot32_16<V>(tb16, off[r], tab_kind);
        continue;
      }
    }
    if constexpr (TABQ8) {
      if (FCP_F_FORM(s_col[j].flags) != FCP_FORM_PASSTHROUGH) {
        const char *tb8 = reinterpret_cast<const char *>(s_col[j].table) + e; // the lane's codes in row 0; the scale dim - e behind
        const int tail = s_col[j].dim - e;
        if (is_row(off[r])) v[r] = wide ? ld_slot_q8<V>(tb8, tail, off[r], (uint32_t)s_col[j].dim + 8u) : ld_slot32_q8<V>(tb8, tail, off[r]);
        continue;
      }
    }
    if (is_row(off[r])) v[r] = wide ? ld_slot<V>(tb, off[r], spr) : ld_slot32<V>(tb, off[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int b = B.row_blk + r0 + r;
    if constexpr (NARROW) {
      if (b < B.rows) st_out_narrow<V>(outp16 + 2 * (int64_t)b * ostride, v[r], H.store_through, out_kind);
    } else {
      if (b < B.rows) st_out<V>(outp + (int64_t)b * ostride, v[r], H.store_through);
    }
  }
}

template <int V, int R, bool SHARDED>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dense_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(DenseLds<R>)];
  dense_body<V, R, SHARDED>(L, blockIdx.x, smem);
}

// Table reads a lane of the ragged kernel keeps in flight while it walks a bag (measured:
// 12 / 16 need 71 / 87 VGPRs and lose more to occupancy than they gain, profiles/HISTORY.md, round 1).
constexpr int kWalk = 8;
constexpr int kWalkFirst = 10; // widest first batch of a bag walk (10: 64 VGPRs, the most that keeps 8 waves per SIMD without scratch)
constexpr int kWalkLong = 6;   // the same in the rounds after the first (rows whose bags exceed the wave's tile)
                               // (8 would need 66 VGPRs in the loop around the rounds)

// ---------------------------------------------------------------------------
// Ragged kernel: any mix of column forms (dynamic shapes: multi-hot bags of
// variable length, scatter columns, passthrough, Sum(axis=1)).
//
// Same block shape as the dense kernel, one output row per wave (RB = 4).
//   phase 0  (block) the span's column records -> LDS; the only barrier
//            (plans whose few segment-id columns are searched in the blocks add a
//            second one around the search);
//   phase 1  (wave) a wave owns ONE output row, so it stages its own row's bags:
//            lane j < ncols reads the CSR range [lo, lo+cnt) of (column j, row) —
//            the row-offset buffer — a wave prefix sum (shuffles) assigns the bag a
//            slice of the wave's LDS offset tile and the lane marks the slice in the
//            wave's owner table; then one lane per *id* (owner table -> column,
//            position) fetches it and stores the table slot offset (Bucketize, range
//            check, row shard: once per id instead of once per lane, all ids of the
//            row in one memory round trip);
//   phase 2  (wave) lane q walks its column's bag — range and slice come from the
//            owner lane by cross-lane reads: 8 (then 4) slot offsets -> as many
//            independent 16-byte table reads in flight -> adds in id order
//            (sequential fp32 order: deterministic, the oracle's; the additions TF-CPU
//            performs for bags of up to 9 ids — from 10 on TF sums every further 8 rows among
//            themselves first, orc_sparse_segment_reduce_tfcpu, within 1e-5), divides for mean (sum / count, cuda_emitter.cc:625,
//            :903); the wave stores 1 KiB contiguous of the concat row.
// Bags longer than 64 ids, or bags that do not fit the wave's 384-entry tile, are
// walked from global memory by the lanes themselves (same arithmetic order).
// Round 1 staged at block scope (ranges, a block-wide scan and the ids of all four
// rows behind four barriers, 19.7 KB of LDS); measured against this form on RAGGED,
// E and F the two are equal within noise (30.3-30.7 us RAGGED): a launch is bounded
// by its ramp, tail and the ~2.4 us kernel boundary, not by the barriers
// (profiles/HISTORY.md, round 2).  The wave-scope form stays: 15.1 KB of LDS, one barrier.
// The kernel is instruction-issue bound rather than HBM bound (rocprofv3: ~490
// VALU per wave before this layout), hence the pre-scaled 32-bit slot offsets:
// a table read costs one LDS read, one compare, one 64-bit shift-add, one load.
// ---------------------------------------------------------------------------
// First position i in [0, n] whose segment id is >= target, in the sorted id stream of one
// column (int32, or int64 read as two dwords; element i lives at index i * stride) — the
// CSR offset ComputeSegmentOffsets (cuda_emitter.cc:768-818) would store for row `target`.
// 16-ary search: every level issues 16 independent probes, so a column with nnz ids costs
// ceil(log16 nnz) memory round trips (3 for nnz <= 4096) instead of log2 nnz.
__device__ __forceinline__ int64_t seg_at(const char *seg, bool is64, int stride, int p) {
  const int64_t e = (int64_t)p * stride;
  return is64 ? ld_i64_a4(seg + 8 * e) : (int64_t)*as_global(reinterpret_cast<const int32_t *>(seg + 4 * e));
}

// One level of the 16-ary search on [a, z]: 16 independent probes, then the interval shrinks to
// less than a 16th.
__device__ __forceinline__ void seg_narrow(const char *seg, bool is64, int stride, int target, int &a, int &z) {
  const int step = (z - a + 15) >> 4;
  int64_t v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int p = a + k * step;
    v[k] = INT64_MAX;
    if (p < z) v[k] = seg_at(seg, is64, stride, p);
  }
  int c = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) c += v[k] < (int64_t)target ? 1 : 0;
  const int valid = (z - a + step - 1) / step; // probes that were inside [a, z)
  const int na = c ? a + (c - 1) * step + 1 : a;
  if (c < valid) z = a + c * step; // probe c is >= target
  a = na;
}

__device__ __forceinline__ int seg_lower_bound(const char *seg, bool is64, int stride, int n, int target, int rows) {
  int a = 0, z = n; // the answer lies in [a, z]; everything before a is < target, everything from z on is >= target
  if (n > 256 && rows > 0) {
    // Rows hold about nnz / rows ids each, so row `target` starts near target * nnz / rows.  Search a
    // 256-wide window around that guess speculatively, together with the two probes that tell whether
    // the window brackets the answer (same round trip); if it does, one level is saved, if not the
    // full search starts over.
    const int g = (int)((int64_t)target * n / rows);
    const int lo = max(g - 128, 0), hi = min(lo + 256, n);
    const int64_t below = lo > 0 ? seg_at(seg, is64, stride, lo - 1) : INT64_MIN;
    const int64_t above = hi < n ? seg_at(seg, is64, stride, hi) : INT64_MAX;
    int wa = lo, wz = hi;
    seg_narrow(seg, is64, stride, target, wa, wz);
    if (below < (int64_t)target && above >= (int64_t)target) {
      a = wa;
      z = wz;
    }
  }
  while (z > a) seg_narrow(seg, is64, stride, target, a, z);
  return a;
}

// LDS accesses of ONE wave execute in program order; the compiler only has to keep that order.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Where slot offset `off` of a bag is read from: the table row, or — an id that contributes nothing (out of
// range, another rank's row, dropped by the filter, past the end of the bag) — the plan's zero line: one hot
// cache line instead of a predicated read, so the walk is branch-free (no exec-mask bookkeeping around every
// read); adding its +0.0 is exact (acc is never -0.0: it starts at +0.0).
template <int V> __device__ __forceinline__ VF<V> ld_slot_or_zero(const float *tb, const float *zeros, uint32_t off, uint32_t spr) {
  typedef typename VecType<V>::T T;
  const FCP_GLOBAL T *g = is_row(off) ? as_global(reinterpret_cast<const T *>(tb)) + (uint64_t)off * spr : as_global(reinterpret_cast<const T *>(zeros));
  const T t = *g;
  VF<V> r;
  __builtin_memcpy(&r, &t, sizeof(T));
  return r;
}

// (16-bit tables: `tb` is a byte address; the zero line serves both widths — 2 * V of its zero bytes widen to +0.0)
template <int V>
__device__ __forceinline__ VF<V> ld_slot_or_zero16(const char *tb, const float *zeros, uint32_t off, uint32_t spr, int tab_kind) {
  typedef typename NarrowType<V>::T T;
  const FCP_GLOBAL T *g = is_row(off) ? as_global(reinterpret_cast<const T *>(tb)) + (uint64_t)off * spr : as_global(reinterpret_cast<const T *>(zeros));
  return widen16<V>(*g, tab_kind);
}

// (8-bit row-quantised tables; the zero line: zero codes with a zero scale and a zero bias dequantise to fma(0, +0, +0) = +0.0)
template <int V>
__device__ __forceinline__ Q8Raw ld_slot_or_zero_q8(const char *tb, const float *zeros, int tail, uint32_t off, uint32_t row_bytes) {
  // (both candidates are formed first: the choice is a v_cndmask pair, never a branch around the multiply — a branch per
  // read would cut the batch of reads into dependent pieces.  The zero line of a q8 plan is as long as its longest row, so
  // the scale and bias are read `tail` bytes behind the codes there too: zeros.)
  const char *in_table = tb + (uint64_t)off * row_bytes, *in_zeros = reinterpret_cast<const char *>(zeros);
  const char *codes = is_row(off) ? in_table : in_zeros;
  return ld_q8_raw<V>(codes, codes + tail);
}

// The walk of one bag slice for one output slot: the n table slot offsets staged at s[0..n) are added to `acc`
// in id order (sequential fp32 adds: the order of the oracle; TF-CPU's up to 9 ids per bag), kWalk table reads in flight
// per lane.  EVERY lane issues its first kWalk reads at once, whatever its bag length; further batches
// only while some bag of the wave goes on.  (Round 2 walked "8, then 4" behind per-lane conditions: lanes with
// up to 4 ids sat out the first pass and issued their reads only after it.)
// TAB16 (16-bit tables): `tb` carries the lane's base as a byte address, the reads are the 16-bit loader's.
// TABQ8 (8-bit row-quantised tables): `tb` carries the lane's base as a byte address, `q8_tail` the distance from the lane's
// codes to the row's scale; `spr` is the row's size in BYTES, dim + 8.
// X: FCP_VAR_TAB16, FCP_VAR_TABQ8, or any other variant for the float32 walk.
template <int V, int N, FcpVariant X = FCP_VAR_F32>
__device__ __forceinline__ void bag_walk_batch(const float *tb, const float *zeros, uint32_t spr, const uint32_t *s, int base, int n, VF<V> &acc,
                                               int tab_kind = 0, int q8_tail = 0) {
  constexpr bool TAB16 = X == FCP_VAR_TAB16, TABQ8 = X == FCP_VAR_TABQ8;
  uint32_t off[N];
#pragma unroll
  for (int k = 0; k < N; ++k) off[k] = base + k < n ? s[base + k] : kNoRow;
  if constexpr (TABQ8) {
    // the reads stay in flight as they arrived (three dwords per row, not V floats); an element is dequantised where it
    // is added, in id order
    Q8Raw raw[N];
#pragma unroll
    for (int k = 0; k < N; ++k) raw[k] = ld_slot_or_zero_q8<V>(reinterpret_cast<const char *>(tb), zeros, q8_tail, off[k], spr);
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
      for (int t = 0; t < V; ++t) acc.v[t] = acc.v[t] + dequant_q8(raw[k], t);
    return;
  }
  VF<V> w[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if constexpr (TAB16)
      w[k] = ld_slot_or_zero16<V>(reinterpret_cast<const char *>(tb), zeros, off[k], spr, tab_kind);
    else
      w[k] = ld_slot_or_zero<V>(tb, zeros, off[k], spr);
  }
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int t = 0; t < V; ++t) acc.v[t] = acc.v[t] + w[k].v[t]; // id order
}

template <int V, int WALK, FcpVariant X = FCP_VAR_F32>
__device__ __forceinline__ void bag_walk_sum(const float *tb, const float *zeros, uint32_t spr, const uint32_t *s, int n, VF<V> &acc,
                                             int tab_kind = 0, int q8_tail = 0) {
  // The first batch is as wide as the wave's longest bag needs, up to kWalkFirst reads per lane: every bag of
  // the wave in ONE round of reads whenever none is longer than that (BASELINE's RAGGED and the reference's models
  // E / F draw 0..10 / 1..10 ids per row: with 8-wide batches nearly every wave ran a second round for its one or two
  // 9- and 10-id bags; RAGGED 30.2 -> 28.9 us, profiles/r03_ragged_walk_width_ab.txt).  Wave-uniform choices.
  int base = WALK;
  if (WALK >= 8 && !__any(n > 4)) {
    bag_walk_batch<V, 4, X>(tb, zeros, spr, s, 0, n, acc, tab_kind, q8_tail);
    return;
  } else if (WALK >= 8 && kWalkFirst > WALK && __any(n > WALK)) {
    bag_walk_batch<V, kWalkFirst, X>(tb, zeros, spr, s, 0, n, acc, tab_kind, q8_tail);
    base = kWalkFirst;
  } else {
    bag_walk_batch<V, WALK, X>(tb, zeros, spr, s, 0, n, acc, tab_kind, q8_tail);
  }
  for (; __any(n > base);) { // wave-uniform trip count
    if (WALK > 4 && !__any(n > base + 4)) { // a short tail (bags of 9..12 ids): half a batch
      bag_walk_batch<V, 4, X>(tb, zeros, spr, s, base, n, acc, tab_kind, q8_tail);
      base += 4;
    } else {
      bag_walk_batch<V, WALK, X>(tb, zeros, spr, s, base, n, acc, tab_kind, q8_tail);
      base += WALK;
    }
  }
}

// ---- per-id weights (fcp_column_ext_t::weights_input1: TensorFlow's embedding_lookup_sparse(sp_ids, sp_weights)) --------
// One step of a bag's denominator, in id order: MEAN adds the weight, SQRTN its rounded square.  A rounded product, then a
// rounded add: contraction into a fused multiply-add is switched off for this code (TF multiplies and sums in two ops).
__device__ __forceinline__ float weight_den_step(float den, float w, bool squares) {
#pragma clang fp contract(off)
  const float term = squares ? w * w : w;
  return den + term;
}

// The weighted walk of one bag slice: acc = fl32(acc + fl32(w_k * row_k)) in id order — contraction off, as above.  The
// weights of a bag are contiguous in the blob (w[k] belongs to s[k]); every lane of a column asks for the same address,
// and the weight loads are issued together with the batch of table reads.  An id that contributes nothing (dropped by the
// filter, another rank's row, past the end of the slice) adds neither a term nor a weight; an id outside the vocabulary
// reads the zero line, its product is added and its weight counts.  `den` (one scalar per lane, not per element) is
// accumulated only when the caller wants it (an unsharded MEAN / SQRTN column).  Batches of four: the body has to stay
// within 64 VGPRs for every V next to the weights and the denominator.
template <int V>
__device__ __forceinline__ void bag_walk_weighted(const float *tb, const float *zeros, uint32_t spr, const uint32_t *s, int n,
                                                  const float *w, bool want_den, bool squares, VF<V> &acc, float &den) {
#pragma clang fp contract(off)
  constexpr int N = 4;
  const FCP_GLOBAL float *gw = as_global(w);
#pragma unroll 1
  for (int base = 0; base < n; base += N) {
    uint32_t off[N];
    float wt[N];
    VF<V> x[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = base + k < n ? s[base + k] : kNoRow;
#pragma unroll
    for (int k = 0; k < N; ++k) wt[k] = gw[min(base + k, n - 1)]; // (clamped: never past the bag; unused when off is kNoRow)
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = ld_slot_or_zero<V>(tb, zeros, off[k], spr);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool counts = off[k] <= kBadRow; // a table row, or the zero line of an id outside the vocabulary
#pragma unroll
      for (int t = 0; t < V; ++t) {
        const float prod = wt[k] * x[k].v[t];
        const float sum = acc.v[t] + prod;
        acc.v[t] = counts ? sum : acc.v[t];
      }
      if (want_den && counts) den = weight_den_step(den, wt[k], squares);
    }
  }
}

// Inclusive prefix sum over the 64 lanes of a wave with data-parallel-primitive moves: four shifts inside the rows of
// 16 lanes, then the row totals broadcast to the rows after them (row_bcast:15 / row_bcast:31) — six VALU instructions
// and no LDS traffic, where six __shfl_up steps cost six ds_bpermute round trips plus their index arithmetic.
__device__ __forceinline__ int wave_inclusive_sum(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true); // row_shr:1 (lanes without a source read 0)
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true); // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true); // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true); // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1 and 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false); // row_bcast:31 -> rows 2 and 3
  return x;
}

struct RaggedLds {
  static constexpr int RB = FCP_WAVES_PER_BLOCK; // rows per block, one per wave
  static constexpr int CAPW = 384;               // staged slot offsets per wave (row) and round
  LdsCol col[FCP_WAVE];
  uint32_t ids[RB][CAPW];
  uint8_t owner[RB][CAPW];                       // staged id slot -> owner lane (= column within the span)
  int32_t bound[FCP_WAVE * (FCP_WAVES_PER_BLOCK + 1)]; // seg_search: row offsets r0..r0+RB of every column
};

// WEIGHTED: the instantiation for plans with per-id weights or the sqrtn combiner (fcp_weighted.hip).  `wts`: per column
// (concat order) the byte offset of its float32 weights in the blob, or -1.  Everything it adds sits behind
// `if constexpr (WEIGHTED)`: the unweighted instantiations are the code they were.
// NARROW: as in the dense body — bf16 / fp16 output plans (fcp_narrow.hip), everything behind `if constexpr (NARROW)`.
// TAB16: as in the dense body — bf16 / fp16 table plans (fcp_tables16.hip), everything behind `if constexpr (TAB16)`; never
// together with WEIGHTED (such plans are refused when they are created).
// TABQ8: as in the dense body — 8-bit row-quantised table plans (fcp_tables_q8.hip), everything behind `if constexpr (TABQ8)`;
// never together with WEIGHTED either.
// TABMIX: as in the dense body — plans whose tables have more than one format (fcp_tables_mixed.hip): the lane's column names
// its kind (FCP_F_TABKIND), the walk is the float32, the 16-bit or the q8 walk accordingly; everything behind
// `if constexpr (TABMIX)`; never together with WEIGHTED either.
// `kind`: as in the dense body.
template <int V, bool SHARDED, FcpVariant X = FCP_VAR_F32>
__device__ __forceinline__ void ragged_body(const FcpLaunch &L, int bid, char *smem, const int64_t *wts = nullptr, int kind = 0) {
  constexpr bool WEIGHTED = X == FCP_VAR_WEIGHTED, NARROW = X == FCP_VAR_NARROW, TAB16 = X == FCP_VAR_TAB16, TABQ8 = X == FCP_VAR_TABQ8,
                 TABMIX = X == FCP_VAR_TABMIX;
  const int out_kind = kind, tab_kind = kind;
  constexpr int RB = RaggedLds::RB, CAPW = RaggedLds::CAPW;
  RaggedLds &S = *reinterpret_cast<RaggedLds *>(smem);
  LdsCol *s_col = S.col;

  BlockPos B;
  // The front of a block (records -> CSR ranges -> ids) is a chain of dependent round trips with a handful of
  // instructions between them; issued at a higher wave priority those instructions do not queue behind the long
  // walk loops of the CU's other waves (back to 0 before the walk): RAGGED -0.35 us, batch 1024 -0.5 us
  // (profiles/r03_ragged_front_priority_ab.txt).  The dense body showed no difference.
  __builtin_amdgcn_s_setprio(3);
  const Hot H = load_hot(L);
  if (!locate_block<RB>(L, H, bid, B)) return;
  const int tid = threadIdx.x;
  const int lane = tid & (FCP_WAVE - 1);
  const int wave = tid >> 6;
  const int q = B.q0 + lane;
  const uint32_t my_col = B.map[min(q, B.nslots - 1)];
  const int world = H.world, rank = H.rank;

  // ---- regular CSR (FcpLaunch::csr_reg): the wave's row ranges are requested NOW, next to the column records, instead
  // of behind them — their address needs the span's first column position only
  int pre0 = 0, pre1 = 0;
  const int csr_reg_stride = H.g0.csr_reg_stride;
  if (csr_reg_stride && lane < B.ncols && B.row_blk + wave < B.rows) {
    const FCP_GLOBAL int32_t *cr = as_global(L.csr_reg) + (int64_t)(B.first_col + lane) * csr_reg_stride + (B.row_blk + wave);
    pre0 = cr[0];
    pre1 = cr[1];
  }
  // ---- phase 0 (block) --------------------------------------------------------------------
  if (tid < B.ncols) stage_col(H, &s_col[tid], H.cols + B.first_col + tid, H.dyn + B.first_col + tid);
  __syncthreads();

  // ---- phase 1a' (block): segment-id columns without a pre-pass: RB+1 row offsets per column ---
  if (H.seg_search) {
    for (int u = tid; u < B.ncols * (RB + 1); u += FCP_BLOCK_THREADS) {
      const LdsCol &c = s_col[u / (RB + 1)];
      const unsigned sk = FCP_F_SEGKIND(c.flags), f = FCP_F_FORM(c.flags);
      int v = 0;
      if ((sk == FCP_SEG_IDS_I32 || sk == FCP_SEG_IDS_I64) && (f == FCP_FORM_SEGMENT_REDUCE || f == FCP_FORM_GATHER_SCATTER))
        v = seg_lower_bound(reinterpret_cast<const char *>(c.csr), sk == FCP_SEG_IDS_I64, c.seg_stride, c.nnz,
                            min(B.row_blk + u % (RB + 1), B.rows), B.rows);
      S.bound[u] = v;
    }
    __syncthreads();
  }
  const int b = B.row_blk + wave;
  if (b >= B.rows) return; // wave-uniform; no block barrier follows

  // ---- phase 1a (wave): range [lo, lo + cnt) of (column lane, row b) ------------------------------------
  int lo = 0, cnt = 0;
  if (lane < B.ncols) {
    const unsigned form = FCP_F_FORM(s_col[lane].flags);
    if (form == FCP_FORM_GATHER) {
      lo = b;
      cnt = 1;
    } else if (form == FCP_FORM_SEGMENT_REDUCE || form == FCP_FORM_GATHER_SCATTER) {
      const int nnz = s_col[lane].nnz;
      int o0, o1;
      const unsigned sk = FCP_F_SEGKIND(s_col[lane].flags);
      if (form == FCP_FORM_GATHER_SCATTER && sk != FCP_SEG_CSR_I32) {
        // ScatterNd with its row ids as delivered, in ANY order (GatherScatterRows, cuda_emitter.cc:296-345):
        // the pre-pass left "1 + position of the last id written to row b" (0: none) in the column's scratch
        const int t = as_global(s_col[lane].csr)[b];
        o0 = t - 1;
        o1 = t > 0 ? t : -1;
      } else if (H.seg_search && sk != FCP_SEG_CSR_I32) {
        o0 = S.bound[lane * (RB + 1) + wave];
        o1 = S.bound[lane * (RB + 1) + wave + 1];
      } else if (csr_reg_stride) { // requested in front of the records (above)
        o0 = pre0;
        o1 = pre1;
      } else {
        const FCP_GLOBAL int32_t *csr = as_global(s_col[lane].csr);
        o0 = csr[b];
        o1 = csr[b + 1];
      }
      lo = min(max(o0, 0), nnz);
      const int hi = min(max(o1, lo), nnz);
      cnt = hi - lo;
      // GATHER_SCATTER: the last id of the row wins; a row with several ids (duplicate row ids) is walked
      // whole only when an id filter may drop its last ones
      if (form == FCP_FORM_GATHER_SCATTER && cnt > 1 && (s_col[lane].xform & 3u) != FCP_XFORM_FILTER) {
        lo = hi - 1;
        cnt = 1;
      }
    }
  }

  // my slot: which column (its facts are re-read from LDS where they are used: few registers live across the staging)
  const int j = (int)(my_col - B.first_col);
  const bool live = q < B.nslots;
  VF<V> acc = vzero<V>();
  int dropped = 0; // ids the column's filter removed: they do not count in a mean

  uint8_t *ow = S.owner[wave];
  uint32_t *wi = S.ids[wave];
  // ---- phase 1b (wave): slices of the wave's offset tile — a prefix sum over the lanes' bag lengths; a bag gets
  // what is left of the tile after the bags of the lanes before it (`take` of its `cnt` ids; all of them unless the
  // row holds more than CAPW ids, see "long bags" below)
  const int want = min(cnt, CAPW);
  const int incl = wave_inclusive_sum(want);
  const int offx = incl - want;
  const int take = max(min(want, CAPW - offx), 0);
  const int limit = min(__shfl(incl, FCP_WAVE - 1), CAPW);
  if (take <= 16)
    for (int i = 0; i < take; ++i) ow[offx + i] = (uint8_t)lane; // fire-and-forget LDS writes
  for (unsigned long long big = __ballot(take > 16); big; big &= big - 1) { // long slices are marked by the whole wave
    const int p = __ffsll((long long)big) - 1;
    const int po = __shfl(offx, p), pt = __shfl(take, p);
    for (int i = lane; i < pt; i += FCP_WAVE) ow[po + i] = (uint8_t)p;
  }
  wave_lds_order();

  // ---- one lane per staged id -> table slot offset in the wave's tile ---------------------------------------
  for (int base = 0; base < limit; base += FCP_WAVE) { // uniform trip count: the cross-lane reads need every lane
    const int k = base + lane;
    const int p = k < limit ? (int)ow[k] : 0;
    const int px = __shfl(offx, p), pl = __shfl(lo, p);
    if (k < limit) {
      bool bad;
      wi[k] = fetch_slot_offset<V, SHARDED>(s_col[p], L.xforms + B.first_col + p, pl + (k - px), nullptr, rank, world, bad);
      // a column that straddles two spans is staged by two blocks: the one holding its first slot counts.  (ScatterNd
      // columns count where the row's winner is known: an id that a later write replaces never reached the output.)
      if (bad && H.bad_ids && s_col[p].out_off >= B.q0 * V && FCP_F_FORM(s_col[p].flags) != FCP_FORM_GATHER_SCATTER)
        atomicAdd(H.bad_ids, 1ull);
    }
  }
  wave_lds_order();

  __builtin_amdgcn_s_setprio(0);
  // ---- phase 2 (wave): the owning lanes consume their column's slice ------------------------------------------
  // (a slot's column facts are re-read from LDS where they are used: few registers live across the staging)
  // the weighted instantiation: where this lane's column keeps its weights (null: an unweighted column, walked and
  // finished exactly as in the unweighted kernel — no multiplication by one), and the lane's denominator
  const float *wbase = nullptr;
  float den = 0.0f;
  if constexpr (WEIGHTED) {
    if (wts) { // (null: the plan only uses the sqrtn combiner)
      const int64_t wo = as_global(wts)[B.first_col + j];
      if (wo >= 0) wbase = reinterpret_cast<const float *>(H.blob + wo);
    }
  }
  // wpos (weighted instantiation only): position in the column's id stream of s[0]
  auto consume = [&](auto walk_width, const uint32_t *s, int n, int wpos) __attribute__((always_inline)) {
    constexpr int WALK = decltype(walk_width)::value;
    const unsigned form = FCP_F_FORM(s_col[j].flags);
    const float *tb = s_col[j].table + (q * V - s_col[j].out_off);
    if constexpr (TAB16) // the same element as a byte address: element offset x 2, in 64 bits
      tb = reinterpret_cast<const float *>(reinterpret_cast<const char *>(s_col[j].table) + 2 * (int64_t)(q * V - s_col[j].out_off));
    uint32_t spr = (uint32_t)(s_col[j].dim / V); // slots per table row
    int q8_tail = 0;
    if constexpr (TABQ8) { // the lane's codes in row 0 as a byte address, their distance to the row's scale, the row's bytes
      const int e = q * V - s_col[j].out_off;
      tb = reinterpret_cast<const float *>(reinterpret_cast<const char *>(s_col[j].table) + e);
      q8_tail = s_col[j].dim - e;
      spr = (uint32_t)s_col[j].dim + 8u;
    }
    int kind = 0; // TABMIX: FCP_TAB_* of this lane's table; `tb`, `spr` and `q8_tail` as that format's walk takes them
    if constexpr (TABMIX) {
      kind = (int)FCP_F_TABKIND(s_col[j].flags);
      const int e = q * V - s_col[j].out_off;
      if (kind == FCP_TAB_Q8) {
        tb = reinterpret_cast<const float *>(reinterpret_cast<const char *>(s_col[j].table) + e);
        q8_tail = s_col[j].dim - e;
        spr = (uint32_t)s_col[j].dim + 8u;
      } else if (kind != FCP_TAB_F32) {
        tb = reinterpret_cast<const float *>(reinterpret_cast<const char *>(s_col[j].table) + 2 * (int64_t)e);
      }
    }
    if (form == FCP_FORM_SEGMENT_REDUCE) {
      if ((s_col[j].xform & 3u) == FCP_XFORM_FILTER && (FCP_F_COMBINER(s_col[j].flags) == FCP_COMBINER_MEAN ||
                                                        (WEIGHTED && FCP_F_COMBINER(s_col[j].flags) == FCP_COMBINER_SQRTN))) {
        // ids the filter dropped do not count in the mean: a separate pass over the staged offsets, only for
        // such columns (counting inside the walk cost every column 12 registers)
#pragma unroll 1
        for (int k = 0; k < n; ++k) dropped += s[k] == kFiltered;
      }
      if constexpr (WEIGHTED) {
        if (wbase) {
          const unsigned comb = FCP_F_COMBINER(s_col[j].flags);
          bag_walk_weighted<V>(tb, H.zeros, spr, s, n, wbase + wpos, !SHARDED && comb != FCP_COMBINER_SUM, comb == FCP_COMBINER_SQRTN,
                               acc, den);
        } else { // (no wider than kWalkLong: next to the weight pointer and the denominator a 10-wide batch spills at V = 4)
          bag_walk_sum<V, (WALK < kWalkLong ? WALK : kWalkLong)>(tb, H.zeros, spr, s, n, acc);
        }
      } else if constexpr (TABMIX) {
        // the walk of the lane's kind; the votes inside a walk count the lanes of that kind only.  One ballot tells whether
        // the wave's pooled lanes hold one kind: then the choice is a scalar branch and the 16-bit widening knows its type
        auto walk = [&](int k) __attribute__((always_inline)) {
          if (k == FCP_TAB_F32)
            bag_walk_sum<V, WALK>(tb, H.zeros, spr, s, n, acc);
          else if (k == FCP_TAB_Q8)
            bag_walk_sum<V, WALK, FCP_VAR_TABQ8>(tb, H.zeros, spr, s, n, acc, 0, q8_tail);
          else
            bag_walk_sum<V, WALK, FCP_VAR_TAB16>(tb, H.zeros, spr, s, n, acc, k);
        };
        const int k0 = __builtin_amdgcn_readfirstlane(kind);
        if (__ballot(kind != k0) == 0ull)
          walk(k0);
        else
          walk(kind);
      } else if constexpr (TABQ8) {
        bag_walk_sum<V, WALK, FCP_VAR_TABQ8>(tb, H.zeros, spr, s, n, acc, 0, q8_tail);
      } else if constexpr (TAB16) {
        bag_walk_sum<V, WALK, FCP_VAR_TAB16>(tb, H.zeros, spr, s, n, acc, tab_kind);
      } else {
        bag_walk_sum<V, WALK>(tb, H.zeros, spr, s, n, acc);
      }
    } else if (form == FCP_FORM_GATHER || form == FCP_FORM_GATHER_SCATTER) {
      // a pure copy of one row (rows without ids stay zero); of several ids the last one the filter kept wins
      // (TF: ScatterNd after the filter op; the oracle compacts first)
      int k = n - 1;
      while (k > 0 && s[k] == kFiltered) --k;
      const uint32_t off = s[k];
      if (off != kFiltered) {
        acc = vzero<V>();
        if constexpr (TABMIX) {
          if (is_row(off)) {
            if (kind == FCP_TAB_F32)
              acc = ld_slot<V>(tb, off, spr);
            else if (kind == FCP_TAB_Q8)
              acc = ld_slot_q8<V>(reinterpret_cast<const char *>(tb), q8_tail, off, spr);
            else
              acc = ld_slot16<V>(reinterpret_cast<const char *>(tb), off, spr, kind);
          }
        } else if constexpr (TABQ8) {
          if (is_row(off)) acc = ld_slot_q8<V>(reinterpret_cast<const char *>(tb), q8_tail, off, spr);
        } else if constexpr (TAB16) {
          if (is_row(off)) acc = ld_slot16<V>(reinterpret_cast<const char *>(tb), off, spr, tab_kind);
        } else {
          if (is_row(off)) acc = ld_slot<V>(tb, off, spr);
        }
        // the winner of a ScatterNd row is out of the vocabulary: counted once, by the lane of the column's first slot
        if (form == FCP_FORM_GATHER_SCATTER && off == kBadRow && H.bad_ids && q * V == s_col[j].out_off) atomicAdd(H.bad_ids, 1ull);
      }
    }
  };
  {
    const int ptake = __shfl(take, j), poff = __shfl(offx, j);
    int wpos = 0;
    if constexpr (WEIGHTED) wpos = __shfl(lo, j);
    if (live && ptake > 0) consume(std::integral_constant<int, kWalk>(), wi + poff, ptake, wpos);
  }

  // ---- long bags (rare: a row whose bags hold more than CAPW ids, e.g. multi-hot history features of hundreds
  // of ids): what the tile could not take in goes through it in further rounds.  Every bag that has ids left gets
  // an EQUAL share of the tile per round (a power of two: position -> (bag, index) is a shift and a mask; no
  // prefix sum), so all the wave's lanes keep walking their own bags at once, and the owning lanes go on adding
  // to their running sums — the order of the adds is the order of the ids, however they are chunked.  (Round 2
  // walked such bags from global memory, one dependent id read -> row read pair at a time.)
  for (int done = take;;) {
    const int rem = cnt - done;
    const unsigned long long act = __ballot(rem > 0);
    if (!act) break; // wave-uniform
    const int nact = __popcll(act);
    const int sh_log2 = 31 - __clz(CAPW / nact); // nact <= 64: at least 4 ids per bag and round
    const int share = 1 << sh_log2;
    const int my_rank = __popcll(act & ((1ull << lane) - 1ull));
    const int tk = rem > 0 ? min(rem, share) : 0;
    wave_lds_order(); // the tile's previous contents have been consumed
    if (rem > 0) ow[my_rank] = (uint8_t)lane;
    wave_lds_order();
    const int limit = nact << sh_log2;
    const int from = lo + done;
    for (int base = 0; base < limit; base += FCP_WAVE) { // uniform trip count
      const int k = base + lane;
      const int p = k < limit ? (int)ow[k >> sh_log2] : 0;
      const int i = k & (share - 1);
      const int ptk = __shfl(tk, p), pf = __shfl(from, p);
      if (k < limit && i < ptk) {
        bool bad;
        wi[k] = fetch_slot_offset<V, SHARDED>(s_col[p], L.xforms + B.first_col + p, pf + i, nullptr, rank, world, bad);
        if (bad && H.bad_ids && s_col[p].out_off >= B.q0 * V && FCP_F_FORM(s_col[p].flags) != FCP_FORM_GATHER_SCATTER)
          atomicAdd(H.bad_ids, 1ull);
      }
    }
    wave_lds_order();
    const int ptake = __shfl(tk, j), prank = __shfl(my_rank, j);
    int wpos = 0;
    if constexpr (WEIGHTED) wpos = __shfl(from, j);
    if (live && ptake > 0) consume(std::integral_constant<int, kWalkLong>(), wi + (prank << sh_log2), ptake, wpos);
    done += tk;
  }
  const int pcnt = __shfl(cnt, j);
  const LdsCol &C = s_col[j];
  const unsigned form = FCP_F_FORM(C.flags);
  if (!live || form == FCP_FORM_EXTERNAL) return; // EXTERNAL: somebody else's slot (ConcatOutputs host input), never written here

  const int dim = C.dim;
  const int e = q * V - C.out_off;
  if (form == FCP_FORM_PASSTHROUGH) {
    if (rank == 0) acc = ld_blob_f32<V>(C.ids + 4 * ((int64_t)b * dim + e)); // table-free: shard rank 0
  } else if (form == FCP_FORM_BATCH_COL_REDUCTION) {
    // cuda_emitter.cc:1231-1236: r ascending, sequential fp32 adds
    const int inner = rank == 0 ? C.inner : 0;
    for (int rr = 0; rr < inner; ++rr) {
      const VF<V> x = ld_blob_f32<V>(C.ids + 4 * (((int64_t)b * inner + rr) * dim + e));
#pragma unroll
      for (int t = 0; t < V; ++t) acc.v[t] = acc.v[t] + x.v[t];
    }
  } else if (WEIGHTED && form == FCP_FORM_SEGMENT_REDUCE && !SHARDED && FCP_F_COMBINER(C.flags) != FCP_COMBINER_SUM) {
    // the three denominators: MEAN the kept count or the sum of the weights, SQRTN the correctly rounded square root of the
    // kept count or of the sum of the squared weights; ONE IEEE division per element; a zero denominator (no kept ids,
    // weights that cancel) gives a row of +0.0 whatever the numerator holds (TF's div_no_nan)
    float d = wbase ? den : (float)(pcnt - dropped);
    if (FCP_F_COMBINER(C.flags) == FCP_COMBINER_SQRTN) d = sqrtf(d); // (correctly rounded: hipcc's default for sqrtf; __fsqrt_rn is the native 1-ulp instruction here)
    if (d == 0.0f) {
      acc = vzero<V>();
    } else {
#pragma unroll
      for (int t = 0; t < V; ++t) acc.v[t] = acc.v[t] / d;
    }
  } else if (!WEIGHTED && form == FCP_FORM_SEGMENT_REDUCE && !SHARDED && FCP_F_COMBINER(C.flags) == FCP_COMBINER_MEAN && pcnt > dropped) {
    const float fc = (float)(pcnt - dropped); // sum / count of the ids that reached the lookup
#pragma unroll
    for (int t = 0; t < V; ++t) acc.v[t] = acc.v[t] / fc;
  }
  if constexpr (NARROW) {
    st_out_narrow<V>(H.arena + C.out_base + 2 * (e + (int64_t)b * C.out_stride), acc, H.store_through, out_kind);
    return;
  }
  st_out<V>(reinterpret_cast<float *>(H.arena + C.out_base) + e + (int64_t)b * C.out_stride, acc, H.store_through);
}

} // namespace
