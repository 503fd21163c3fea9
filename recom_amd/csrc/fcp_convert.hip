// fcp_convert.hip — fcp_table_convert / fcp_table_row_bytes: the formats the plans READ (FCP_FLAG_TABLES_BF16 / _F16 / _Q8),
// WRITTEN on the device, once, at load time, from the float32 table a checkpoint holds — and back.  Plans do not quantise;
// this does.  The reference reads float32 tables only and has no counterpart.
//
// Four directions, one of the two kinds always float32:
//   float32 -> q8     fcp_quantize_q8_kernel<V, G>: the real kernel (quantize_row of fcp_table_walk.h per row).  Bit for bit what quantized::embedding_bag_byte_prepack
//                     writes (fcp_hip.h spells the arithmetic out).  A row is handled by a power-of-two group of G <= 64
//                     lanes, every lane owning V-element slots (V = 4 | 2 | 1, as on the read side): dim 64 is 16 lanes x
//                     global_load_dwordx4 and four rows per wave, dims <= 4 are one row per lane.  The row stays in registers
//                     between the min / max pass and the encode pass — up to kQSlots slots per lane, dim <= 64 * kQSlots * V;
//                     what lies beyond is read a second time.  The group's min and max are __shfl_xor butterflies (no LDS);
//                     min and max are order-free, so the lane layout cannot change a bit.  Codes leave V bytes at a time
//                     (dword | ushort | ubyte), scale and bias as one pair at the alignment the format allows (Q8Pair<V>),
//                     from the group's first lane.  Reads 4 * dim, writes dim + 8 bytes per row: memory-bound.
//   q8 -> float32     ld_q8<V> of the read side: one v_fma_f32 per element.
//   float32 -> 16     st_out_narrow<V> of the narrow-output store: fl16, rounded once.
//   16 -> float32     widen16<V> of the 16-bit table loaders: exact.
// The last three are streaming kernels, one slot per lane.  The host chunks every direction into launches of at most 2^30
// threads, so an in-launch index fits 32 bits; byte offsets are formed in 64 bits.
//
// No scratch, no LDS; the default modes of the other units (denormals kept, IEEE).  Contraction is off from here to the end of
// the file: every operation of the quantiser rounds once, by itself.  The divisions are the correctly rounded ones.
#include "fcp_fused_bodies.h"
#include "fcp_host.h"

#pragma clang fp contract(off)

#include "fcp_table_walk.h" // (behind the pragma: its code rounds every operation once, too)

static_assert(FCP_TAB_BF16 == FCP_OUT_BF16 && FCP_TAB_F16 == FCP_OUT_F16, "st_out_narrow takes the table kind as its output kind");

namespace {

// dst / src: the first row of this launch; rows: of this launch (< 2^30).  Block = 256 / G rows; a group never straddles a
// wave, and it is live or not as a whole — lanes of rows beyond the end take part in the butterflies and touch no memory.
template <int V, int G>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_quantize_q8_kernel(char *dst, const float *src, int32_t rows, int32_t dim) {
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * (FCP_BLOCK_THREADS / G) + tid / G;
  quantize_row<V, G>(dst + row * ((int64_t)dim + 8), src + row * dim, dim, tid & (G - 1), row < rows);
}

// n: slots of this launch (<= 2^30); src: the first row, its stride dim + 8 bytes; spr: slots per row, dim / V
template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_dequantize_q8_kernel(float *dst, const char *src, uint32_t n, uint32_t spr, int32_t dim) {
  const uint32_t i = blockIdx.x * FCP_BLOCK_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = i / spr;
  const uint32_t e = (i - r * spr) * V;
  const char *row = src + (uint64_t)r * ((uint64_t)dim + 8);
  st_f32<V>(dst + (uint64_t)i * V, ld_q8<V>(row + e, row + dim));
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_narrow16_kernel(char *dst, const float *src, uint32_t n, int32_t kind) {
  const uint32_t i = blockIdx.x * FCP_BLOCK_THREADS + threadIdx.x;
  if (i >= n) return;
  st_out_narrow<V>(dst + (uint64_t)i * (2 * V), ld_f32<V>(src + (uint64_t)i * V), FCP_ST_PLAIN, kind);
}

template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_widen16_kernel(float *dst, const char *src, uint32_t n, int32_t kind) {
  const uint32_t i = blockIdx.x * FCP_BLOCK_THREADS + threadIdx.x;
  if (i >= n) return;
  typedef typename NarrowType<V>::T T;
  const T t = *as_global(reinterpret_cast<const T *>(src + (uint64_t)i * (2 * V)));
  st_f32<V>(dst + (uint64_t)i * V, widen16<V>(t, kind));
}

// G: 1 for dims <= 4, else the power of two that holds the row's slots, at most 64
template <int V> void quantize(char *dst, const float *src, int64_t rows, int dim, hipStream_t s) {
  with_group(group_of(dim, V), [&](auto g) {
    constexpr int G = decltype(g)::value;
    const int64_t per_launch = kMaxLaunchThreads / G;
    for (int64_t r0 = 0; r0 < rows; r0 += per_launch) {
      const int64_t n = std::min(rows - r0, per_launch);
      hipLaunchKernelGGL((fcp_quantize_q8_kernel<V, G>), blocks_for(n * G), dim3(FCP_BLOCK_THREADS), 0, s,
                         dst + r0 * ((int64_t)dim + 8), src + r0 * dim, (int32_t)n, (int32_t)dim);
    }
  });
}

template <int V> void dequantize(float *dst, const char *src, int64_t rows, int dim, hipStream_t s) {
  const int64_t spr = dim / V;
  const int64_t per_launch = std::max<int64_t>(1, kMaxLaunchThreads / spr); // (one row of 2^31 - 1 elements: 2^31 threads)
  for (int64_t r0 = 0; r0 < rows; r0 += per_launch) {
    const int64_t n = std::min(rows - r0, per_launch) * spr;
    hipLaunchKernelGGL(fcp_dequantize_q8_kernel<V>, blocks_for(n), dim3(FCP_BLOCK_THREADS), 0, s, dst + r0 * dim,
                       src + r0 * ((int64_t)dim + 8), (uint32_t)n, (uint32_t)spr, (int32_t)dim);
  }
}

// the 16-bit directions: the rows are one contiguous run of rows * dim / V slots on both sides
template <int V> void stream16(void *dst, const void *src, int64_t slots, bool narrow, int kind, hipStream_t s) {
  for (int64_t i0 = 0; i0 < slots; i0 += kMaxLaunchThreads) {
    const int64_t n = std::min(slots - i0, kMaxLaunchThreads);
    if (narrow)
      hipLaunchKernelGGL(fcp_narrow16_kernel<V>, blocks_for(n), dim3(FCP_BLOCK_THREADS), 0, s, static_cast<char *>(dst) + i0 * 2 * V,
                         static_cast<const float *>(src) + i0 * V, (uint32_t)n, (int32_t)kind);
    else
      hipLaunchKernelGGL(fcp_widen16_kernel<V>, blocks_for(n), dim3(FCP_BLOCK_THREADS), 0, s, static_cast<float *>(dst) + i0 * V,
                         static_cast<const char *>(src) + i0 * 2 * V, (uint32_t)n, (int32_t)kind);
  }
}

template <int V> void convert(void *dst, int dst_kind, const void *src, int src_kind, int64_t rows, int dim, hipStream_t s) {
  if (dst_kind == FCP_TAB_Q8)
    quantize<V>(static_cast<char *>(dst), static_cast<const float *>(src), rows, dim, s);
  else if (src_kind == FCP_TAB_Q8)
    dequantize<V>(static_cast<float *>(dst), static_cast<const char *>(src), rows, dim, s);
  else
    stream16<V>(dst, src, rows * (dim / V), src_kind == FCP_TAB_F32, src_kind == FCP_TAB_F32 ? dst_kind : src_kind, s);
}

} // namespace

extern "C" int64_t fcp_table_row_bytes(int32_t kind, int32_t dim) {
  return dim > 0 && fcpf::known_tab_kind(kind) ? fcpf::row_bytes(kind, dim) : -1;
}

extern "C" int fcp_table_convert(void *dst, int32_t dst_kind, int64_t dst_row0, const void *src, int32_t src_kind, int64_t rows,
                                 int32_t dim, int32_t device, void *stream) {
  if (rows < 0) return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: rows is negative");
  if (dst_row0 < 0) return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: dst_row0 is negative");
  if (dim <= 0) return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: dim must be positive");
  if (!fcpf::known_tab_kind(dst_kind)) return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: dst_kind is no FCP_TAB_* value");
  if (!fcpf::known_tab_kind(src_kind)) return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: src_kind is no FCP_TAB_* value");
  if (rows > 0 && !dst) return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: dst is null");
  if (rows > 0 && !src) return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: src is null");
  if (rows + dst_row0 >= fcpf::kRowLimit || rows >= fcpf::kRowLimit)
    return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: dst_row0 + rows must stay below 2^32 - 3, a plan's row limit");
  const int vec = vec_of(dim);
  if ((uintptr_t)dst % fcpf::base_alignment(dst_kind, vec))
    return fail(FCP_ERR_INVALID_ARGUMENT, std::string("fcp_table_convert: dst is not ") + std::to_string(fcpf::base_alignment(dst_kind, vec)) +
                                              "-byte aligned (a " + kind_name(dst_kind) + " table of this dim)");
  if ((uintptr_t)src % fcpf::base_alignment(src_kind, vec))
    return fail(FCP_ERR_INVALID_ARGUMENT, std::string("fcp_table_convert: src is not ") + std::to_string(fcpf::base_alignment(src_kind, vec)) +
                                              "-byte aligned (a " + kind_name(src_kind) + " table of this dim)");
  if (dst_kind == src_kind)
    return fail(FCP_ERR_INVALID_ARGUMENT, "fcp_table_convert: dst_kind equals src_kind; exactly one of the two is FCP_TAB_F32");
  if (dst_kind != FCP_TAB_F32 && src_kind != FCP_TAB_F32)
    return fail(FCP_ERR_UNSUPPORTED, std::string("fcp_table_convert: ") + kind_name(src_kind) + " -> " + kind_name(dst_kind) +
                                         " is not implemented; convert through float32");
  if (rows == 0) return FCP_OK;
  void *first = static_cast<char *>(dst) + dst_row0 * fcp_table_row_bytes(dst_kind, dim);
  return on_device("fcp_table_convert", device, stream, [&](hipStream_t s) {
    with_vec(vec, [&](auto v) { convert<decltype(v)::value>(first, dst_kind, src, src_kind, rows, dim, s); });
  });
}
