// fcp_kernels.hip — hand-written gfx950 (CDNA4, MI355X) kernels of the fused
// feature-column path.  HBM-bound gather / pool / concat: no MFMA on purpose.
//
// Replaces, for every model, what the reference generates as CUDA text:
//   FusedKnl + struct FCi            graph_optimizers/cuda_emitter.cc:1976-2134
//   Bucketize                        :233-247
//   GatherRowsToGlbMem               :250-293
//   GatherScatterRows                :296-345
//   SparseSegmentSum / Mean          :402-501 / :564-661
//   experiment::ComputeSegmentOffsets / SparseSegmentReduce   :768-962
//   BatchColReduction                :1216-1241
//   ConcatOutputsKnl / ScatterBlock  custom_ops/concat_outputs/concat_outputs_op_gpu.cu.cc:85-131
//
// Work decomposition (the MI355X-first part).  The reference launches ONE
// 64-thread block per column (`FusedKnl<<<num_fc, 64>>>`, :2234) which walks
// the whole batch serially — at most #columns waves on the chip.  Here the unit
// of work is a *slot* of the concatenated output row: the output matrix
// [rows, sum(dim)] of a concat group is cut into V-float slots (V = 4 when all
// dims are multiples of 4: one 16-byte access per lane); a wave owns 64
// consecutive slots (1 KiB of one output row — spanning as many neighbouring
// columns as fit) for R consecutive batch rows, a 256-thread block owns that
// span for 4*R rows.  Consequences:
//   * every store instruction of a wave writes 1 KiB contiguous bytes of the
//     final concat layout — the concat pass and its intermediate arena vanish;
//   * a table row of dim floats is read by dim/4 adjacent lanes as one
//     contiguous run (coalesced into whole 64/128-byte requests);
//   * per block, the column records, the CSR row ranges and the ids of the
//     span are fetched ONCE (coalesced, one request per cache line) and staged in
//     LDS; the lanes then read them as LDS broadcasts;
//   * 1000 columns x batch 512 give 3840 blocks / 15360 waves instead of 1000
//     waves, enough to keep >16 MB of loads in flight (HBM latency x bandwidth);
//   * blocks that share a span (the same columns / tables) are given the same
//     `blockIdx % 8`, i.e. the same XCD and L2 under round-robin dispatch, so
//     skewed (Zipf) ids and small bucketize tables are served from one L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/fcp_hip.h"
#include <hip/hip_ext.h>
#include "fcp_internal.h"

#include "fcp_fused_launch.h"

namespace {

template <int V, bool SHARDED>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) fcp_ragged_kernel(const FcpLaunch L) {
  __shared__ __attribute__((aligned(16))) char smem[sizeof(RaggedLds)];
  ragged_body<V, SHARDED>(L, blockIdx.x, smem);
}

// (the hybrid launch: fcp_fused_launch.h)
template <int V, int R, bool SHARDED>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) fcp_hybrid_kernel(const FcpHybridLaunch H) {
  __shared__ __attribute__((aligned(16))) char smem[kHybridLds<R>];
  const int bid = blockIdx.x;
  if (bid < H.ragged_blocks) {
    ragged_body<V, SHARDED>(H.ragged, bid, smem); // the longer-running blocks are dispatched first
  } else {
    dense_body<V, R, SHARDED>(H.dense, bid - H.ragged_blocks, smem);
  }
}

// ---------------------------------------------------------------------------
// Segment-offset pre-pass: sorted segment ids -> CSR offsets[0..rows]
// (experiment::ComputeSegmentOffsets, cuda_emitter.cc:768-818: position idx
// writes offsets[id] = idx for id in (seg[idx-1], seg[idx]], seg[-1] = -1,
// seg[nnz] = rows).  The reference runs this serially inside one block per
// column; here one thread per position, all columns in one launch; the
// predecessor's id comes from the neighbouring lane (wave shuffle) and a
// wave without any segment boundary retires on one ballot.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int64_t load_seg(const char *seg, unsigned segkind, int stride, int64_t i) {
  if (segkind == FCP_SEG_IDS_I32) return *reinterpret_cast<const int32_t *>(seg + 4 * i * stride);
  return ld_i64_a4(seg + 8 * i * stride);
}

// Segment id of element i when it is a function of several index coordinates (FcpSegMap: a SparseReshape folded into
// the index expression, cuda_emitter.cc:1874-1916): (sum_k idx[i*stride + k] * mul[k]) / div, one factor scaled by the
// request's symbol.  Rare columns, cold code: out of line, 64-bit division and all.
__device__ __noinline__ int64_t load_seg_mapped(const char *seg, unsigned segkind, int stride, int64_t i, const FcpSegMap *mp,
                                                int64_t sym) {
  const FcpSegMap m = *mp;
  int64_t lin = 0;
  for (int k = 0; k < m.n; ++k) {
    const int64_t v = load_seg(seg, segkind, 1, i * stride + k);
    if (v < 0) return -1; // not an index: sorts before every row
    lin += v * (m.sym_slot == k ? m.mul[k] * sym : m.mul[k]);
  }
  const int64_t div = m.sym_slot == 4 ? m.div * sym : m.div;
  return lin / div;
}

// One block = FCP_SEG_IDS_PER_BLOCK consecutive positions of one column's id stream, in rounds of 256 (neighbouring
// lanes hold neighbouring ids); every load of the block is issued before the first boundary test, so the block is one
// memory round trip long whatever the number of rounds.  (Round 1: one id per thread, 4x the blocks — the same time
// alone, but with several requests in flight the small blocks held wave slots the other requests' kernels wanted:
// RAGGED with SparseTensor indices 28-30 us per request overlapped, 26-27 us with this form.)
#ifndef FCP_SEG_ROUNDS
#define FCP_SEG_ROUNDS 4
#endif
#define FCP_SEG_IDS_PER_BLOCK (FCP_SEG_ROUNDS * FCP_BLOCK_THREADS)
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_segment_offsets_kernel(const FcpSegLaunch L) {
  const int c = L.seg_cols[blockIdx.y];
  const FcpColDyn cd = L.dyn[c];
  const int nnz = cd.nnz;
  const int64_t base = (int64_t)blockIdx.x * FCP_SEG_IDS_PER_BLOCK;
  if (base > nnz) return;
  const FcpColStatic cs = L.cols[c];
  const unsigned segkind = FCP_F_SEGKIND(cs.flags);
  const int stride = cs.seg_stride;
  const int64_t rows = cd.rows;
  const char *seg = L.blob + cd.seg_off;
  const int lane = threadIdx.x & (FCP_WAVE - 1);
  int32_t *csr = reinterpret_cast<int32_t *>(L.arena + L.csr_arena_off) + cd.csr_base;
  if (FCP_F_FORM(cs.flags) == FCP_FORM_GATHER_SCATTER) {
    // ScatterNd row ids arrive in ANY order (GatherScatterRows, cuda_emitter.cc:296-345, scatters whatever it is
    // given): instead of row offsets the column's scratch (zeroed before this launch) receives the inverse map
    // inv[row] = 1 + the LAST position whose row id is `row` (atomic max: "the last write wins", the order of a
    // sequential scatter and of the oracle); ids the column's filter drops never reach the scatter.
    if (L.skip_inverse) return;
    const bool filtered = (cs.xform & 3u) == FCP_XFORM_FILTER;
    LdsCol lc;
    if (filtered) {
      static_cast<FcpColStatic &>(lc) = cs;
      lc.ids = L.blob + cd.ids_off;
      lc.csr = nullptr;
      lc.out_base = 0;
      lc.out_stride = 0;
      lc.nnz = nnz;
      lc.bnd_off = -1; // boundaries, if any, are read from global memory
    }
#pragma unroll 1
    for (int r = 0; r < FCP_SEG_ROUNDS; ++r) {
      const int64_t i = base + r * FCP_BLOCK_THREADS + threadIdx.x;
      if (i >= nnz) break;
      if (filtered) { // the filter op sits in front of the scatter: what it drops never gets there
        bool bad;
        if (fetch_slot_offset<1, false>(lc, L.xforms + c, i, nullptr, 0, 1, bad) == kFiltered) continue;
      }
      const int64_t row = load_seg(seg, segkind, stride, i);
      if (row < 0 || row >= rows) { // TF's ScatterNd on a GPU drops such rows
        if (L.bad_ids) atomicAdd(L.bad_ids, 1ull);
        continue;
      }
      atomicMax(csr + row, (int32_t)(i + 1));
    }
    return;
  }
  int64_t cur[FCP_SEG_ROUNDS], first_prev[FCP_SEG_ROUNDS];
  if (L.segmaps && L.segmaps[c].n > 0) { // (uniform per block)
    const FcpSegMap *mp = L.segmaps + c;
    const int64_t sym = cd.seg_sym;
#pragma unroll 1
    for (int r = 0; r < FCP_SEG_ROUNDS; ++r) {
      const int64_t i = base + r * FCP_BLOCK_THREADS + threadIdx.x;
      cur[r] = rows;
      if (i < nnz) cur[r] = load_seg_mapped(seg, segkind, stride, i, mp, sym);
      first_prev[r] = -1;
      if (lane == 0 && i > 0 && i <= nnz) first_prev[r] = load_seg_mapped(seg, segkind, stride, i - 1, mp, sym);
    }
  } else {
#pragma unroll
    for (int r = 0; r < FCP_SEG_ROUNDS; ++r) {
      const int64_t i = base + r * FCP_BLOCK_THREADS + threadIdx.x;
      cur[r] = rows;
      if (i < nnz) cur[r] = load_seg(seg, segkind, stride, i);
      first_prev[r] = -1;
      if (lane == 0 && i > 0 && i <= nnz) first_prev[r] = load_seg(seg, segkind, stride, i - 1); // the neighbour wave's last id
    }
  }
#pragma unroll
  for (int r = 0; r < FCP_SEG_ROUNDS; ++r) {
    const int64_t i = base + r * FCP_BLOCK_THREADS + threadIdx.x;
    const bool active = i <= nnz;
    const int64_t c0 = cur[r] > rows ? rows : cur[r];
    int64_t prev = __shfl_up(c0, 1);
    if (lane == 0) prev = first_prev[r] > rows ? rows : first_prev[r];
    const bool boundary = active && c0 > prev;
    // sorted-ascending is the caller's contract (TF SparseSegment*, SparseTensor indices); a descending step is
    // reported through the bad-id counter when the plan asks for it
    if (L.bad_ids && active && i < nnz && c0 < prev) atomicAdd(L.bad_ids, 1ull);
    if (boundary)
      for (int64_t id = prev + 1 < 0 ? 0 : prev + 1; id <= c0; ++id) csr[id] = (int32_t)i;
  }
}

// ---------------------------------------------------------------------------
// ConcatOutputs (reference layout pass, concat_outputs_op_gpu.cu.cc:85-131):
// out[p, off_k + e] = in_k[p*dim_k + e].  Used with FCP_LAYOUT_PER_COLUMN (hundreds of narrow inputs), by
// the host half of Addons>ConcatOutputs (a few payloads scattered into the EXTERNAL slots) and by the
// column-sharded step (8 wide blocks side by side: there it is half of a rank's work per request).
// One thread per VEC floats; a block is a tile of TY rows x TX vectors of one input, TX = the widest
// input of the launch rounded up to a power of two (at most 256), so that narrow inputs still fill
// their waves with rows.  No integer division per element, no grid cap (round 1: scalar copies behind a
// 64-block grid-stride loop: 2.35 TB/s on the 8 x [64, 15000] blocks of BASELINE configs[4]).
// ---------------------------------------------------------------------------
#define FCP_CONCAT_CHUNK 192
struct FcpConcatArgs {
  const float *in[FCP_CONCAT_CHUNK];
  int32_t off[FCP_CONCAT_CHUNK];
  int32_t dim[FCP_CONCAT_CHUNK];
  int32_t stride[FCP_CONCAT_CHUNK]; // row stride of the input in floats (= dim for a contiguous [prefix, dim] input)
  float *out;
  int64_t prefix;
  int32_t width;
  int32_t n;
  int32_t tx_log2; // threads along a row
  int32_t cpr;     // column chunks per row: ceil(max_dim / VEC / TX)
};

template <int VEC> __global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_concat_outputs_kernel(const FcpConcatArgs A) {
  const int k = blockIdx.y;
  const int dimv = A.dim[k] / VEC;
  const int tx = 1 << A.tx_log2;
  const int lx = threadIdx.x & (tx - 1), ly = threadIdx.x >> A.tx_log2;
  const int64_t tile = blockIdx.x / A.cpr;
  const int chunk = (int)(blockIdx.x - tile * A.cpr);
  const int64_t p = tile * (FCP_BLOCK_THREADS >> A.tx_log2) + ly;
  const int e = chunk * tx + lx;
  if (p >= A.prefix || e >= dimv) return;
  typedef typename VecType<VEC>::T T;
  const T v = *as_global(reinterpret_cast<const T *>(A.in[k]) + (p * (A.stride[k] / VEC) + e));
  __builtin_nontemporal_store(v, as_global(reinterpret_cast<T *>(A.out + (p * A.width + A.off[k])) + e));
}

// ---------------------------------------------------------------------------
// Row-shard finalize (no reference counterpart): after the
// all-to-all, rank h holds `world` partial-sum slices of its batch slice;
// add them in rank order (deterministic) and apply the mean division.
// ---------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(FCP_BLOCK_THREADS)
    fcp_shard_finalize_kernel(const FcpLaunch L, int g, const float *__restrict__ partials, int world,
                              int64_t row_begin, int64_t row_count, float *__restrict__ out, const int64_t *__restrict__ wts) {
  const int nslots = L.groups[g].nslots;
  const int nxb = (nslots + FCP_BLOCK_THREADS - 1) / FCP_BLOCK_THREADS; // blocks per output row (1-D grid: any row count)
  const int q = (int)(blockIdx.x % nxb) * FCP_BLOCK_THREADS + threadIdx.x;
  const int64_t bl = blockIdx.x / nxb;
  if (q >= nslots || bl >= row_count) return;
  const int64_t W = (int64_t)nslots * V;
  const uint32_t c = L.slot_map[L.groups[g].slot_map_off + q];
  const FcpColStatic cs = L.cols[c];
  const FcpColDyn cd = L.dyn[c];
  if (FCP_F_FORM(cs.flags) == FCP_FORM_EXTERNAL) return; // the hole stays for fcp_concat_outputs_host
  if (FCP_F_FORM(cs.flags) != FCP_FORM_SEGMENT_REDUCE) {
    // one owner per row (gather, scatter, passthrough, BatchColReduction): every other rank wrote +0.0, all bits clear, so
    // the OR of the slices' bits is the owner's value, -0.0 and NaN payloads included (a sum from +0.0 turns -0.0 into +0.0)
    VU<V> bits;
#pragma unroll
    for (int t = 0; t < V; ++t) bits.v[t] = 0u;
    for (int w = 0; w < world; ++w) {
      const VU<V> x = *reinterpret_cast<const VU<V> *>(partials + ((int64_t)w * row_count + bl) * W + (int64_t)q * V);
#pragma unroll
      for (int t = 0; t < V; ++t) bits.v[t] |= x.v[t];
    }
    *reinterpret_cast<VU<V> *>(out + bl * W + (int64_t)q * V) = bits;
    return;
  }
  VF<V> acc = vzero<V>();
  for (int w = 0; w < world; ++w) {
    const VF<V> x = *reinterpret_cast<const VF<V> *>(partials + ((int64_t)w * row_count + bl) * W + (int64_t)q * V);
#pragma unroll
    for (int t = 0; t < V; ++t) acc.v[t] = acc.v[t] + x.v[t];
  }
  // (a plan with shard_world == 1 is not sharded: its kernels have already divided)
  // MEAN and SQRTN; `wts` (plans with weighted columns): per column the byte offset of its weights in the blob, or -1
  const unsigned comb = FCP_F_COMBINER(cs.flags);
  if (L.shard_world > 1 && FCP_F_FORM(cs.flags) == FCP_FORM_SEGMENT_REDUCE && (comb == FCP_COMBINER_MEAN || comb == FCP_COMBINER_SQRTN)) {
    const unsigned segkind = FCP_F_SEGKIND(cs.flags);
    const int32_t *csr = segkind == FCP_SEG_CSR_I32
                             ? reinterpret_cast<const int32_t *>(L.blob + cd.seg_off)
                             : reinterpret_cast<const int32_t *>(L.arena + L.csr_arena_off) + cd.csr_base;
    const int64_t b = row_begin + bl;
    int lo = csr[b], hi = csr[b + 1];
    lo = min(max(lo, 0), cd.nnz);
    hi = min(max(hi, lo), cd.nnz);
    int kept = hi - lo;
    const int64_t wo = wts ? wts[c] : -1;
    const FCP_GLOBAL float *gw = wo >= 0 ? as_global(reinterpret_cast<const float *>(L.blob + wo)) : nullptr;
    float den = 0.0f; // weighted columns: the WHOLE row's weights (or their squares) in id order, whichever rank owned the id
    if (gw && (cs.xform & 3u) != FCP_XFORM_FILTER)
      for (int i = lo; i < hi; ++i) den = weight_den_step(den, gw[i], comb == FCP_COMBINER_SQRTN);
    if ((cs.xform & 3u) == FCP_XFORM_FILTER) {
      // ids the column's filter drops do not count in the mean; which ones they are does not depend on the
      // rank (hash and intervals are applied to the raw id, before the ownership test), so the finalizing
      // rank re-reads the row's ids and counts the kept ones
      LdsCol lc;
      static_cast<FcpColStatic &>(lc) = cs;
      lc.ids = L.blob + cd.ids_off;
      lc.csr = nullptr;
      lc.out_base = 0;
      lc.out_stride = 0;
      lc.nnz = cd.nnz;
      lc.bnd_off = -1; // boundaries, if any, are read from global memory
      kept = 0;
      for (int i = lo; i < hi; ++i) {
        bool bad;
        const bool keep = fetch_slot_offset<V, false>(lc, L.xforms + c, i, nullptr, 0, 1, bad) != kFiltered;
        kept += keep ? 1 : 0;
        if (gw && keep) den = weight_den_step(den, gw[i], comb == FCP_COMBINER_SQRTN);
      }
    }
    // (unweighted MEAN: kept == 0 leaves the sum of the slices, +0.0 in every element, as before)
    float fc = gw ? den : (float)kept;
    if (comb == FCP_COMBINER_SQRTN) fc = sqrtf(fc); // (correctly rounded, as in the kernels)
    if (fc == 0.0f) {
      acc = vzero<V>();
    } else {
#pragma unroll
      for (int t = 0; t < V; ++t) acc.v[t] = acc.v[t] / fc;
    }
  }
  *reinterpret_cast<VF<V> *>(out + bl * W + (int64_t)q * V) = acc;
}


// ---------------------------------------------------------------------------
// Descriptor upload: copies the request's FcpColDyn[] from pinned host memory
// (read over PCIe through its device mapping) into device memory.  Stands in
// for the reference's per-call cudaMemcpyAsync of KnlArgs (cuda_emitter.cc
// :2216); hipMemcpyAsync of these ~10-50 KB cost ~28 us per request end to end
// on this path, a 2-block kernel costs a few.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_upload_kernel(const uint4 *__restrict__ src,
                                                                       uint4 *__restrict__ dst, int n16) {
  for (int i = blockIdx.x * FCP_BLOCK_THREADS + threadIdx.x; i < n16; i += gridDim.x * FCP_BLOCK_THREADS)
    dst[i] = src[i];
}

} // namespace

// ---------------------------------------------------------------------------
// The request stager's copy as a KERNEL (FCP_STAGER_COPY_KERNEL): bytes [0, n) from the pinned staging ring (read over
// PCIe through its device mapping) to the slot's device twin.  src and dst are 4-byte aligned and equally misaligned
// against 16 bytes (the same offset into two page-aligned buffers), n is a multiple of 4: head and tail by dwords, the
// body by 16-byte words, four independent loads in flight per thread (a PCIe read is ~2 us away: 64 blocks x 256
// threads x 4 x 16 B = 1 MB requested per round).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(FCP_BLOCK_THREADS) fcp_h2d_copy_kernel(const char *__restrict__ src, char *__restrict__ dst, size_t n) {
  const size_t head = min((size_t)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15), n);
  const size_t body = (n - head) & ~(size_t)15, tail = n - head - body;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  if (t < head / 4) reinterpret_cast<uint32_t *>(dst)[t] = reinterpret_cast<const uint32_t *>(src)[t];
  if (t < tail / 4) reinterpret_cast<uint32_t *>(dst + head + body)[t] = reinterpret_cast<const uint32_t *>(src + head + body)[t];
  const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
  uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
  const size_t n4 = body / 16;
  for (size_t i = t; i < n4; i += 4 * nt) {
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k * nt < n4) v[k] = s4[i + k * nt];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k * nt < n4) d4[i + k * nt] = v[k];
  }
}

// ------------------------------- launchers ---------------------------------

// Private-stream requests (fcp_lanes.hip): the completion event of a request is attached to the dispatch packet of its
// LAST kernel (hipExtLaunchKernelGGL's stop event) instead of being recorded as a marker packet of its own behind it.
// Thread-local: set by the request path just before it enqueues, taken (and cleared) by the fused / hybrid launcher.
static thread_local hipEvent_t tl_stop_event = nullptr;
void fcp_set_stop_event(void *ev) { tl_stop_event = static_cast<hipEvent_t>(ev); }
bool fcp_stop_event_pending() { return tl_stop_event != nullptr; }
// FCP_ORDER_INPUTS_READY plans (fcp_plan_set_request_order): the next fused / hybrid launch of this thread goes out WITHOUT
// the barrier bit (hipExtAnyOrderLaunch): the command processor need not wait for the queue to drain before it takes the
// packet, which makes the hand-over between two requests cheaper (S2: 28.3 -> 26.0-26.5 us per request back to back on one
// stream, no events, no extra streams).  It does NOT start while blocks of the kernel in front of it still run, not even
// into its tail (round 5, scripts/probes/any_order_probe.hip: 21.4 us after the start of a predecessor whose blocks retire
// between 10 and 20 us, against 22.7 us with the barrier bit).
static thread_local int tl_launch_flags = 0;
void fcp_set_any_order(bool on) { tl_launch_flags = on ? (int)hipExtAnyOrderLaunch : 0; }
// what fcp_klaunch (fcp_fused_launch.h) and the plain dense kernel's launcher take, and clear
void fcp_take_launch_extras(void **stop_event, int *flags) {
  *stop_event = tl_stop_event;
  *flags = tl_launch_flags;
  tl_stop_event = nullptr;
  tl_launch_flags = 0;
}

// the float32 matrix: every kernel in a sharded and an unsharded instantiation
int fcp_launch_f32(const FcpFusedWork &W, ihipStream_t *s) {
  if (W.dense_blocks <= 0 && W.ragged_blocks <= 0) return 0;
  int e = 0;
  with_bool(fcp_work_sharded(W), [&](auto SHARDED) {
    constexpr bool SH = decltype(SHARDED)::value;
    e = fcp_launch_work(
        W, s, [](auto V, auto R) { return fcp_dense_kernel<V, R, SH>; }, [](auto V) { return fcp_ragged_kernel<V, SH>; },
        [](auto V, auto R) { return fcp_hybrid_kernel<V, R, SH>; });
  });
  return e;
}

// Launch counters of the kernels outside the fused matrix (fcp_aux_launch_counts): process-wide, relaxed — the stager's
// copies are enqueued from pack-pool threads.  A launch counts once the runtime has taken it.
static std::atomic<int64_t> g_aux_launches[FCP_AUX_KERNELS];
static int counted(int which, int err) {
  if (!err) g_aux_launches[which].fetch_add(1, std::memory_order_relaxed);
  return err;
}
// FCP_AUX_*_V4 / _V2 / _V1 follow each other
static int vec_slot(int vec) { return vec == 4 ? 0 : (vec == 2 ? 1 : 2); }

extern "C" int fcp_aux_launch_counts(int64_t *counts, int32_t capacity, int32_t reset) {
  if (capacity < 0 || (capacity > 0 && !counts)) return -FCP_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < FCP_AUX_KERNELS; ++i) {
    const int64_t v = reset ? g_aux_launches[i].exchange(0, std::memory_order_relaxed) : g_aux_launches[i].load(std::memory_order_relaxed);
    if (i < capacity) counts[i] = v;
  }
  return FCP_AUX_KERNELS;
}

int fcp_launch_h2d_copy(const void *host_mapped_src, void *dst, size_t bytes, ihipStream_t *s) {
  if (bytes == 0) return 0;
  if ((bytes & 3) || ((reinterpret_cast<uintptr_t>(host_mapped_src) ^ reinterpret_cast<uintptr_t>(dst)) & 15) ||
      (reinterpret_cast<uintptr_t>(dst) & 3))
    return (int)hipErrorInvalidValue;
  const int blocks = (int)std::min<size_t>(64, (bytes / 16 + FCP_BLOCK_THREADS - 1) / FCP_BLOCK_THREADS + 1);
  hipLaunchKernelGGL(fcp_h2d_copy_kernel, dim3(blocks), dim3(FCP_BLOCK_THREADS), 0, s, static_cast<const char *>(host_mapped_src),
                     static_cast<char *>(dst), bytes);
  return counted(FCP_AUX_H2D_COPY, (int)hipGetLastError());
}

int fcp_launch_upload(const void *host_mapped_src, void *dst, size_t bytes, ihipStream_t *s) {
  const int n16 = (int)((bytes + 15) / 16);
  if (n16 <= 0) return 0;
  const int blocks = n16 >= 4096 ? 8 : (n16 >= 1024 ? 4 : 1);
  hipLaunchKernelGGL(fcp_upload_kernel, dim3(blocks), dim3(FCP_BLOCK_THREADS), 0, s,
                     static_cast<const uint4 *>(host_mapped_src), static_cast<uint4 *>(dst), n16);
  return counted(FCP_AUX_UPLOAD, (int)hipGetLastError());
}

// any_order: FCP_ORDER_INPUTS_READY plans — the pre-pass reads the blob and writes the new arena's scratch only, so it needs
// no barrier against the previous request's kernel (a cheaper hand-over); the fused kernel behind it keeps the barrier bit
// and waits for it
int fcp_launch_segment_offsets(const FcpSegLaunch &L, int n_seg_cols, int max_nnz, ihipStream_t *s, bool any_order) {
  if (n_seg_cols <= 0) return 0;
  const int gx = (max_nnz + 1 + FCP_SEG_IDS_PER_BLOCK - 1) / FCP_SEG_IDS_PER_BLOCK;
  if (any_order)
    hipExtLaunchKernelGGL(fcp_segment_offsets_kernel, dim3(gx, n_seg_cols), dim3(FCP_BLOCK_THREADS), 0, s, nullptr, nullptr,
                          (int)hipExtAnyOrderLaunch, L);
  else
    hipLaunchKernelGGL(fcp_segment_offsets_kernel, dim3(gx, n_seg_cols), dim3(FCP_BLOCK_THREADS), 0, s, L);
  return counted(FCP_AUX_SEGMENT_OFFSETS, (int)hipGetLastError());
}

int fcp_launch_concat_outputs(const void *const *inputs, const int32_t *dims, const int32_t *col_offsets, const int32_t *in_strides,
                              int32_t n, int64_t prefix, int32_t width, int32_t first_off, void *out,
                              ihipStream_t *s) {
  int32_t off = first_off;
  for (int32_t begin = 0; begin < n; begin += FCP_CONCAT_CHUNK) {
    FcpConcatArgs A;
    const int32_t m = (n - begin) < FCP_CONCAT_CHUNK ? (n - begin) : FCP_CONCAT_CHUNK;
    int32_t max_dim = 1;
    for (int32_t k = 0; k < m; ++k) {
      A.in[k] = static_cast<const float *>(inputs[begin + k]);
      A.dim[k] = dims[begin + k];
      A.stride[k] = in_strides ? in_strides[begin + k] : dims[begin + k];
      A.off[k] = col_offsets ? col_offsets[begin + k] : off;
      off += dims[begin + k];
      if (dims[begin + k] > max_dim) max_dim = dims[begin + k];
    }
    A.out = static_cast<float *>(out);
    A.prefix = prefix;
    A.width = width;
    A.n = m;
    // widest vector every address of the launch is aligned for
    int vec = 4;
    uintptr_t bits = reinterpret_cast<uintptr_t>(out) | (uintptr_t)(4u * (uint32_t)width);
    for (int32_t k = 0; k < m; ++k)
      bits |= reinterpret_cast<uintptr_t>(A.in[k]) | (uintptr_t)(4u * (uint32_t)A.dim[k]) | (uintptr_t)(4u * (uint32_t)A.off[k]) |
              (uintptr_t)(4u * (uint32_t)A.stride[k]);
    while (vec > 1 && (bits & (uintptr_t)(4 * vec - 1))) vec >>= 1;
    const int max_dimv = (max_dim + vec - 1) / vec;
    int tx_log2 = 0;
    while ((1 << tx_log2) < max_dimv && (1 << tx_log2) < FCP_BLOCK_THREADS) ++tx_log2;
    A.tx_log2 = tx_log2;
    A.cpr = (max_dimv + (1 << tx_log2) - 1) >> tx_log2;
    const int ty = FCP_BLOCK_THREADS >> tx_log2;
    const int64_t gx = (prefix + ty - 1) / ty * A.cpr;
    if (gx <= 0) continue;
    if (gx > 0x7fffffff) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)m), block(FCP_BLOCK_THREADS);
    with_int<4, 2, 1>(vec, [&](auto V) { hipLaunchKernelGGL(fcp_concat_outputs_kernel<V>, grid, block, 0, s, A); });
    const int err = counted(FCP_AUX_CONCAT_V4 + vec_slot(vec), (int)hipGetLastError());
    if (err) return err;
  }
  return 0;
}

int fcp_launch_shard_finalize(const FcpLaunch &L, int group, const float *partials, int world,
                              int64_t row_begin, int64_t row_count, float *out, int vec,
                              ihipStream_t *s, const int64_t *wts) {
  if (row_count <= 0) return 0;
  const int nslots = L.groups[group].nslots;
  const int64_t nblocks = (int64_t)((nslots + FCP_BLOCK_THREADS - 1) / FCP_BLOCK_THREADS) * row_count;
  if (nblocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)nblocks);
  with_int<4, 2, 1>(vec, [&](auto V) {
    hipLaunchKernelGGL(fcp_shard_finalize_kernel<V>, grid, dim3(FCP_BLOCK_THREADS), 0, s, L, group, partials, world, row_begin,
                       row_count, out, wts);
  });
  return counted(FCP_AUX_SHARD_FINALIZE_V4 + vec_slot(vec), (int)hipGetLastError());
}
