// fcp_host.h — what the host-side translation units of libfcp_hip.so share: the plan object, the per-request descriptor
// cache, the private-stream (lane) state and the helpers that cross files.  Internal: nothing here is part of the ABI
// (include/fcp_hip.h).  Round 6 carved the single 3 700-line fcp_api.hip into
//   fcp_plan.hip     the device half of the plan object: const buffers, static records and device resources; accessors
//   fcp_process.hip  the request path: descriptor slots, launch records, fcp_internal_process, fcp_process_feature_columns
//   fcp_lanes.hip    plan-owned private streams (EXPERIMENTAL): lanes, verification, supervisor, result registry
//   fcp_concat.hip   Addons>ConcatOutputs entry points and fcp_shard_finalize
//   fcp_stager.hip   Addons>ConcatInputs packers, the request stager, the pack pool
// and the levels that need no GPU header became units of ordinary C++:
//   fcp_plan_desc.cc  validation, the formats' refusals, plan files, the placement gate, fcp_last_error (fcp_plan_desc.h)
//   fcp_plan_shape.cc the host half of the plan (HostPlan, build_host_plan) and shape evaluation (evaluate_shapes): per-column
//                     records, arena layout and launch geometry from a request's shapes (fcp_plan_shape.h)
//   fcp_formats.h     the one table of the storage formats' facts (names, flag bits, element and row sizes)
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fcp_hip.h"
#include "fcp_internal.h"
#include "fcp_env.h"
#include "fcp_formats.h"
#include "fcp_plan_desc.h"
#include "fcp_plan_shape.h"

namespace fcph {

int hip_fail(const char *what, hipError_t e); // (fail: fcp_plan_desc.h)

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return hip_fail(#expr, e_);   \
  } while (0)

constexpr int kSlots = 32; // descriptor slots per plan: distinct (shapes, stream) pairs resident at once (8 until round 4: 16 rotating shapes reinstalled on every request)

constexpr int kAllSlotsBusy = -2; // find_or_reserve: every slot is pinned by a concurrent request
constexpr int kNeedsInstall = -3; // find_or_reserve during stream capture: these shapes are not resident

struct DynSlot {
  bool valid = false;
  std::vector<int32_t> key;
  FcpColDyn *h_dyn = nullptr; // pinned, mapped (host copy; source of the upload-kernel path)
  void *h_dyn_dev = nullptr;  // device-side address of h_dyn
  FcpColDyn *d_dyn = nullptr; // what the kernels read
  hipEvent_t uploaded = nullptr; // upload-kernel path: recorded after the upload
  uint64_t done_gen = 0;         // != 0: `done` is a private lane's completion event of that lane generation (see g_lane_generation)
  hipEvent_t done = nullptr;     // recorded after the first kernel that used this content; one event per
                                 // (slot, stream) — re-recording an event last used on ANOTHER stream costs
                                 // ~20 us under concurrency (HIP serialises it), on its own stream < 1 us
  std::vector<std::pair<void *, hipEvent_t>> done_pool;
  bool done_valid = false;       // `done` covers every kernel that has used this content so far
  void *stream = nullptr;        // stream of the request that installed this content
  uint64_t tick = 0;
  int users = 0;                 // requests between "slot chosen" and "kernels enqueued": not evictable
  int uses = 0;                  // requests that have used this content since it was installed
  bool captured = false;         // a stream capture recorded a launch that reads this slot: a graph replay will read
                                 // it at any later time, so it is never evicted (fcp_plan_release_captures)
  bool img_built = false;        // plain dense plans: the slot holds a span image (rewritten when tables are re-bound); under the plan's mutex
  bool was_valid = false;        // reserved for installation: the previous content had readers to wait for
  DynMeta meta;
};

// One private stream of a plan (fcp_plan_set_private_streams).  A request that takes the lane holds `mu` while it
// enqueues (record on the caller's stream, wait on the lane, kernels, record on the lane), so an event pair is never
// interleaved between two host threads.  Events rotate: re-recording an event that an older consumer has not waited
// for yet makes that consumer wait for LATER work of the same lane, which covers the older request (same stream).
constexpr int kLaneEvents = 8;
constexpr int kMaxPoolLanes = 16; // (more than three only for experiments: FCP_PRIVATE_LANES_UNCAPPED)
struct PrivateLane {
  hipStream_t stream = nullptr;
  std::mutex mu;
  hipEvent_t in[kLaneEvents] = {};  // recorded on the caller's stream: everything the request may depend on
  hipEvent_t out[kLaneEvents] = {}; // recorded on the lane behind the request's last kernel
  uint32_t next = 0;
};

// The private lanes of ONE DEVICE, shared by every plan on it (created on first use, kept for the life of the process).
// The command processor overlaps at most four event-linked queues — a caller's stream and three lanes; with a fifth every
// request costs a multiple (profiles/r04_private_streams_queue_mapping.txt).  Lanes per plan would multiply them: two
// models served by one process, three lanes each, fall off that cliff as soon as both are busy.
// Lanes are destroyed and re-created only while no live plan relies on them (verify_lanes), i.e. after every plan that used
// them has synchronised them and let go.  A descriptor slot whose `done` event is a lane's completion event remembers the
// generation it was taken from: a different generation now means those lanes — and every kernel that ran on them — are gone.
extern std::atomic<uint64_t> g_lane_generation;
// the completion event of the private-stream request this thread is issuing (fcp_process_feature_columns -> fcp_internal_process)
extern thread_local hipEvent_t tl_lane_done;
extern thread_local uint64_t tl_lane_done_gen;

// What a private-stream request waits for on the caller's stream is known only once the allocator has answered: TF's
// allocator hands out memory in compute-stream order, and between this call's entry and its malloc_buff another
// Session::Run thread may have queued a kernel that still reads the very memory the arena gets.  So
// fcp_process_feature_columns leaves the dependency here and fcp_internal_process enqueues it — event record on the caller's
// stream, wait on the lane — right behind malloc_buff, in front of the first command that touches the arena.
struct LaneDep {
  hipEvent_t in;
  hipStream_t caller, lane;
};
extern thread_local const LaneDep *tl_lane_dep;
// gathered + written bytes of the request this thread processed last (DynMeta::work_bytes; the supervisor's unit of work)
extern thread_local int64_t tl_work_bytes;

// Supervision of one plan's lane traffic behind ONE caller stream (the first that took the lanes; TensorFlow has one): an
// online A/B of the two ways a request can run, under the caller's REAL traffic — its consumers, its host threads, its pace.
//   evaluation: kSupWindow consecutive requests run on the CALLER's stream between two timing events there (time per byte of
//               work in stream order), the next kSupWindow on the private streams between two timing events on one of them
//               (the second behind the first request >= kSupWindow later that lands on the same lane); ratio = lanes / stream
//               order.  No idle / busy heuristics: a caller that issues sparsely measures ~1.0 in both (nothing to overlap:
//               the lanes buy nothing), readers right behind their requests measure > 1 (the events are pure cost), lanes
//               that overlap measure 0.64-0.92, a hardware-queue mapping that stopped overlapping 1.1 and more
//               (profiles/r05_caller_threads_grid.txt).
//   decision:   two consecutive evaluations with ratio > keep_ratio (0.97): the caller is DEMOTED — verdict 0, one line on
//               stderr, its requests stay on its stream; two consecutive ones below it re-admit a demoted caller (traffic
//               changes: a trickle at start-up, load later).  One evaluation alone never switches.
//   schedule:   the first at the caller's first eligible request, the next after 256 requests, then the gap doubles up to
//               `period` (8192): one evaluation costs kSupWindow requests in the mode that loses, < 1 % of the traffic.
// Cost outside evaluations: one mutex and a counter per request.
constexpr int kSupWindow = 48;
struct LaneSupervisor {
  std::mutex mu;
  bool on = true;
  uint32_t period = 8192, first_gap = 256;
  double keep_ratio = 0.97;
  void *caller = nullptr;
  bool use_lanes = true;        // the mode requests run in between evaluations
  uint64_t seq = 0;             // eligible requests of the supervised caller so far
  uint64_t next_eval = 1, gap = 256;
  // phase of the running evaluation: 0 none, 1 stream-order window open, 2 lane window to open, 3 lane window open,
  // 4 both closed (events pending)
  int phase = 0;
  hipEvent_t b0 = nullptr, b1 = nullptr; // on the caller's stream
  hipEvent_t w0 = nullptr, w1 = nullptr; // on one lane
  PrivateLane *w_lane = nullptr;
  int so_count = 0, w_count = 0;
  int64_t so_bytes = 0, w_bytes = 0;
  int strikes = 0;              // consecutive evaluations that contradict the present mode
  uint64_t evaluations = 0, lane_requests = 0;
  double so_ns_per_byte = 0, last_ratio = 0, worst_ratio = 0;
  bool demoted = false;         // == !use_lanes after at least one decision
};

struct LanePool {
  std::mutex cal_mu;                                  // lanes / spacers are created, probed and re-created under it
  std::vector<std::unique_ptr<PrivateLane>> lanes;
  std::vector<hipStream_t> spacers;                   // streams that only hold hardware queues (verify_lanes)
  std::atomic<int> n_relying{0};                      // live plans that found the present mapping good, or use it unverified
  std::atomic<uint32_t> rr{0};
  // Test aid (FCP_DIAG=lane_fault_us=N, read by fcp_plan_set_private_streams): every lane request first waits for the device's
  // previous lane request and then spins for N us on its lane — lanes that serialise and stall, the signature of a
  // hardware-queue mapping that does not overlap (profiles/r04_private_streams_queue_mapping.txt: 29-86 us per S2
  // request), made deterministic for the supervisor's test.
  std::atomic<int> fault_us{0};
  std::atomic<hipEvent_t> last_out{nullptr};
};
void sup_reset(LaneSupervisor &S, const fcp::Env &env);
LanePool *lane_pool_for(int device);

// Results whose kernels run on a private lane, by arena address range: what fcp_result_wait looks up.  An entry is
// replaced when its address range is handed out again and dropped once its event has completed (nothing to wait for).
struct PendingResult {
  uintptr_t end;
  hipEvent_t done;
  const void *owner; // the plan whose lane owns `done`
};
// (fcp_lanes.hip) the registry of results / inputs whose kernels run on a private lane
void pending_register(const void *owner, void *arena, int64_t bytes, const void *blob, int64_t blob_bytes, hipEvent_t done);
void pending_clear_range(void *arena, int64_t bytes);
void pending_forget(const void *owner);
int stager_input_wait(const void *base, int64_t bytes, hipStream_t stream);
int stager_input_synchronize(const void *base, int64_t bytes);
int wait_for_inputs(const void *const *inputs, int32_t n, void *stream);

} // namespace fcph
using namespace fcph; // (an internal header: every includer is one of the five files above)

// The plan: its host half (fcp_plan_shape.h: everything decided without a device) and, here, what needs HIP or a device.
struct fcp_plan : fcph::HostPlan {
  uint32_t *d_span_list = nullptr; // device copy of span_list
  uint32_t *d_slot_map = nullptr;
  FcpColStatic *d_cols = nullptr;
  FcpXform *d_xforms = nullptr; // per column, only for plans with id transforms
  FcpSegMap *d_segmaps = nullptr; // per column, only for plans with segment-id maps
  // Plain dense plan (fcp_dense_plain.hip): float32 concat output, one group, unsharded, V 4, no wide rows, no id transform,
  // every column a gather by int32 / int64 ids or by float32 values bucketized with reproducible boundaries.  Decided at
  // plan creation (FCP_DIAG=dense_generic keeps such a plan on the generic kernel).  Every descriptor slot then carries,
  // behind its FcpColDyn records, the per-span image: plain_spans records of plain_stride bytes.  plain_tmpl is the image
  // with everything that does not depend on the request or the bound tables; plain_entries names, per FcpPlainCol of the
  // image, its byte offset there and the column (concat position) it describes.
  bool plain_dense = false;
  // The plain kernel's block mapping (fcp_plain_map.h): the partial last group of eight spans dealt evenly over the XCDs,
  // or the generic kernel's.  FCP_DIAG=plain_even_deal=0|1 at plan creation; the default is FCP_PLAIN_EVEN_DEAL_DEFAULT.
  bool plain_even_deal = false;
  // FCP_DIAG=store_policy=sc1 at plan creation: every launch of the plain dense kernel stores `sc1`, whatever the output
  // size or the arena (the A/B's and the tests' seam; store_policy_for).  No other kernel has the form or reads the key.
  bool plain_store_sc1 = false;
  int32_t plain_stride = 0, plain_spans = 0, plain_cols_off = 0; // (plain_cols_off: FcpPlainSpan::cols_off of every record)
  std::vector<char> plain_tmpl;
  std::vector<std::pair<uint32_t, int32_t>> plain_entries;
  std::atomic<int32_t> last_dense_front{0}; // fcp_plan_last_dense_front: FCP_DENSE_FRONT_* of the last request
  std::vector<FcpColStatic> h_cols;
  char *d_const = nullptr;
  int32_t *d_seg_cols = nullptr;
  unsigned long long *d_bad = nullptr;
  float *d_zeros = nullptr;     // 256 zero bytes (a q8 plan: its longest row, rounded up): the row a skipped id of a bag reads (ld_slot_or_zero)
  std::vector<const void *> bound_tables;
  bool tables_bound = false;
  // Traffic counting (fcp_plan_traffic_bind / fcp_plan_traffic_count, fcp_table_traffic.hip): the counted lookup columns in
  // concat order with the count array of each one's table (device array of one entry per plan column, allocated by the first
  // bind; the first traffic_n entries are live), and the caller's skipped counter.  Under the plan's mutex.
  FcpTrafficCol *d_traffic = nullptr;
  int32_t traffic_n = 0; // 0: nothing is bound
  unsigned long long *traffic_skipped = nullptr;

  // How new shape-dependent descriptors reach the device (dynamic shapes: every
  // request).  With a large PCIe BAR the descriptor ring lives in fine-grained
  // device memory and the HOST writes it directly (posted writes, ~0.3 us for 24 KiB,
  // nothing on the GPU's critical path); otherwise a small kernel on the request's
  // stream copies it from pinned host memory.  FCP_DYN_UPLOAD=kernel forces the latter.
  bool host_writes_dyn = false;
  std::mutex mu;
  DynSlot slots[kSlots];
  uint64_t tick = 0;

  // Plan-owned private streams (fcp_plan_set_private_streams): requests of ONE caller stream run on a rotating set of
  // lanes so that consecutive requests overlap on the GPU (the front of one launch under the memory phase of another).
  LanePool *pool = nullptr;                             // the device's lanes; the plan uses the first lane_count of them
  uint32_t lane_flags = 0;
  // Verification (verify_lanes): whether event-linked streams overlap depends on the hardware queues the runtime mapped
  // them to, which no API shows.  The first request of every caller stream runs a synthetic probe of the request pattern;
  // while no caller has been found good, other mappings are tried (lanes re-created with another priority, behind
  // `spacers` — streams that only hold hardware queues); a caller behind which no mapping overlaps keeps its requests.
  std::vector<std::pair<void *, bool>> lane_verdicts;   // caller stream -> its requests may take the lanes (under pool->cal_mu)
  std::atomic<void *> lane_good_caller{nullptr};        // the last caller found good: the request path's shortcut
  int32_t lane_count = 0;                               // lanes asked for (<= kMaxLanes); 0: private streams off
  std::atomic<bool> lane_relies{false};                 // counted in pool->n_relying
  // The cross-stream events of a lane cost the host ~8 us per request and the GPU's command processor a few packets:
  // a request pays for them only when its kernel is long enough to have something to overlap.  The plan remembers
  // the work of the shapes it installed last (gathered rows + output bytes); lighter requests stay on the caller's stream.
  std::atomic<int64_t> last_work_bytes{0};
  int64_t lane_min_work = 0;
  int32_t request_order = FCP_ORDER_STREAM; // fcp_plan_set_request_order
  std::atomic<uintptr_t> recent_arena[2] = {}; // the arenas of the last two requests (store_policy_for)
  // what the last request enqueued (fcp_plan_last_launch): written with relaxed stores beside the values the request path
  // computes anyway, read by diagnostics only
  struct LastLaunch {
    std::atomic<int32_t> kernel{0}, rows_per_wave{0}, store_policy{0}, dense_blocks{0}, ragged_blocks{0}, segment_offsets{0};
    // fcp_plan_last_csr: the segment-offset scratch (arena byte offset, -1 before the first request) and, per plan column,
    // its int32 index there (only seg_cols have one; the others stay -1)
    std::atomic<int64_t> csr_arena_off{-1};
    std::unique_ptr<std::atomic<int32_t>[]> csr_base;
  } last_launch;
  // Run-time supervision of the lanes (LaneSupervisor below): a verdict is learnt once, a mapping can go bad later (another
  // library of the process creates streams; the runtime re-maps queues): sampled windows of lane requests are timed
  // against the stream-order rate of the same requests and the caller is demoted to its own stream when they lose.
  std::atomic<bool> lane_demoted{false};                // some caller of this plan has been demoted (NO_VERIFY plans look it up)
  LaneSupervisor sup;
  std::atomic<bool> sup_window{false};                  // a timing window of an evaluation is open (sup.phase 1 or 3): what a
                                                        // request that bypasses the supervisor looks at (sup_abort)
};

namespace fcph {

struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  int enter(int dev) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return hip_fail("hipGetDevice", e);
    if (prev != dev) {
      e = hipSetDevice(dev);
      if (e != hipSuccess) return hip_fail("hipSetDevice", e);
      changed = true;
    }
    return FCP_OK;
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

// What the table entries do behind their argument checks: enter the device, enqueue(stream) — launches only — and report a
// failed launch as "<who>: kernel launch".
template <class F> int on_device(const char *who, int32_t device, void *stream, F enqueue) {
  DeviceGuard guard;
  const int rc = guard.enter(device);
  if (rc) return rc;
  enqueue(static_cast<hipStream_t>(stream));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FCP_OK : hip_fail((std::string(who) + ": kernel launch").c_str(), e);
}

// Pinned, mapped staging that an entry fills on the host and a kernel (or a copy) of its stream reads: a ring of four slots per
// device, each grown on demand from a 64 KiB floor.  A slot is free again once the reader that was enqueued behind it has run
// (its event, recorded by Lease::record), so the caller's host arrays may go as soon as the call returns and the call never
// waits for the GPU in the steady state.  The TYPE is shared; every entry that stages keeps an object of its own, so the calls
// in flight that one entry admits do not depend on another's (fcp_concat_outputs_host, fcp_outputs_compare).
struct StageRings {
  struct Slot {
    char *buf = nullptr, *buf_dev = nullptr; // buf_dev: the device mapping of buf
    size_t cap = 0;
    hipEvent_t read = nullptr;
    bool busy = false; // reserved by a call that is filling it / enqueueing its reader (under the ring's mutex)
  };
  struct Ring {
    std::mutex mu; // covers `next` and the slots' `busy` flags only: callers fill and launch outside it
    Slot slots[4];
    size_t next = 0;
  };
  // A reserved slot; gives it back when it goes.
  struct Lease {
    char *buf = nullptr, *buf_dev = nullptr;
    Ring *ring = nullptr;
    Slot *slot = nullptr;
    // behind the slot's last reader on `stream`: the slot is free once that has run
    int record(hipStream_t stream) {
      HIP_TRY(hipEventRecord(slot->read, stream));
      return FCP_OK;
    }
    ~Lease() {
      if (!slot) return;
      std::lock_guard<std::mutex> lock(ring->mu);
      slot->busy = false;
    }
  };
  std::mutex mu;
  std::vector<Ring *> rings; // by device; a ring lives as long as the process (pinned memory is freed at exit)

  // Reserve a slot of `device`'s ring (yielding while all four are taken), wait for its previous reader if that is still
  // running, and make it hold `bytes`.  The caller has entered the device.
  int acquire(int device, size_t bytes, Lease *lease) {
    {
      std::lock_guard<std::mutex> lock(mu);
      if ((int)rings.size() <= device) rings.resize(device + 1, nullptr);
      if (!rings[device]) rings[device] = new Ring();
      lease->ring = rings[device];
    }
    Ring *ring = lease->ring;
    for (;;) {
      {
        std::lock_guard<std::mutex> lock(ring->mu);
        for (int t = 0; t < 4 && !lease->slot; ++t) {
          Slot &c = ring->slots[(ring->next + t) % 4];
          if (!c.busy) {
            c.busy = true;
            ring->next = (ring->next + t + 1) % 4;
            lease->slot = &c;
          }
        }
      }
      if (lease->slot) break;
      std::this_thread::yield(); // more than four calls in flight on this device
    }
    Slot &sl = *lease->slot;
    if (sl.read && hipEventQuery(sl.read) != hipSuccess) HIP_TRY(hipEventSynchronize(sl.read));
    if (sl.cap < bytes) {
      if (sl.buf) HIP_TRY(hipHostFree(sl.buf));
      sl.buf = nullptr;
      sl.buf_dev = nullptr;
      sl.cap = 0;
      const size_t cap = std::max<size_t>(bytes, 1 << 16);
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sl.buf), cap, hipHostMallocMapped));
      HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&sl.buf_dev), sl.buf, 0));
      sl.cap = cap;
    }
    if (!sl.read) HIP_TRY(hipEventCreateWithFlags(&sl.read, hipEventDisableTiming));
    lease->buf = sl.buf;
    lease->buf_dev = sl.buf_dev;
    return FCP_OK;
  }
};

bool stream_is_capturing(hipStream_t stream); // (fcp_process.hip)

// A host-built descriptor image into the caller's workspace, for the kernels the entry enqueues behind it on `stream`: the one
// place that orders the slot's hand-over.  The caller has entered the device.  In this order: a capturing stream is refused
// (FCP_ERR_UNSUPPORTED, "<who>: " + capture_refusal; null where the caller has refused it already); *d_image is the workspace's
// first 16-byte boundary; a slot of `rings` is leased; fill(char *slot) writes all image_bytes on the host, the padding of its
// sections as zeros (the slot holds an earlier call's bytes; zeroing it whole here cost fcp_outputs_compare a microsecond in
// a thousand columns); a fence; the upload kernel slot -> *d_image; the slot's read event (the slot is free once that has run).
template <class F> int upload_image(const char *who, StageRings &rings, int32_t device, hipStream_t stream, void *workspace, size_t image_bytes,
                                    const char *capture_refusal, F fill, char **d_image) {
  if (capture_refusal && stream_is_capturing(stream)) return fail(FCP_ERR_UNSUPPORTED, std::string(who) + ": " + capture_refusal);
  *d_image = reinterpret_cast<char *>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  StageRings::Lease sl;
  int rc = rings.acquire(device, image_bytes, &sl);
  if (rc) return rc;
  fill(sl.buf);
  __atomic_thread_fence(__ATOMIC_SEQ_CST); // the image is in memory before the launch that reads it is queued
  const int e = fcp_launch_upload(sl.buf_dev, *d_image, image_bytes, stream);
  if (e) return hip_fail((std::string(who) + ": descriptor upload launch").c_str(), (hipError_t)e);
  return sl.record(stream);
}

// ---- functions that cross translation units -----------------------------------------------------------------------
// fcp_plan.hip
// bytes of one descriptor slot: the FcpColDyn records and, in plans with weighted columns, the weights' offsets behind them
inline size_t slot_dyn_bytes(const fcp_plan *p) {
  return p->cols.size() * sizeof(FcpColDyn) + (p->has_weights ? p->cols.size() * sizeof(int64_t) : 0) +
         (p->plain_dense ? p->plain_tmpl.size() : 0);
}
// plain dense plans (never weighted): the span image of a descriptor slot, behind its records (48-byte records: 16-byte aligned)
inline size_t slot_image_off(const fcp_plan *p) { return p->cols.size() * sizeof(FcpColDyn); }
inline const int64_t *slot_weights(const fcp_plan *p, const FcpColDyn *dyn) {
  return p->has_weights ? reinterpret_cast<const int64_t *>(dyn + p->cols.size()) : nullptr;
}
void build_plain_template(fcp_plan *p); // the gate and the image template of plain dense plans (plan creation)
// fcp_process.hip (and stream_is_capturing, above)
int bind_tables(fcp_plan *p, const void *const *input_ptrs, bool capturing);
void build_key(const fcp_plan *p, const fcp_process_args_t *a, std::vector<int32_t> &key);
int find_or_reserve(fcp_plan *p, const std::vector<int32_t> &key, DynSlot **out, bool *install, bool capturing);
int install_slot(fcp_plan *p, const fcp_process_args_t *a, DynSlot &s);
void publish_slot(fcp_plan *p, DynSlot &s, const std::vector<int32_t> &key, void *stream);
void fill_launch(const fcp_plan *p, const DynSlot &s, int kind, const void *blob, void *arena, int store_policy, FcpLaunch *L);
// fcp_lanes.hip
void destroy_lanes(LanePool *pool);
int create_lanes(LanePool *pool, int n, int prio);
int process_on_private_streams(fcp_plan_t *p, const fcp_process_args_t *a, fcp_process_result_t *r);

struct SlotUnpin { // every exit path of a request: publish what `done` covers and give the slot back
  fcp_plan *p;
  DynSlot *s;
  bool recorded;
  ~SlotUnpin() {
    std::lock_guard<std::mutex> lock(p->mu);
    if (recorded) s->done_valid = s->uses == 1; // hits that joined meanwhile are not covered by `done`
    --s->users;
  }
};

} // namespace fcph

// the request on the stream it names (fcp_process.hip; also called by fcp_shard.hip)
extern "C" int fcp_internal_process(fcp_plan_t *p, const fcp_process_args_t *a, fcp_process_result_t *r);
