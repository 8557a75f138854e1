// api.inc -- extern "C" entry points of librayca_hip.so (declared in include/rayca_hip.h).
// Included at the end of kernels.hip so that the kernels' anonymous namespace is visible.  Here: the owners of device resources
// (DeviceBuffer, FrameCtx, and the types of the several-devices frame that RaycaScene holds), the one way a context's buffer is
// sized (ensure, grow_behind_pass), the pass protocol (ContextPass), the frame driver and the single-device entry points.  The
// kernels the entry points launch themselves are in aux_kernels.inc, kernel selection in select.inc, a scene's lifetime (create,
// destroy, finish, info, update, read-backs) in scene.inc, the several-devices frame (rayca_hip_render_multi and its issue /
// wait forms) in multi.inc, the image-space post passes in post.inc.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "refill.hpp"
#include "staging.hpp"

using namespace rayca;

namespace {

thread_local std::string g_last_error;

int32_t fail(int32_t code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                                         \
  do {                                                                                                        \
    hipError_t e__ = (expr);                                                                                  \
    if (e__ != hipSuccess)                                                                                    \
      return fail(e__ == hipErrorOutOfMemory ? RAYCA_ERR_OOM : RAYCA_ERR_HIP,                                 \
                  std::string(#expr) + ": " + hipGetErrorString(e__));                                        \
  } while (0)

// A device allocation and its owner.  ensure() (and grow_behind_pass on top of it) is the one way to size it; release() frees it
// early, the destructor with its owner.  Move-only and not assignable: a buffer is emptied by release(), never by writing an
// empty one over it.
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
};

}  // namespace

// Everything one frame in flight owns: work counters, statistics, per-depth path records, ray queues, the
// traversal stack's spill area, events.  A scene has kMaxContexts (8) of them (RaycaRenderOptions.context), created
// on first use, so that several frames of the same scene can be in flight on different streams: the tail of one
// frame (a few slow waves) then overlaps the head of the next (measured on the atrium, 1080p depth-1:
// 0.63 -> 0.48 ms per frame with two frames in flight).
// The context owns all of it and gives it back in one place, release(); the stream alone may leave before that (scene_destroy_now
// hands an idle stream to the StreamSetPool and clears the pointer).
constexpr uint32_t kMaxContexts = 8;
struct FrameCtx {
  bool ready = false;
  hipStream_t stream = nullptr;
  uint32_t* heads_alloc = nullptr;    // [second counter set][first counter set][2 queue counters]
  uint32_t* heads = nullptr;          // first set: 8 work counters on their own lines, then the 2 queue counters
  uint32_t* heads_b = nullptr;        // second set (wavefront engine: the shadow pass of the same generation)
  TraceCounters* counters = nullptr;
  unsigned long long* shade_stats = nullptr;  // [64 lines][16]: shaded / shadow / bounce counts of k_wf_shade
  DeviceBuffer path_direct, path_brdf, path_state, accum, queue[2], out8, out32, ray_io, stack_spill, frames, mis_samples, wf_hits, wf_sh_ray, wf_sh_x;
  DeviceBuffer denoise[2];            // rayca_hip_denoise_device: the two images its iterations go back and forth between
  DeviceBuffer denoise_var[2];        // rayca_hip_denoise_variance_device: the two variance planes that go with them (4 B a pixel)
  DeviceBuffer ambient_mask;          // rayca_hip_ambient_device without mask_out: the mask words its trace kernel ORs into (8 B a point); rayca_hip_direct_device's likewise
  DeviceBuffer probe_mask;            // rayca_hip_probe_lookup_device with visibility and without mask_out: the same, 4 B a point
  DeviceBuffer plan_weight;           // rayca_hip_sample_plan_device without weight_out: the weights its offsets kernel reads back (4 B a pixel)
  DeviceBuffer plan_sums;             // ... and the sums of its 64-pixel row segments, their prefix sums once scanned (4 B a segment); rayca_hip_surface_cdf_device: its first word is the largest area's bits
  DeviceBuffer gather_samples;        // rayca_hip_gather_device without samples_out: the radiance records of one internal frame (16 B a ray)
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  // Which of the context's counters are known to be zero, a bit each: the first work-counter set, the second, the two queue
  // counters.  A launch that draws from one clears its bit; k_resolve zeroes all three behind a frame, and a fused k_generation
  // launch the set it does not draw from (GenArgs.clear), so that the next frame finds what it needs clean and issues no memset.
  enum : uint32_t { kCleanHeads = 1u, kCleanHeadsB = 2u, kCleanQueues = 4u, kCleanAll = 7u };
  uint32_t heads_clean = 0u;
  hipEvent_t ev_done = nullptr;       // recorded behind the last kernel of every frame of this context
  bool frame_pending = false;         // ev_done has been recorded at least once
  std::vector<hipEvent_t> ev_trace;   // pairs around the timed launches of a frame (LaunchLog)
  std::mutex mu;
  // Everything back to the device, the stream included if it is still here.  The caller has waited for the context's last pass
  // and made its device current.  (A buffer this list forgets is not leaked: its own destructor frees it, with the context.)
  void release() {
    for (DeviceBuffer* b : {&path_direct, &path_brdf, &path_state, &accum, &queue[0], &queue[1], &out8, &out32, &ray_io, &stack_spill, &frames, &mis_samples,
                            &wf_hits, &wf_sh_ray, &wf_sh_x, &denoise[0], &denoise[1], &denoise_var[0], &denoise_var[1], &ambient_mask, &plan_weight, &plan_sums, &gather_samples, &probe_mask})
      b->release();
    if (heads_alloc) (void)hipFree(heads_alloc);
    if (counters) (void)hipFree(counters);
    heads_alloc = heads = heads_b = nullptr;
    counters = nullptr;
    shade_stats = nullptr;
    for (hipEvent_t* e : {&ev_begin, &ev_end, &ev_done}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
    for (hipEvent_t e : ev_trace) (void)hipEventDestroy(e);
    ev_trace.clear();
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    ready = frame_pending = false;
    heads_clean = 0u;
  }
  ~FrameCtx() { release(); }
};

// One host thread per part of rayca_hip_render_multi beyond the first: it issues that part's launches (a frame is 3-20
// launches and a hipSetDevice; eight parts one after the other on the caller's thread would cost more host time than a
// rank's share of a 1080p frame takes on its GPU).  The threads stay with the scene that assembles the frames.
struct PartWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, busy = false, quit = false;
  PartWorker() { th = std::thread([this] { loop(); }); }
  ~PartWorker() {
    {
      std::lock_guard<std::mutex> lock(mu);
      quit = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
  void post(std::function<void()> j) {
    {
      std::lock_guard<std::mutex> lock(mu);
      job = std::move(j);
      has_job = true;
      busy = true;
    }
    cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lock(mu);
    cv.wait(lock, [this] { return !busy; });
  }
  void loop() {
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      cv.wait(lock, [this] { return has_job || quit; });
      if (quit) return;
      std::function<void()> j = std::move(job);
      has_job = false;
      lock.unlock();
      j();
      lock.lock();
      busy = false;
      cv.notify_all();
    }
  }
};

// State of rayca_hip_render_multi (multi.inc), kept by the scene that assembles the frame (scenes[0]): per frame context the events
// and buffers of the frame in flight on it, and for the set of devices the communicators and issue threads.  All of it is made
// for one set of devices and given back by MultiCtx::release: when another set is adopted, and with the scene.
struct MultiFrame {
  std::vector<hipEvent_t> done;      // per part: its rows are rendered
  hipEvent_t gathered = nullptr;     // scenes[0]'s device: exchange, de-interleave and copy-out of this context's last frame are done
  bool gathered_valid = false;
  DeviceBuffer gather, frame;        // [part][max_rows][W][4] and [H][W][4] on scenes[0]'s device
  bool pending = false;              // a frame has been issued and not waited for
  bool rccl = false;                 // ... with the RCCL transport (its senders' streams are drained by the wait too)
  void release(const std::vector<int>& devices);   // (done[i] is an event of devices[i])
};
struct MultiCtx {
  std::vector<int> devices;          // device of every part, in part order
  std::vector<void*> comms;          // ncclComm_t per part (RCCL transport), created for exactly `devices`
  MultiFrame frames[kMaxContexts];
  std::vector<std::unique_ptr<PartWorker>> workers;   // parts 1..n-1
  bool peer_enabled = false;
  void release();   // the caller has waited for the frames in flight (MultiFrame::gathered)
  ~MultiCtx() { release(); }
};

struct RaycaScene {
  int device = 0;
  RaycaSceneDesc counts{};   // the creation descriptor with its pointers cleared: the counts rayca_hip_scene_update holds to
  HostScene host;
  DevScene dev{};
  std::vector<void*> allocations;
  uint64_t device_bytes = 0;
  float build_ms = 0.0f, runtime_init_ms = 0.0f;
  int cu_count = 0;
  FrameCtx ctx[kMaxContexts];
  // Which node format -- binary or 4-wide, f32 or fp16 boxes?  It depends on scene, ray coherence and kernel
  // (measured with two frames in flight: soup Flat 12.9 ms on f32 nodes, 10.4 ms on fp16; atrium depth-1 frame
  // 0.481 vs 0.523 ms the other way round; atrium Flat binary-fp16 0.205, wide-f32 0.234), and all four give the
  // same bits, so the first sixteen large frames of each (mode, generation class) are rendered with each format in
  // turn, four times, and timed (the best of the four counts; with two, one bench run in a dozen settled on the slower).
  struct Tune {
    int decided = -1;      // -1: still measuring, else the format: bit 0 = 4-wide, bit 1 = fp16
    uint32_t launched = 0; // calibration frames handed out (frame i is rendered with format i & 3)
    uint32_t booked = 0;   // calibration frames whose time has been booked -- under the format they were LAUNCHED with
    float best[4] = {1e30f, 1e30f, 1e30f, 1e30f};
    // Flat camera rays, once the format is decided: k_generation or the lane-refill kernel (refill.hip)?  Eight more
    // frames, alternating, the best of four each (four were not enough: one slow frame decided it the wrong way in one
    // bench run out of a dozen); same bits either way.
    int refill = -1;       // -1: not decided, 0: k_generation, 1: k_flat_refill
    uint32_t refill_launched = 0, refill_booked = 0;
    float refill_best[2] = {1e30f, 1e30f};
  } tune[2][2];            // [Flat, Path][generation 0, bounce generations]
  // scene_create returns with the binary f32 nodes on the device; the other three formats (4-wide, and both with fp16 boxes:
  // host_scene.cpp finish_node_formats) are made and uploaded by `formats_thread` while the first frames already run.  `dev` is
  // never written after scene_create; `dev_full` = `dev` + the other formats is complete before formats_state becomes 1.
  DevScene dev_full{};
  std::thread formats_thread;
  std::mutex formats_mu;               // join
  std::atomic<int> formats_state{1};   // 0: being made, 1: there (or none to make), -1: failed (formats_rc, formats_err)
  std::atomic<bool> formats_cancel{false};   // rayca_hip_scene_destroy: the thread stops at its next phase boundary
  int32_t formats_rc = RAYCA_OK;
  std::string formats_err;
  std::vector<void*> formats_allocations;
  uint64_t formats_bytes = 0;
  float formats_ms = 0.0f;
  uint32_t node_count = 0, prim_count = 0;   // (the host arrays they count are released once everything is on the device)
  // the frame contexts of the last four asynchronous render calls (context + 1, a byte each): how many frames the host
  // keeps in flight, which sizes the persistent grids (frames_in_flight_hint)
  std::atomic<uint32_t> recent_contexts{0};
  std::mutex streams_mu;               // make_scene_streams
  hipStream_t build_streams[2] = {nullptr, nullptr};   // the device builder's (two trees side by side)
  std::atomic<int> build_streams_ready{0};              // make_scene_streams has made (or failed to make) those two
  int streams_made = 0;                // 0: none, 1: the builders' two, 2: the frame contexts' too
  std::thread ctx_thread;              // sets frame context 0 up behind scene_create (joined by scene_destroy)
  MultiCtx multi;
  std::mutex multi_mu;
  std::mutex tune_mu;      // guards every read and write of tune[][] (frames of different contexts run on different threads)
  // RAYCA_NEE_SKIP=0, read when the scene is created, turns off the skipping of NEE samples that cannot contribute
  // (trace_core.inc nee_irrelevant): for A/B measurements and the tests that compare frames with and without it.  Same bits.
  bool nee_skip = true;
};

namespace {

template <typename T>
int32_t upload(RaycaScene* s, const T* src, size_t count, const T** dst) {
  const size_t bytes = sizeof(T) * (count ? count : 1);
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  s->allocations.push_back(p);
  s->device_bytes += bytes;
  if (count) {  // (the null stream, like the hipMemcpy this was; large arrays through page-locked blocks: staging.hpp)
    StagedCopier staged;
    HIP_TRY(staged.copy(p, src, sizeof(T) * count, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  *dst = static_cast<const T*>(p);
  return RAYCA_OK;
}

// How many frames the host has in flight, as far as the last four calls tell: the number of different frame contexts among
// them when the caller passes its own stream (a call without one waits for its frame: nothing overlaps it).  Only ever
// changes how the work of a frame is spread over the chip, never a pixel.
uint32_t frames_in_flight_hint(RaycaScene* s, uint32_t context, bool asynchronous) {
  if (!asynchronous) {
    s->recent_contexts.store(0u, std::memory_order_relaxed);
    return 1u;
  }
  uint32_t r = s->recent_contexts.load(std::memory_order_relaxed);
  r = (r << 8) | (context + 1u);
  s->recent_contexts.store(r, std::memory_order_relaxed);
  uint32_t seen = 0, n = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t id = (r >> (8 * i)) & 255u;
    if (id != 0u && !(seen & (1u << id))) {
      seen |= 1u << id;
      ++n;
    }
  }
  return n ? n : 1u;
}

// The other node formats: there yet?  (acquire: pairs with the release store of the thread that made them)
bool formats_ready(const RaycaScene* s) { return s->formats_state.load(std::memory_order_acquire) == 1; }
// Wait for them (engines and requests that are tied to one of those formats).
int32_t formats_wait(RaycaScene* s) {
  {
    std::lock_guard<std::mutex> lock(s->formats_mu);
    if (s->formats_thread.joinable()) s->formats_thread.join();
  }
  if (s->formats_state.load(std::memory_order_acquire) == 1) return RAYCA_OK;
  return fail(s->formats_rc, s->formats_err);
}

int32_t ensure(DeviceBuffer& b, size_t bytes) {
  if (b.bytes >= bytes && b.ptr) return RAYCA_OK;
  b.release();
  HIP_TRY(hipMalloc(&b.ptr, bytes));
  b.bytes = bytes;
  return RAYCA_OK;
}
// The growth rule: a buffer of a frame context at `bytes` or more.  An earlier pass of the context that has not been waited for
// may still be working in the buffer to be replaced -- on another stream -- so regrowing waits for the context's ev_done first.
// Every buffer of a FrameCtx is sized through here; plain ensure is for buffers no context pass uses.  A call that does not
// regrow costs the one comparison.  (The context's mutex is held and its device current.)
int32_t grow_behind_pass(FrameCtx* c, DeviceBuffer& b, size_t bytes) {
  if (b.bytes < bytes && c->frame_pending) HIP_TRY(hipEventSynchronize(c->ev_done));
  return ensure(b, bytes);
}

// The streams of all frame contexts of a scene, made in one go.  HIP runs a process's streams over four hardware queues per
// device and ties a stream to one of them when it is created: the queue with the fewest streams at that moment.  Frames in
// flight only overlap if their streams sit on different queues -- a rank's eighth of a 1080p frame takes 0.073 ms per frame
// with four of them in flight on four queues and 0.12-0.16 ms when two share one (tests/gpu_rank_share_probe.py,
// profiles/r02_queue_log.txt) -- and streams made one by one, whenever a context is first used, land wherever the other
// streams of the process (the scene builder's, RCCL's, the host's) left the counts at that moment.  Streams made back to
// back level the queues out first and then go round them in turn: twelve throw-away streams to do the levelling, then the
// contexts' streams, consecutive contexts on consecutive queues.
// The two streams the device builder builds a scene's two trees on are made in the same run, for the same reason: on one
// queue the two builds run one after the other (a level of one waits for a level of the other) instead of side by side.
// A scene's streams -- two for the builders, one per frame context -- outlive it: a destroyed scene hands the set (idle:
// scene_destroy_now has waited for everything on them) to the next scene on the same device.  Creating the 22 streams below
// takes ~10 ms, which a host that rebuilds the scene per draw() had on the critical path of every scene_create once the
// flatten became shorter than that; the streams keep the hardware queues they were created on, so the balance the ballast
// bought is kept too.  At most kStreamSetsKept sets per device wait here.
struct StreamSet {
  hipStream_t build[2] = {};
  hipStream_t ctx[kMaxContexts] = {};
};
constexpr size_t kStreamSetsKept = 4;
struct StreamSetPool {
  std::mutex mu;
  std::unordered_map<int, std::vector<StreamSet>> sets;   // by device
};
StreamSetPool& stream_set_pool() {
  static StreamSetPool* p = new StreamSetPool();   // (never destroyed: a scene may be released at process exit)
  return *p;
}
// all = false: the builders' two only (what scene_create waits for) -- unless a whole set waits in the pool.  The frame
// contexts' streams are made by the first ensure_ctx: the upload thread's, once the primitives are on the device -- by then the
// builders have made their allocations, which a run of twenty stream creations beside them stretched from 1 to 13 ms in a
// process's first scene_create.
void make_scene_streams(RaycaScene* s, bool all) {
  std::lock_guard<std::mutex> lock(s->streams_mu);
  if (s->streams_made == 2 || (s->streams_made == 1 && !all)) return;
  if (s->streams_made == 0) {
    StreamSetPool& pool = stream_set_pool();
    std::lock_guard<std::mutex> plock(pool.mu);
    std::vector<StreamSet>& kept = pool.sets[s->device];
    if (!kept.empty()) {
      const StreamSet set = kept.back();
      kept.pop_back();
      for (int i = 0; i < 2; ++i) s->build_streams[i] = set.build[i];
      for (uint32_t i = 0; i < kMaxContexts; ++i)
        if (!s->ctx[i].stream) s->ctx[i].stream = set.ctx[i];
        else if (set.ctx[i]) (void)hipStreamDestroy(set.ctx[i]);
      s->streams_made = 2;
      s->build_streams_ready.store(1, std::memory_order_release);
      return;
    }
  }
  if (s->streams_made == 0) {
    for (hipStream_t& b : s->build_streams)
      if (hipStreamCreateWithFlags(&b, hipStreamNonBlocking) != hipSuccess) b = nullptr;  // (the builder then makes its own)
    s->streams_made = 1;
    s->build_streams_ready.store(1, std::memory_order_release);
  }
  if (!all) return;
  s->streams_made = 2;
  hipStream_t ballast[12] = {};
  for (hipStream_t& b : ballast)
    if (hipStreamCreateWithFlags(&b, hipStreamNonBlocking) != hipSuccess) b = nullptr;
  for (FrameCtx& c : s->ctx)
    if (!c.stream && hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) c.stream = nullptr;  // (ensure_ctx tries again)
  for (hipStream_t b : ballast)
    if (b) (void)hipStreamDestroy(b);
  (void)hipGetLastError();
}

// one allocation: TraceCounters, then (128-B aligned) the 64 statistics lines of k_wf_shade
constexpr size_t kShadeStatsOffset = ((sizeof(TraceCounters) + 127) / 128) * 128;
constexpr size_t kCountersBytes = kShadeStatsOffset + 64 * 16 * sizeof(unsigned long long);

// first use of a frame context: stream, counters, events
int32_t ensure_ctx(RaycaScene* s, FrameCtx* c) {
  if (c->ready) return RAYCA_OK;
  HIP_TRY(hipSetDevice(s->device));
  make_scene_streams(s, true);
  if (!c->stream) HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (!c->ev_begin) HIP_TRY(hipEventCreate(&c->ev_begin));
  if (!c->ev_end) HIP_TRY(hipEventCreate(&c->ev_end));
  if (!c->ev_done) HIP_TRY(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  if (!c->heads_alloc) {
    void* heads = nullptr;
    HIP_TRY(hipMalloc(&heads, (16 * 64 + 64) * sizeof(uint32_t)));
    c->heads_alloc = static_cast<uint32_t*>(heads);
    c->heads_b = c->heads_alloc;
    c->heads = c->heads_alloc + 8 * 64;
    HIP_TRY(hipMemset(c->heads_alloc, 0, (16 * 64 + 64) * sizeof(uint32_t)));
  }
  if (!c->counters) {
    void* ctr = nullptr;
    HIP_TRY(hipMalloc(&ctr, kCountersBytes));
    c->counters = static_cast<TraceCounters*>(ctr);
    c->shade_stats = reinterpret_cast<unsigned long long*>(static_cast<char*>(ctr) + kShadeStatsOffset);
    HIP_TRY(hipMemset(c->counters, 0, kCountersBytes));
  }
  // hipMemset of device memory is asynchronous (null stream) and the frame streams are non-blocking: without this
  // the zeroing could land in the middle of the first kernel and hand out batches twice
  HIP_TRY(hipStreamSynchronize(nullptr));
  c->ready = true;
  return RAYCA_OK;
}

uint32_t tile_rows(const RaycaTile& t, uint32_t height) {
  if (t.parts <= 1) return height;
  const uint32_t band = t.band_rows ? t.band_rows : 1;
  uint32_t n = 0;
  for (uint32_t y = 0; y < height; ++y)
    if ((y / band) % t.parts == t.part) ++n;
  return n;
}

// light/quad.rs:40-46 (sin_theta = 1 - cos_theta, as written in the reference)
float quad_area(F4 ab, F4 ac) {
  const float ab_len = length(ab), ac_len = length(ac);
  const float cos_theta = dot(ab, ac) / (ab_len * ac_len);
  const float sin_theta = 1.0f - cos_theta;
  return sin_theta * ab_len * ac_len;
}

bool is_emissive(const RaycaMaterial& m) {  // phong.rs:54-56, Color::close color/mod.rs:160-169
  if (m.kind != RAYCA_MATERIAL_PHONG) return false;
  const bool close_to_black = fabsf(m.emission[0] - 0.0f) < FLT_EPSILON && fabsf(m.emission[1] - 0.0f) < FLT_EPSILON &&
                              fabsf(m.emission[2] - 0.0f) < FLT_EPSILON && fabsf(m.emission[3] - 1.0f) < FLT_EPSILON;
  return !close_to_black;
}

// The device records of a material and a light (scene_create and rayca_hip_scene_update: the same bits).  Zero-filled
// first, so that two records compare equal with memcmp exactly when the kernels read the same values.
DevMaterial dev_material(const RaycaMaterial& m) {
  DevMaterial d;
  std::memset(&d, 0, sizeof d);
  std::memcpy(d.color, m.color, 16); std::memcpy(d.ambient, m.ambient, 16); std::memcpy(d.emission, m.emission, 16);
  std::memcpy(d.diffuse, m.diffuse, 16); std::memcpy(d.specular, m.specular, 16);
  d.kind = m.kind; d.albedo_texture = m.albedo_texture; d.normal_texture = m.normal_texture;
  d.metallic_roughness_texture = m.metallic_roughness_texture;
  d.metallic_factor = m.metallic_factor; d.roughness_factor = m.roughness_factor; d.shininess = m.shininess;
  d.emissive = is_emissive(m) ? 1u : 0u;
  return d;
}

DevLight dev_light(const HostLight& l) {
  DevLight d;
  std::memset(&d, 0, sizeof d);
  d.kind = l.kind; d.material = l.material; d.intensity = l.intensity;
  d.color[0] = l.color.r; d.color[1] = l.color.g; d.color[2] = l.color.b; d.color[3] = l.color.a;
  d.attenuation[0] = l.attenuation.x; d.attenuation[1] = l.attenuation.y; d.attenuation[2] = l.attenuation.z;
  d.ab[0] = l.ab.x; d.ab[1] = l.ab.y; d.ab[2] = l.ab.z;
  d.ac[0] = l.ac.x; d.ac[1] = l.ac.y; d.ac[2] = l.ac.z;
  const F4 pos = to_point(trs_world_translation(l.local));  // Point3::from(light_node.trs.get_translation())
  d.position[0] = pos.x; d.position[1] = pos.y; d.position[2] = pos.z; d.position[3] = pos.w;
  const F4 dir = -rotate(vec3(1.0f, 0.0f, 0.0f), l.local.rotation);  // DirectionalLight::get_direction  directional.rs:47-51
  d.direction[0] = dir.x; d.direction[1] = dir.y; d.direction[2] = dir.z;
  d.trs_translation[0] = l.local.translation.x; d.trs_translation[1] = l.local.translation.y; d.trs_translation[2] = l.local.translation.z;
  d.trs_rotation[0] = l.local.rotation.x; d.trs_rotation[1] = l.local.rotation.y; d.trs_rotation[2] = l.local.rotation.z; d.trs_rotation[3] = l.local.rotation.w;
  d.trs_scale[0] = l.local.scale.x; d.trs_scale[1] = l.local.scale.y; d.trs_scale[2] = l.local.scale.z;
  if (l.kind == RAYCA_LIGHT_QUAD) {
    const F4 n = normalized(cross(l.ab, l.ac));
    d.normal[0] = n.x; d.normal[1] = n.y; d.normal[2] = n.z;
    d.area = quad_area(l.ab, l.ac);
  }
  return d;
}

#include "select.inc"   // how a launch gets its kernel and its plan

// ---- one frame: the frame driver (frame_run) drives the per-engine launch steps below --------------------------------

// The launches of one frame: how many, and the event pairs around the timed ones (the i-th timed launch, of class
// ev_class[i], sits between events 2i and 2i + 1 of the context's ev_trace, which are made on first use and kept).
struct LaunchLog {
  FrameCtx* c = nullptr;
  size_t ev_used = 0;
  std::vector<int> ev_class;   // kernel class (RAYCA_KERNEL_*) per event pair
  uint32_t launches = 0, trace_launches = 0;
};
// One launch: `launch()` issues it and returns RAYCA_OK or an error.  `timed`: bracketed by an event pair of kernel class
// `cls`, whose index in ev_trace (of its first event) goes to *pair.  `trace`: it counts as a traversal launch.
template <typename Launch>
int32_t timed_launch(LaunchLog& log, hipStream_t stream, int cls, bool timed, bool trace, Launch&& launch, size_t* pair = nullptr) {
  std::vector<hipEvent_t>& ev = log.c->ev_trace;
  if (timed) {
    for (hipEvent_t e; ev.size() < log.ev_used + 2;) {
      HIP_TRY(hipEventCreate(&e));
      ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(ev[log.ev_used], stream));
    log.ev_class.push_back(cls);
    if (pair) *pair = log.ev_used;
    log.ev_used += 2;
  }
  const int32_t rc = launch();
  if (rc != RAYCA_OK) return rc;
  HIP_TRY(hipGetLastError());
  if (timed) HIP_TRY(hipEventRecord(ev[log.ev_used - 1], stream));
  ++log.launches;
  if (trace) ++log.trace_launches;
  return RAYCA_OK;
}

// ---- one pass on a frame context: what a frame, a query and every post pass do around their launches ------------------------
// The ownership rule.  A pass holds its context's mutex and runs on the caller's stream (opts.stream) or the context's own.
// It starts behind the context's previous pass ON THE DEVICE -- that one may still be running on another stream and owns the
// same work buffers -- and behind opts.wait_event; it leaves the context's ev_done (and opts.record_event) behind its last
// launch.  ev_done is what rayca_hip_scene_update, scene_destroy and every regrowth of a buffer that a pass in flight may
// use wait for, before they overwrite or free it.  The regrowth is spelled once: grow_behind_pass, through which every buffer of
// a FrameCtx is sized -- by a pass for itself, and by the calls that stage through a context's buffers (rayca_hip_render, the
// parts of the several-devices frame).  The context's own stream is not the caller's to wait on, so a pass on it is synchronous;
// so is a pass that reports statistics.
//   pass_acquire ... [buffers, memsets] ... ev_begin when timing ... launches ... pass_retire ... pass_finish
// ev_begin is where kernel_ms starts: behind whatever the pass clears or prepares first, so every entry records it itself.
struct ContextPass {
  FrameCtx* c;
  hipStream_t stream;
  void* record_event;
  bool timing;       // RaycaStats asked for: ev_begin / ev_end bracket the launches
  bool own_stream;   // the context's stream, not the caller's
};
int32_t pass_acquire(RaycaScene* s, const RaycaRenderOptions& o, bool timing, ContextPass& p) {   // (o.context is in range, its mutex held)
  FrameCtx* c = &s->ctx[o.context];
  HIP_TRY(hipSetDevice(s->device));
  const int32_t rc = ensure_ctx(s, c);
  if (rc != RAYCA_OK) return rc;
  p = ContextPass{c, o.stream ? static_cast<hipStream_t>(o.stream) : c->stream, o.record_event, timing, o.stream == nullptr};
  if (c->frame_pending) HIP_TRY(hipStreamWaitEvent(p.stream, c->ev_done, 0));
  if (o.wait_event) HIP_TRY(hipStreamWaitEvent(p.stream, static_cast<hipEvent_t>(o.wait_event), 0));
  return RAYCA_OK;
}
int32_t pass_retire(const ContextPass& p) {
  if (p.timing) HIP_TRY(hipEventRecord(p.c->ev_end, p.stream));
  HIP_TRY(hipEventRecord(p.c->ev_done, p.stream));
  if (p.record_event) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(p.record_event), p.stream));
  p.c->frame_pending = true;
  return RAYCA_OK;
}
// The synchronisation the rule asks for and, with stats_out (given iff p.timing), the statistics every pass but a frame fills
// alike: everything zero but the time from ev_begin to pass_retire and its `launches`, under RAYCA_KERNEL_OTHER.
int32_t pass_finish(const ContextPass& p, uint32_t launches, RaycaStats* stats_out) {
  if (p.own_stream || stats_out) HIP_TRY(hipStreamSynchronize(p.stream));
  if (!stats_out) return RAYCA_OK;
  std::memset(stats_out, 0, sizeof *stats_out);
  HIP_TRY(hipEventElapsedTime(&stats_out->kernel_ms, p.c->ev_begin, p.c->ev_end));
  stats_out->kernel_launches = launches;
  stats_out->class_ms[RAYCA_KERNEL_OTHER] = stats_out->kernel_ms;
  stats_out->class_launches[RAYCA_KERNEL_OTHER] = launches;
  return RAYCA_OK;
}

// One pass whose launches need nothing of the context but its stream, shaped like timed_launch: the context's lock,
// `prepare(c)` under it (buffers of the context that must exist before the pass queues its waits), pass_acquire, ev_begin when
// timing, `body(stream, launches)`, pass_retire, pass_finish.  The body enqueues on `stream`, checks hipGetLastError behind
// each launch and counts what it launched.  (o.context is in range: pass_options has seen `o`.)  A `prepare` that finds nothing to
// do -- what it reads of the scene it reads under the lock -- returns kPassNothing: the call is RAYCA_OK without a pass.
constexpr int32_t kPassNothing = 1;   // (errors are negative)
template <typename Prepare, typename Body>
int32_t run_pass(RaycaScene* s, const RaycaRenderOptions& o, RaycaStats* stats_out, Prepare&& prepare, Body&& body) {
  FrameCtx* c = &s->ctx[o.context];
  std::lock_guard<std::mutex> lock(c->mu);
  int32_t rc = prepare(c);
  if (rc != RAYCA_OK) return rc == kPassNothing ? RAYCA_OK : rc;
  ContextPass pass{};
  if ((rc = pass_acquire(s, o, stats_out != nullptr, pass)) != RAYCA_OK) return rc;
  if (pass.timing) HIP_TRY(hipEventRecord(c->ev_begin, pass.stream));
  uint32_t launches = 0;
  if ((rc = body(pass.stream, launches)) != RAYCA_OK) return rc;
  if ((rc = pass_retire(pass)) != RAYCA_OK) return rc;
  return pass_finish(pass, launches, stats_out);
}
template <typename Body>
int32_t run_pass(RaycaScene* s, const RaycaRenderOptions& o, RaycaStats* stats_out, Body&& body) {
  return run_pass(s, o, stats_out, [](FrameCtx*) -> int32_t { return RAYCA_OK; }, body);
}

// What a device pass other than a frame takes of RaycaRenderOptions: stream, context and the two events always, and the
// groups of fields in `accepts`; every other field must be zero.  `what` names the call in the message.
enum : uint32_t { kOptTraversal = 1u, kOptCollectStats = 2u, kOptTile = 4u };
int32_t pass_options(const RaycaRenderOptions& o, const char* what, uint32_t accepts) {
  if (o.context >= kMaxContexts) return fail(RAYCA_ERR_BAD_ARG, "context out of range");
  if ((accepts & kOptTraversal) && o.traversal > RAYCA_TRAVERSAL_EXHAUSTIVE) return fail(RAYCA_ERR_BAD_ARG, "unknown traversal");
  const char* field = nullptr;
  if (!(accepts & kOptTraversal) && o.traversal != 0) field = "traversal";
  else if (!(accepts & kOptCollectStats) && o.collect_stats != 0) field = "collect_stats";
  else if (o.engine != 0) field = "engine";
  else if (o.camera_rays != 0) field = "camera_rays";
  else if (o.reserved != 0) field = "reserved";
  else if (!(accepts & kOptTile) && (o.tile.part != 0 || o.tile.parts != 0 || o.tile.band_rows != 0 || o.tile.reserved != 0)) field = "tile";
  if (field) return fail(RAYCA_ERR_BAD_ARG, std::string("RaycaRenderOptions.") + field + " does not apply to " + what + ": must be zero");
  return RAYCA_OK;
}

// generation class, index of the event pair, the format launched; refill: -1 = a format calibration, 0/1 = a kernel calibration
struct TuneEvent { int cls; size_t ev; int format; int refill; };

// What feeds generation 0 of a frame whose rays are not the camera's: a ray array (rayca_hip_radiance_device, k_enqueue_rays) or the
// inputs the rays are made from (one internal frame of rayca_hip_gather_device, k_enqueue_gather).  Ray i of the feed is "pixel" i of
// the frame and draws from the stream of (cfg.seed, first_index + i, sample).
struct RayFeed {
  const float* rays;        // DEVICE: 6 f32 a ray, or nullptr:
  const GatherIo* gather;   // ... the points, normals and table of the frame (its first_index is the feed's)
  uint32_t first_index, sample;
};

// What the steps of one frame share.
struct Frame {
  RaycaScene* s;
  FrameCtx* c;
  RaycaConfig cfg;
  RaycaRenderOptions opts;
  LaunchPlan plan;
  FrameParams fp;
  PathBuffers pb;
  hipStream_t stream;
  const DevScene* dscene;           // s->dev_full once the other node formats are there, else s->dev
  uint8_t* rgba8;
  float4* rgba32f;
  const RayFeed* rays;              // rayca_hip_radiance_device, rayca_hip_gather_device: generation 0 reads this feed's rays from a queue, not the camera's (null for a frame)
  uint32_t in_flight;               // frames_in_flight_hint
  bool fused;                       // one generation, one sample: the generation kernel writes the pixel (no k_resolve)
  bool timing;                     // RaycaStats asked for: every launch timed
  bool all_formats;                 // formats_ready
  uint32_t node_format;             // RaycaStats.node_format
  int frame_format[2] = {-2, -2};   // node format of this frame per generation class (-2 = not asked yet, -1 = default)
  bool frame_calibrates[2] = {false, false};
  std::vector<TuneEvent> tune_events;   // calibration launches of this frame
  LaunchLog log;
};

// generation g reads queue (g - 1) & 1 and writes queue g & 1 (frame_run); their counters sit behind the 8 padded work counters
struct GenQueues {
  QueuedRay* in;
  uint32_t* in_count;
  QueuedRay* out;
  uint32_t* out_count;
};

// One generation of the wavefront engine: closest hits, shading, then shadow rays + direct lighting when there are any.
int32_t wavefront_generation(Frame& f, uint32_t g, const GenQueues& q) {
  RaycaScene* s = f.s;
  FrameCtx* c = f.c;
  const bool sph = s->host.sphere_count != 0, fast = s->dev.ref_leaf_of != nullptr, stats = f.plan.stats;
  const bool gen0 = g == 0 && !f.rays;   // camera rays; the caller's rays (rayca_hip_radiance_device) are a queue like any bounce generation's
  if (fast)   // (the formats these kernels are compiled for: RAYCA_WF_*, trace_core.inc)
    f.node_format |= gen0 ? ((RAYCA_WF_PRIMARY_WIDE ? 1u : 0u) | (RAYCA_WF_PRIMARY_HALF ? 4u : 0u)) : ((RAYCA_WF_BOUNCE_WIDE ? 2u : 0u) | (RAYCA_WF_BOUNCE_HALF ? 8u : 0u));
  // 16 LDS entries per lane (16 KiB per block) so that the lean kernels' occupancy is set by registers
  // (the wide tree never needs more pending entries than the binary one: one plan serves both)
  const StackPlan sp = plan_stack(std::max(s->host.max_depth, s->host.max_depth4), RAYCA_WF_LDS_ENTRIES);
  const Trav trav = !fast ? kTravExact : (sp.spill_entries ? kTravFastSpill : kTravFast);
  const uint32_t npix = f.pb.npix;
  const uint32_t batches = gen0 ? f.fp.tile_count : (npix + 63u) / 64u;
  const uint32_t grid = (batches + 3u) / 4u;  // one thread per ray, four 8x8 tiles per block
  const uint32_t nls = (f.plan.mode == kModePath && f.cfg.direct_sampler == RAYCA_SAMPLER_NEE) ? (uint32_t)s->host.lights.size() * f.cfg.light_samples : 0u;
  int32_t rc;
  WfBuffers wb{};
  if ((rc = grow_behind_pass(c, c->wf_hits, (size_t)npix * 16u)) != RAYCA_OK) return rc;
  wb.hits = static_cast<float4*>(c->wf_hits.ptr);
  wb.nls = nls;
  if (nls) {
    if ((rc = grow_behind_pass(c, c->wf_sh_ray, (size_t)npix * nls * 32u)) != RAYCA_OK) return rc;
    if ((rc = grow_behind_pass(c, c->wf_sh_x, (size_t)npix * nls * 16u)) != RAYCA_OK) return rc;
    wb.sh_ray = static_cast<float4*>(c->wf_sh_ray.ptr);
    wb.sh_x = static_cast<float4*>(c->wf_sh_x.ptr);
  }
  // On a SAH scene the bounce generations' closest hits run on persistent lanes that take the next queue entry when their
  // ray is done (refill.hip k_queue_refill; Knobs.wf_refill off keeps one ray per lane, k_wf_trace), and so do the shadow
  // rays (k_shadow_refill; Knobs.wf_shadow_refill: 0 never, 1 bounce generations, 2 every generation), on the second
  // set of work counters.  The work counters are cleared by frame_run, every generation.
  const bool wf_refill = knobs().wf_refill;
  const int shadow_refill_mode = knobs().wf_shadow_refill;
  TraceLaunch tl{};
  uint32_t lgrid = grid;
  // (a caller's rays on a SAH scene always: k_queue_refill has a form with the slack rays from anywhere need, k_wf_trace<false> has not)
  const bool caller_rays = f.rays && g == 0;
  bool refill = (wf_refill || caller_rays) && !gen0 && fast;
  if (refill && (rc = persistent_grid(s, queue_refill_kernel(sph, stats, caller_rays), sp.lds_bytes, batches, true, f.in_flight, 0u, lgrid)) != RAYCA_OK) return rc;
  if ((rc = bind_stack(c, sp, lgrid, tl)) != RAYCA_OK) return rc;
  if (refill) tl.ticket = 1u;
  WfTraceKernel kt = pick_wf_trace(gen0, trav, sph, stats);
  rc = timed_launch(f.log, f.stream, refill ? RAYCA_KERNEL_QUEUE_REFILL : RAYCA_KERNEL_WF_TRACE, f.timing, true, [&] {
    if (refill)
      launch_queue_refill(sph, stats, caller_rays, lgrid, sp.lds_bytes, f.stream, *f.dscene, q.in, q.in_count, wb.hits, c->heads, c->counters, tl);
    else
      hipLaunchKernelGGL(kt, dim3(lgrid), dim3(kBlock), sp.lds_bytes, f.stream, *f.dscene, f.fp, q.in, q.in_count, wb, c->counters, tl);
    return RAYCA_OK;
  });
  if (rc != RAYCA_OK) return rc;
  WfShadeKernel ks = pick_wf_shade(f.plan.mode, gen0, f.fused, sph, caller_rays);
  const uint32_t shade_grid = ((gen0 ? f.fp.tile_count * 64u : npix) + kShadeBlock - 1) / kShadeBlock;
  rc = timed_launch(f.log, f.stream, RAYCA_KERNEL_WF_SHADE, f.timing, false, [&] {
    hipLaunchKernelGGL(ks, dim3(shade_grid), dim3(kShadeBlock), 0, f.stream, *f.dscene, f.fp, q.in, q.in_count, q.out, q.out_count, wb, f.pb, g,
                       f.rgba8, f.rgba32f, c->shade_stats);
    return RAYCA_OK;
  });
  if (rc != RAYCA_OK || !nls) return rc;
  lgrid = grid;
  refill = wf_refill && fast && (!gen0 ? shadow_refill_mode >= 1 : shadow_refill_mode >= 2);
  if (refill && (rc = persistent_grid(s, shadow_refill_kernel(gen0, sph, stats), sp.lds_bytes, batches, true, f.in_flight, 0u, lgrid)) != RAYCA_OK) return rc;
  if ((rc = bind_stack(c, sp, lgrid, tl)) != RAYCA_OK) return rc;
  if (refill) tl.ticket = 1u;
  WfShadowKernel kh = pick_wf_shadow(gen0, trav, sph, stats);
  const ShadowRefillArgs sa{wb.sh_ray, wb.sh_x, wb.nls, f.pb.direct, f.pb.state, f.pb.npix};
  return timed_launch(f.log, f.stream, refill ? RAYCA_KERNEL_SHADOW_REFILL : RAYCA_KERNEL_WF_SHADOW, f.timing, true, [&] {
    if (refill)
      launch_shadow_refill(gen0, sph, stats, lgrid, sp.lds_bytes, f.stream, *f.dscene, f.fp, q.in, q.in_count, sa, g, c->heads_b, c->counters, tl);
    else
      hipLaunchKernelGGL(kh, dim3(lgrid), dim3(kBlock), sp.lds_bytes, f.stream, *f.dscene, f.fp, q.in, q.in_count, wb, f.pb, g, c->counters, tl);
    return RAYCA_OK;
  });
}

// What one generation of the fused engine launches (GenChoice, select.inc).
GenChoice choose_generation(Frame& f, uint32_t g) {
  RaycaScene* s = f.s;
  const LaunchPlan& plan = f.plan;
  RaycaScene::Tune& tu = s->tune[plan.mode == kModePath ? 1 : 0][g == 0 ? 0 : 1];
  GenChoice ch{f.all_formats ? format_forced() : 0, false, false, false};  // (binary f32 until the other formats are there)
  // Flat camera rays on a SAH scene: k_generation, or the lane-refill kernel (refill.hip)?  Decided per scene by timing
  // eight frames (Knobs.refill pins it) -- BEFORE the node format is timed, on 4-wide f32 nodes: the kernels differ
  // by far more than the formats do (soup: 6.2 against 11 ms), and the formats rank differently under the two (soup:
  // binary and 4-wide fp16 nodes tie under k_generation, 7.2 against 6.2 ms under lane refill), so the format has to be
  // timed on the kernel that will run it.
  const int refill_env = knobs().refill;
  const bool refill_possible = f.fused && plan.mode == kModeFlat && plan.ordered && s->dev.ref_leaf_of != nullptr;
  const int refill_forced = !refill_possible ? 0 : (f.opts.camera_rays == RAYCA_CAMERA_REFILL ? 1 : (f.opts.camera_rays == RAYCA_CAMERA_GENERATION ? 0 : refill_env));
  ch.refill = refill_forced > 0;
  bool kernel_pending = false;
  if (refill_possible && f.all_formats && refill_forced < 0) {   // (the timing runs on 4-wide nodes: once they are there)
    std::lock_guard<std::mutex> tune_lock(s->tune_mu);
    if (tu.refill >= 0) ch.refill = tu.refill != 0;
    else if (f.pb.npix >= 65536u && !plan.stats && tu.refill_launched < 8u) {
      ch.refill = (tu.refill_launched++ & 1u) != 0;
      ch.refill_cal = true;
      if (ch.format < 0) ch.format = 1;
    } else {
      kernel_pending = true;
    }
  }
  const bool can_tune = plan.ordered && s->dev.ref_leaf_of != nullptr && wide_forced() < 0 && f.all_formats;
  if (can_tune && !ch.refill_cal && !kernel_pending) {
    const int cls = g == 0 ? 0 : 1;
    if (f.frame_format[cls] == -2) {  // one decision per frame and class: all bounce generations of a frame use one format
      std::lock_guard<std::mutex> tune_lock(s->tune_mu);
      f.frame_format[cls] = -1;
      if (tu.decided >= 0) f.frame_format[cls] = tu.decided;
      else if (f.pb.npix >= 65536u && !plan.stats && tu.launched < 16u) {  // the counting instantiation is slower: never timed
        f.frame_format[cls] = (int)(tu.launched++ & 3u);
        f.frame_calibrates[cls] = true;
      }
    }
    if (f.frame_format[cls] >= 0) ch.format = f.frame_format[cls];
    ch.calibrating = f.frame_calibrates[cls];
  }
  return ch;
}

// A fused camera frame of the fused engine is one k_generation (or k_flat_refill) launch, which looks after the work counters itself
// (fused_generation); every other frame has them cleared by frame_run.
bool own_counters(const Frame& f) { return f.fused && !f.plan.wavefront && !f.rays; }

// One generation of the fused engine: one k_generation (or k_flat_refill) launch.
int32_t fused_generation(Frame& f, uint32_t g, const GenQueues& q) {
  RaycaScene* s = f.s;
  FrameCtx* c = f.c;
  const GenChoice ch = choose_generation(f, g);
  // path frames park each lane's ShadeCtx behind the stack rows (kernels.hip, RAYCA_PARK_CTX): kCtxBytes per lane, 6 656 B per
  // wave.  Their LDS part of the stack is capped at path_lds_entries(): four rows of 256 B for the instantiations compiled for five
  // waves per SIMD, so that a wave holds 7 680 B and twenty waves per CU -- what their 96 registers admit -- fit 160 KiB whether LDS
  // is handed out in granules of 512 B or of 1 280 B (8 192 B would round to 8 960 B under the second: eighteen waves); twelve rows
  // for the counting and the sphere instantiations, which stay at four waves (sixteen of 9 728 B fit).  Deeper entries go to the
  // (cold) spill area.  (-DRAYCA_CTX_COMPACT=0: 7 KiB + twelve rows, sixteen waves of 10 KiB.)  What is parked is read back in two
  // parts: the context by every NEE sample that is prepared and by the bounce behind them, the direct sum by the vertex's record.  A
  // generation on the last-vertex form (last_form, select.inc: no vertex of it bounces) reads the sum alone behind its samples; the
  // layout and the allocation are the same for both forms -- its NEE samples still need the context.
  const bool park = RAYCA_PARK_CTX && f.plan.mode == kModePath;
  const bool sph = s->host.sphere_count != 0;
  const bool last = last_form(f.plan.mode, f.cfg, g);
  const TravPlan tp = plan_traversal(s, f.plan.ordered, g, ch.format, park ? path_lds_entries(path_waves(f.plan.stats, sph)) : kMaxLdsEntries);
  f.node_format |= (traits(tp.trav).wide ? (g == 0 ? 1u : 2u) : 0u) | (traits(tp.trav).half ? (g == 0 ? 4u : 8u) : 0u) | (ch.calibrating ? 256u : 0u) |
                   (ch.refill_cal ? 512u : 0u) | (ch.refill ? 1024u : 0u) | (last && g < 16u ? 65536u << g : 0u) |
                   (f.fused && f.plan.mode == kModePath ? 8192u : 0u);
  const StackPlan sp = tp.stack;
  // (k_generation runs as workgroups of kGenBlock threads, k_flat_refill as 256-thread blocks: rows and quads per thread of the workgroup)
  const uint32_t block = ch.refill ? (uint32_t)kBlock : (uint32_t)kGenBlock;
  const size_t lds_bytes = ((size_t)sp.lds_entries * 4u + (park ? (size_t)kCtxBytes : 0u)) * block;
  GenKernel k = pick_kernel(f.plan.mode, g == 0, f.fused, tp.trav, sph, f.plan.stats, last);
  const RefillFlavour rf{tp.trav, sph, f.plan.stats};   // (launched only where choose_generation allows it: one of the kTravFast*)
  const uint32_t batches = g == 0 ? f.fp.tile_count : (f.pb.npix + 63u) / 64u;
  const uint32_t grid_mult = knobs().grid_mult;
  uint32_t grid = 0;
  TraceLaunch tl{};
  int32_t rc = persistent_grid(s, ch.refill ? flat_refill_kernel(rf) : reinterpret_cast<const void*>(k), lds_bytes, batches, true, f.in_flight, grid_mult, grid, block / 64u);
  if (rc != RAYCA_OK || (rc = bind_stack(c, sp, grid, tl, block)) != RAYCA_OK) return rc;
  const uint32_t ticket_forced = knobs().ticket;
  tl.ticket = ticket_forced ? ticket_forced : ticket_policy(batches, grid, block / 64u);
  // The work counters.  A generation of a frame with several launches finds them cleared by frame_run.  A fused camera frame is this
  // one launch, and frame_run leaves the counters to it: k_generation draws from whichever of the context's two sets is known to be
  // zero and zeroes the other one itself (GenArgs.clear), so the next such frame of the context swaps them and neither issues a fill
  // launch -- in the steady state a fused Flat or depth-1 path frame is exactly one launch.  Nothing of this launch reads the set it
  // clears, and whatever drew from that set before has retired: the passes of one context are ordered by the context-pass protocol,
  // which is what k_resolve's clear relies on too.  Only when neither set is known clean (the context's first frame, or behind
  // launches that dirtied both) does a memset go first.  k_flat_refill keeps its own memset of the first set: its frames are
  // milliseconds long.
  uint32_t* heads = c->heads;
  uint32_t* clear = nullptr;
  if (own_counters(f)) {
    if (ch.refill) {
      if (!(c->heads_clean & FrameCtx::kCleanHeads)) HIP_TRY(hipMemsetAsync(c->heads, 0, 8 * kHeadStride * sizeof(uint32_t), f.stream));
      c->heads_clean &= ~FrameCtx::kCleanHeads;
    } else {
      if (!(c->heads_clean & (FrameCtx::kCleanHeads | FrameCtx::kCleanHeadsB))) {
        HIP_TRY(hipMemsetAsync(c->heads_b, 0, 17 * kHeadStride * sizeof(uint32_t), f.stream));
        c->heads_clean = FrameCtx::kCleanAll;
      }
      const bool first = (c->heads_clean & FrameCtx::kCleanHeads) != 0u;
      heads = first ? c->heads : c->heads_b;
      clear = first ? c->heads_b : c->heads;
      c->heads_clean = (c->heads_clean & FrameCtx::kCleanQueues) | (first ? FrameCtx::kCleanHeadsB : FrameCtx::kCleanHeads);
    }
  }
  size_t ev = 0;
  rc = timed_launch(f.log, f.stream, ch.refill ? RAYCA_KERNEL_FLAT_REFILL : RAYCA_KERNEL_GENERATION, f.timing || ch.calibrating || ch.refill_cal, true, [&] {
    if (ch.refill)
      launch_flat_refill(rf, grid, lds_bytes, f.stream, *f.dscene, f.fp, c->heads, f.rgba8, f.rgba32f, c->counters, tl);
    else
      hipLaunchKernelGGL(k, dim3(grid), dim3(kGenBlock), lds_bytes, f.stream,
                         GenArgs{*f.dscene, f.fp, heads, q.in, q.in_count, q.out, q.out_count, f.pb, g, f.rgba8, f.rgba32f, c->counters, tl, clear});
    return RAYCA_OK;
  }, &ev);
  if (rc != RAYCA_OK) return rc;
  if (ch.calibrating) f.tune_events.push_back({g == 0 ? 0 : 1, ev, ch.format, -1});
  if (ch.refill_cal) f.tune_events.push_back({0, ev, ch.format, ch.refill ? 1 : 0});
  return RAYCA_OK;
}

// One launch of the per-pixel stack machine (general.inc) for one sample of the frame.
int32_t stack_machine(Frame& f) {
  RaycaScene* s = f.s;
  FrameCtx* c = f.c;
  const RaycaConfig& cfg = f.cfg;
  GeneralKernel k = pick_general_kernel(s->dev.ref_leaf_of != nullptr, s->host.sphere_count != 0, f.plan.stats);
  const StackPlan sp = plan_stack(s->host.max_depth);
  uint32_t grid = 0;
  int32_t rc = persistent_grid(s, reinterpret_cast<const void*>(k), sp.lds_bytes, f.fp.tile_count, false, 1u, 0u, grid);
  if (rc != RAYCA_OK) return rc;
  // recursion depth of the reference's integrators: Pathtracer vertices live at depth < max_depth (unbounded
  // under roulette: capped, overflow is reported), Raytracer/Scratcher at depth <= max_depth, the others at 0
  uint32_t levels = 1;
  if (cfg.integrator == RAYCA_INTEGRATOR_PATHTRACER) levels = cfg.russian_roulette ? 64u : (cfg.max_depth ? cfg.max_depth : 1u);
  else if (cfg.integrator == RAYCA_INTEGRATOR_RAYTRACER || cfg.integrator == RAYCA_INTEGRATOR_SCRATCHER) levels = cfg.max_depth + 2u;
  if (levels > 256u) return fail(RAYCA_ERR_UNSUPPORTED, "max_depth too large for the path-vertex stack");
  GFrameStore store{};
  store.threads = grid * kBlock;
  store.levels = levels + 1u;
  if ((rc = grow_behind_pass(c, c->frames, (size_t)store.levels * 8u * store.threads * 16u)) != RAYCA_OK) return rc;
  store.frames = static_cast<float4*>(c->frames.ptr);
  if (cfg.direct_sampler == RAYCA_SAMPLER_MIS) {
    if ((rc = grow_behind_pass(c, c->mis_samples, (size_t)2u * kMisMaxSamples * store.threads * 16u)) != RAYCA_OK) return rc;
    store.samples = static_cast<float4*>(c->mis_samples.ptr);
  }
  TraceLaunch tl{};
  if ((rc = bind_stack(c, sp, grid, tl)) != RAYCA_OK) return rc;
  tl.ticket = f.fp.tile_count >= 16u * grid ? 2u : 1u;
  c->heads_clean &= ~FrameCtx::kCleanHeads;
  return timed_launch(f.log, f.stream, RAYCA_KERNEL_OTHER, f.timing, true, [&]() -> int32_t {
    HIP_TRY(hipMemsetAsync(c->heads, 0, 8 * kHeadStride * sizeof(uint32_t), f.stream));
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), sp.lds_bytes, f.stream, s->dev, f.fp, c->heads, f.pb, store, c->counters, tl);
    return RAYCA_OK;
  });
}
// The reference panics (todo!(), unwrap on the wrong material kind, stack overflow under roulette) where the stack machine
// raises these flags; the frame is not usable then.
int32_t stack_machine_status(Frame& f) {
  HIP_TRY(hipStreamSynchronize(f.stream));
  TraceCounters tc{};
  HIP_TRY(hipMemcpy(&tc, f.c->counters, sizeof tc, hipMemcpyDeviceToHost));
  if (tc.flags & kFlagTooDeep) return fail(RAYCA_ERR_UNSUPPORTED, "path recursion deeper than the path-vertex stack (Russian roulette did not terminate within 64 bounces)");
  if (tc.flags & kFlagUnsupported)
    return fail(RAYCA_ERR_UNSUPPORTED, "this Config reaches a todo!()/panic arm of the reference on this scene (e.g. directional light under NEE, quad light under Raytracer/Scratcher, get_t of a Pbr material, Whitted radiance of a Ggx material)");
  return RAYCA_OK;
}

// k_resolve: the path records of one sample into the pixels.  On the generation engines the same launch clears the work
// counters for the next frame of this context (see k_resolve).
int32_t resolve(Frame& f) {
  FrameCtx* c = f.c;
  const bool general = f.plan.mode == kModeGeneral;
  const int32_t rc = timed_launch(f.log, f.stream, RAYCA_KERNEL_OTHER, f.timing, false, [&] {
    hipLaunchKernelGGL(k_resolve, dim3((f.pb.npix + kBlock - 1) / kBlock), dim3(kBlock), 0, f.stream, f.fp, f.pb, f.plan.generations,
                       static_cast<float4*>(c->accum.ptr), f.rgba8, f.rgba32f, general ? nullptr : c->heads_b, 17u * kHeadStride);
    return RAYCA_OK;
  });
  if (rc == RAYCA_OK && !general) c->heads_clean = FrameCtx::kCleanAll;
  return rc;
}

// A calibration frame: book its kernel time for the node format (or camera-ray kernel) it was launched with.
int32_t book_calibration(Frame& f) {
  RaycaScene* s = f.s;
  HIP_TRY(hipStreamSynchronize(f.stream));
  float sum[2] = {0.0f, 0.0f};
  int fmt[2] = {-1, -1};
  int refill_choice = -1;
  float refill_ms = 0.0f;
  for (const TuneEvent& te : f.tune_events) {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, f.c->ev_trace[te.ev], f.c->ev_trace[te.ev + 1]));
    if (te.refill >= 0) {
      refill_choice = te.refill;
      refill_ms = ms;
      continue;
    }
    sum[te.cls] += ms;
    fmt[te.cls] = te.format;  // all bounce generations of one frame are launched with one format
  }
  std::lock_guard<std::mutex> tune_lock(s->tune_mu);
  if (refill_choice >= 0) {
    RaycaScene::Tune& tu = s->tune[0][0];
    if (refill_ms < tu.refill_best[refill_choice]) tu.refill_best[refill_choice] = refill_ms;
    if (++tu.refill_booked == 8u) tu.refill = tu.refill_best[1] < tu.refill_best[0] ? 1 : 0;
  }
  for (int cls = 0; cls < 2; ++cls) {
    if (fmt[cls] < 0) continue;
    RaycaScene::Tune& tu = s->tune[f.plan.mode == kModePath ? 1 : 0][cls];
    if (sum[cls] < tu.best[fmt[cls] & 3]) tu.best[fmt[cls] & 3] = sum[cls];
    if (++tu.booked == 16u) {
      int pick = 0;
      for (int p = 1; p < 4; ++p)
        if (tu.best[p] < tu.best[pick]) pick = p;
      tu.decided = pick;
    }
  }
  return RAYCA_OK;
}

int32_t fill_stats(Frame& f, RaycaStats* out) {
  FrameCtx* c = f.c;
  const bool general = f.plan.mode == kModeGeneral;
  HIP_TRY(hipStreamSynchronize(f.stream));
  TraceCounters tc{};
  HIP_TRY(hipMemcpy(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost));
  if (f.plan.wavefront && !general) {
    std::vector<unsigned long long> lines(64 * 16);
    HIP_TRY(hipMemcpy(lines.data(), c->shade_stats, lines.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t l = 0; l < 64; ++l) {
      tc.shaded += lines[l * 16 + 0];
      tc.shadow += lines[l * 16 + 1];
      tc.bounce += lines[l * 16 + 2];
    }
  }
  std::memset(out, 0, sizeof *out);
  out->rays_primary = (uint64_t)f.pb.npix * f.cfg.samples_per_pixel;
  out->rays_shadow = tc.shadow;
  out->rays_bounce = tc.bounce;
  out->boxes_tested = tc.boxes;
  out->triangles_tested = tc.tris;
  out->hits_shaded = tc.shaded;
  out->wave_box_slots = tc.box_slots;
  out->wave_triangle_slots = tc.tri_slots;
  // RAYCA_NEE_SKIP_REPORT: how many of the frame's NEE samples could not contribute on stderr, for frames of the fused engine with collect_stats (only k_generation counts them) --
  // RaycaStats has no room for it and its layout is pinned
  static const bool nee_report = getenv("RAYCA_NEE_SKIP_REPORT") != nullptr;
  if (nee_report && f.plan.mode == kModePath && !f.plan.wavefront && f.plan.stats) fprintf(stderr, "[rayca nee] irrelevant %llu of %llu samples, skip %s\n", tc.nee_irrelevant, tc.shadow, f.fp.nee_skip ? "on" : "off");
  HIP_TRY(hipEventElapsedTime(&out->kernel_ms, c->ev_begin, c->ev_end));
  float tsum = 0.0f;
  for (size_t i = 0; i + 1 < f.log.ev_used; i += 2) {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_trace[i], c->ev_trace[i + 1]));
    const int cls = i / 2 < f.log.ev_class.size() ? f.log.ev_class[i / 2] : RAYCA_KERNEL_OTHER;
    out->class_ms[cls] += ms;
    out->class_launches[cls] += 1u;
    if (cls != RAYCA_KERNEL_WF_SHADE && (cls != RAYCA_KERNEL_OTHER || general)) tsum += ms;   // the traversal kernels (the stack machine is one)
  }
  out->trace_kernel_ms = tsum;
  out->kernel_launches = f.log.launches;
  out->trace_kernel_launches = f.log.trace_launches;
  out->rows_rendered = f.fp.rows;
  out->node_format = f.node_format;
  return RAYCA_OK;
}

// The statistics of several frames that one call ran (rayca_hip_gather_device's internal frames) as one: every counter, time and
// launch count summed -- rows_rendered becomes the number of frames where each is one row -- and node_format ORed.  Every field of
// RaycaStats is named here: the size pins the list, so that a field added to the struct is added here too.
void stats_add(RaycaStats& total, const RaycaStats& s) {
  static_assert(sizeof(RaycaStats) == 8 * sizeof(uint64_t) + 2 * sizeof(float) + 4 * sizeof(uint32_t) + RAYCA_KERNEL_CLASSES * (sizeof(float) + sizeof(uint32_t)),
                "RaycaStats has a field that stats_add does not sum");
  total.rays_primary += s.rays_primary; total.rays_shadow += s.rays_shadow; total.rays_bounce += s.rays_bounce;
  total.boxes_tested += s.boxes_tested; total.triangles_tested += s.triangles_tested; total.hits_shaded += s.hits_shaded;
  total.wave_box_slots += s.wave_box_slots; total.wave_triangle_slots += s.wave_triangle_slots;
  total.kernel_ms += s.kernel_ms; total.trace_kernel_ms += s.trace_kernel_ms;
  total.kernel_launches += s.kernel_launches; total.trace_kernel_launches += s.trace_kernel_launches;
  total.rows_rendered += s.rows_rendered;
  total.node_format |= s.node_format;
  for (int k = 0; k < RAYCA_KERNEL_CLASSES; ++k) {
    total.class_ms[k] += s.class_ms[k];
    total.class_launches[k] += s.class_launches[k];
  }
}

// What camera_ray() and the pixel <-> packed-row mapping of the kernels read from FrameParams, for every call that makes a
// frame's camera rays (render_body, rayca_hip_camera_rays_device).  The two halves of one set-up: per frame the tile, the
// image geometry and the camera -- RAYCA_ERR_BAD_ARG for a tile that names no part; fp.rows == 0 means "nothing to do" --
// and per sample the sub-pixel terms.  The caller has checked that the scene has a camera.
int32_t camera_frame_params(const RaycaScene* s, uint32_t width, uint32_t height, const RaycaTile& tile_in, FrameParams& fp) {
  RaycaTile tile = tile_in;
  if (tile.parts == 0) { tile.parts = 1; tile.part = 0; }
  if (tile.part >= tile.parts) return fail(RAYCA_ERR_BAD_ARG, "tile.part >= tile.parts");
  if (tile.band_rows == 0) tile.band_rows = 1;
  const uint32_t rows = tile_rows(tile, height);
  fp.width = width; fp.height = height; fp.rows = rows;
  fp.part = tile.part; fp.parts = tile.parts; fp.band = tile.band_rows;
  fp.tiles_x = (width + kTileW - 1u) / kTileW;
  fp.tile_count = fp.tiles_x * ((rows + kTileH - 1u) / kTileH);
  const float fw = (float)width, fh = (float)height;
  fp.inv_width = 1.0f / fw;   // scene.rs:106-107
  fp.inv_height = 1.0f / fh;
  fp.aspect = fw / fh;        // scene.rs:114
  fp.angle = tanf(s->host.camera_yfov * 0.5f);  // Camera::get_angle  camera.rs:74-76
  fp.camera = s->host.world_trs[s->host.camera_node];
  return RAYCA_OK;
}
// (the strata of a pixel: `count` a side, `step` apart, the first one `offset` in -- what rayca_hip_sample_plan_device hands its ray
// kernel, which picks a stratum per ray)
struct SubPixelGrid { float step, offset; uint32_t count; };
SubPixelGrid sub_pixel_grid(uint32_t spp) {
  const float strate = sqrtf((float)spp);  // scene.rs:125-127
  return SubPixelGrid{1.0f / strate, 0.5f / strate, (uint32_t)strate};
}
void camera_sample_params(uint32_t spp, uint32_t sample, FrameParams& fp) {
  const SubPixelGrid grid = sub_pixel_grid(spp);
  const float sub_offset = grid.offset, sub_step = grid.step;
  const uint32_t sc_i = grid.count;
  const float ix = (float)(sample % sc_i), iy = (float)(sample / sc_i);  // scene.rs:130-131
  fp.sample = sample;
  fp.sub_step_x = ix * sub_step;
  fp.sub_step_y = iy * sub_step;
  fp.sub_offset = sub_offset;
}

// What the integrators read from FrameParams: the Config of the frame (f.cfg, f.plan and f.dscene are set).
void config_frame_params(const Frame& f, FrameParams& fp) {
  const RaycaConfig& cfg = f.cfg;
  fp.integrator = cfg.integrator; fp.direct_sampler = cfg.direct_sampler; fp.indirect_sampler = cfg.indirect_sampler;
  fp.light_samples = cfg.light_samples; fp.light_stratify = cfg.light_stratify;
  fp.strate_count = cfg.light_stratify ? (uint32_t)sqrtf((float)cfg.light_samples) : 1u;  // config.rs:73-79
  fp.max_depth = cfg.max_depth; fp.russian_roulette = cfg.russian_roulette; fp.seed = cfg.seed; fp.spp = cfg.samples_per_pixel;
  fp.inv_gamma = 1.0f / cfg.gamma;  // color/mod.rs:175-176
  // Not with exhaustive traversal, which reproduces the reference's test counts: every sample traced.  And not where the tree is a
  // single leaf: a ray's whole search is then the root box and that leaf -- there is no traversal to save -- and the accounting
  // "every counted ray has tested the root box" (boxes_tested >= rays, exact for such a scene: tests/test_gpu_engines.py) holds.
  fp.nee_skip = f.s->nee_skip && f.plan.ordered && !(f.dscene->root_ref & kLeafFlag) ? 1u : 0u;
}

// ---- the frame driver: what render_body and rayca_hip_radiance_device run behind their own checks and pass_acquire ---------
// A frame and a radiance query are the same passes over the same buffers: frame_begin, frame_run, frame_finish.  They differ
// in three places, all read off f.rays: generation 0's input (nothing for camera rays; queue 1, which one k_enqueue_rays
// launch fills, for a caller's -- or one k_enqueue_gather launch, for the rays rayca_hip_gather_device makes), queue 1 (a caller's rays need it even at depth 1 and for Flat), and where the Frame gets its
// shape (the caller sets the geometry of f.fp: the camera and tile, or one row of `count` pixels).

// The Frame of an acquired pass and its path buffers.  The caller has set s, cfg, opts, plan, rays and the geometry of fp.
int32_t frame_begin(Frame& f, const ContextPass& pass, void* d_rgba8, void* d_rgba32f) {
  RaycaScene* s = f.s;
  FrameCtx* c = f.c = f.log.c = pass.c;
  const LaunchPlan& plan = f.plan;
  f.stream = pass.stream;
  f.timing = pass.timing;
  int32_t rc;
  // The wavefront engine's kernels are tied to the 4-wide / fp16 nodes, and so is a pinned format: those wait for the thread
  // that makes them.  Everything else renders on the binary f32 nodes until they are there (node_format bit 2048).
  if ((plan.wavefront || format_forced() > 0) && (rc = formats_wait(s)) != RAYCA_OK) return rc;
  f.all_formats = formats_ready(s);
  f.dscene = f.all_formats ? &s->dev_full : &s->dev;
  f.in_flight = frames_in_flight_hint(s, f.opts.context, f.opts.stream != nullptr);
  f.node_format = (f.all_formats ? 0u : 2048u) | (RAYCA_NODE_CH && RAYCA_NODE_CH48 && f.dscene->nodes_ch ? 4096u : 0u);
  f.rgba8 = static_cast<uint8_t*>(d_rgba8);
  f.rgba32f = static_cast<float4*>(d_rgba32f);
  // Flat, one sample: the generation kernel writes the pixel itself.  So does the one-sample depth-1 path frame of the fused engine
  // (fuse_resolve, select.inc), since its generation runs the last-vertex form: that fusion was measured and lost twice while the
  // kernel carried the direct sum through trace() and spilled; the third measurement is in DESIGN.md (the k_generation table).
  // Every other path frame resolves in a pass of its own.
  f.fused = (f.cfg.samples_per_pixel == 1 && plan.mode == kModeFlat) || fuse_resolve(plan, f.cfg, f.rays != nullptr);
  config_frame_params(f, f.fp);

  // One record per pixel and depth; the two queues where a path bounces, queue 1 also where generation 0 reads the caller's rays.
  PathBuffers& pb = f.pb;
  const uint32_t npix = pb.npix = f.fp.rows * f.fp.width;
  const size_t records = (size_t)npix * (plan.generations ? plan.generations : 1);
  const bool path = plan.mode == kModePath, bounces = path && plan.generations > 1;
  if (!f.fused) {
    if ((rc = grow_behind_pass(c, c->path_direct, records * 16)) != RAYCA_OK) return rc;
    if ((rc = grow_behind_pass(c, c->path_state, records * 4)) != RAYCA_OK) return rc;
    if (path && (rc = grow_behind_pass(c, c->path_brdf, records * 16)) != RAYCA_OK) return rc;
    if (f.cfg.samples_per_pixel > 1 && (rc = grow_behind_pass(c, c->accum, (size_t)npix * 16)) != RAYCA_OK) return rc;
    pb.direct = static_cast<float4*>(c->path_direct.ptr);
    pb.brdf = static_cast<float4*>(c->path_brdf.ptr);
    pb.state = static_cast<uint32_t*>(c->path_state.ptr);
  }
  if (bounces && (rc = grow_behind_pass(c, c->queue[0], (size_t)npix * sizeof(QueuedRay))) != RAYCA_OK) return rc;
  if ((bounces || f.rays) && (rc = grow_behind_pass(c, c->queue[1], (size_t)npix * sizeof(QueuedRay))) != RAYCA_OK) return rc;
  return RAYCA_OK;
}

// Every sample and generation of the frame, up to k_resolve.
int32_t frame_run(Frame& f) {
  FrameCtx* c = f.c;
  const hipStream_t stream = f.stream;
  const LaunchPlan& plan = f.plan;
  const bool general = plan.mode == kModeGeneral;
  const uint32_t npix = f.pb.npix, depths = plan.generations, spp = f.cfg.samples_per_pixel;
  int32_t rc;
  if (f.timing || general) HIP_TRY(hipMemsetAsync(c->counters, 0, kCountersBytes, stream));
  if (f.timing) HIP_TRY(hipEventRecord(c->ev_begin, stream));
  uint32_t* q_count = c->heads + 8 * kHeadStride;  // the two queue counters
  for (uint32_t sample = 0; sample < spp; ++sample) {
    // (a caller's rays: fp.sample stays 0, the one sample k_resolve finalises; the paths' stream is rays->sample, in the queue's keys)
    if (!f.rays) camera_sample_params(spp, sample, f.fp);
    if (!f.fused && depths > 1) HIP_TRY(hipMemsetAsync(f.pb.state + npix, 0, (size_t)npix * (depths - 1) * 4, stream));
    if (general && (rc = stack_machine(f)) != RAYCA_OK) return rc;
    for (uint32_t g = 0; !general && g < depths; ++g) {
      // generation 0 clears the work counters and both queue counters in one go (unless k_resolve of the previous frame
      // left them clean); later generations must keep the input queue's counter.  One memset clears both counter sets (the
      // second one is only used by the wavefront engine), in whole lines: a size that is not a multiple of the fill
      // kernel's granule costs a second fill launch, ~5 us.  (Not for a fused camera frame of the fused engine: own_counters.)
      if (!own_counters(f)) {
        if (!(g == 0 && c->heads_clean == FrameCtx::kCleanAll))
          HIP_TRY(hipMemsetAsync(c->heads_b, 0, (16 * kHeadStride + (g == 0 ? kHeadStride : 0)) * sizeof(uint32_t), stream));
        c->heads_clean = 0u;
      }
      // generation g reads what generation g - 1 wrote; generation 0 the caller's rays in queue 1, which generation 1 writes
      // over once they are read, or nothing (the camera)
      const int in = g ? (int)((g - 1) & 1) : (f.rays ? 1 : -1);
      const GenQueues q{in < 0 ? nullptr : static_cast<QueuedRay*>(c->queue[in].ptr), in < 0 ? nullptr : q_count + in,
                        static_cast<QueuedRay*>(c->queue[g & 1].ptr), q_count + (g & 1)};
      if (g != 0) HIP_TRY(hipMemsetAsync(q.out_count, 0, sizeof(uint32_t), stream));
      else if (f.rays) {
        const RayFeed& feed = *f.rays;
        rc = timed_launch(f.log, stream, RAYCA_KERNEL_OTHER, f.timing, false, [&] {
          const dim3 grid((npix + kBlock - 1u) / kBlock);
          if (feed.gather)
            hipLaunchKernelGGL(pick_gather_enqueue(feed.gather->a.rotations != nullptr), grid, dim3(kBlock), 0, stream, *feed.gather, f.cfg.seed, feed.sample, q.in, q.in_count);
          else
            hipLaunchKernelGGL(k_enqueue_rays, grid, dim3(kBlock), 0, stream, feed.rays, npix, feed.first_index, f.cfg.seed, feed.sample, q.in, q.in_count);
          return RAYCA_OK;
        });
        if (rc != RAYCA_OK) return rc;
      }
      if ((rc = plan.wavefront ? wavefront_generation(f, g, q) : fused_generation(f, g, q)) != RAYCA_OK) return rc;
    }
    if (!f.fused && (rc = resolve(f)) != RAYCA_OK) return rc;
  }
  return RAYCA_OK;
}

// Behind the last launch: the pass retires, a calibration frame books its times, the stack machine reports its flags, then the
// statistics -- or the rule of every pass: one on the context's own stream is synchronous.  `caller_drains`: the caller waits
// for that stream itself (rayca_hip_render behind its copies, the parts of rayca_hip_render_multi behind their exchange).
int32_t frame_finish(Frame& f, const ContextPass& pass, RaycaStats* stats_out, bool caller_drains) {
  int32_t rc = pass_retire(pass);
  if (rc != RAYCA_OK) return rc;
  if (!f.tune_events.empty() && (rc = book_calibration(f)) != RAYCA_OK) return rc;
  if (f.plan.mode == kModeGeneral && (rc = stack_machine_status(f)) != RAYCA_OK) return rc;
  if (f.timing) return fill_stats(f, stats_out);
  return caller_drains ? RAYCA_OK : pass_finish(pass, f.log.launches, nullptr);
}

// One frame: the three differences above are the camera's -- f.rays stays null, and camera_frame_params gives the Frame its
// shape.  The caller holds the frame context's mutex (render_impl and rayca_hip_render take it): everything a
// context owns -- work buffers, events, its stream, the staging buffers of rayca_hip_render -- is touched under it.
int32_t render_body(RaycaScene* s, const RaycaConfig* cfg_in, uint32_t width, uint32_t height, const RaycaRenderOptions* opts_in,
                    void* d_rgba8, void* d_rgba32f, RaycaStats* stats_out, bool caller_drains) {
  if (!s || !cfg_in) return fail(RAYCA_ERR_BAD_ARG, "null scene or config");
  if (width == 0 || height == 0) return fail(RAYCA_ERR_BAD_ARG, "empty image");
  if (!s->host.has_camera) return fail(RAYCA_ERR_NO_CAMERA, "scene has no camera (scene.rs:109)");
  if (const int32_t e = refuse_empty_scene(s); e != RAYCA_OK) return e;
  Frame f{};
  f.s = s;
  const RaycaConfig& cfg = f.cfg = *cfg_in;
  const RaycaRenderOptions& opts = f.opts;
  if (opts_in) f.opts = *opts_in;
  LaunchPlan& plan = f.plan;
  plan.ordered = opts.traversal != RAYCA_TRAVERSAL_EXHAUSTIVE;
  plan.stats = opts.collect_stats != 0;
  int32_t rc = validate_config(s, cfg, opts.engine, plan);
  if (rc != RAYCA_OK) return rc;
  if (opts.camera_rays > RAYCA_CAMERA_REFILL) return fail(RAYCA_ERR_BAD_ARG, "unknown camera_rays choice");
  if ((rc = camera_frame_params(s, width, height, opts.tile, f.fp)) != RAYCA_OK) return rc;
  if (f.fp.rows == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if (opts.context >= kMaxContexts) return fail(RAYCA_ERR_BAD_ARG, "context out of range");
  ContextPass pass{};
  if ((rc = pass_acquire(s, opts, stats_out != nullptr, pass)) != RAYCA_OK) return rc;
  if ((rc = frame_begin(f, pass, d_rgba8, d_rgba32f)) != RAYCA_OK || (rc = frame_run(f)) != RAYCA_OK) return rc;
  return frame_finish(f, pass, stats_out, caller_drains);
}

// rayca_hip_render_device: takes the context's mutex around the frame.  With opts->stream == NULL the frame runs on the
// context's own (non-blocking) stream, which the caller has no handle to wait on: that case is synchronous (frame_finish).
int32_t render_impl(RaycaScene* s, const RaycaConfig* cfg, uint32_t width, uint32_t height, const RaycaRenderOptions* opts,
                    void* d_rgba8, void* d_rgba32f, RaycaStats* stats_out) {
  if (!s) return fail(RAYCA_ERR_BAD_ARG, "null scene or config");
  const uint32_t context = opts ? opts->context : 0u;
  if (context >= kMaxContexts) return fail(RAYCA_ERR_BAD_ARG, "context out of range");
  std::lock_guard<std::mutex> lock(s->ctx[context].mu);
  return render_body(s, cfg, width, height, opts, d_rgba8, d_rgba32f, stats_out, false);
}

}  // namespace

// ---- the kernels of the host API, and the several-devices frame ------------------------------------------------------------
namespace {
#include "aux_kernels.inc"
}  // namespace

#include "multi.inc"

extern "C" {

uint32_t rayca_hip_version(void) { return RAYCA_ABI_VERSION; }

int32_t rayca_hip_selftest(void) {
  std::string err;
  int32_t rc = selftest_half_rounding(err);
  if (rc == RAYCA_OK) rc = selftest_device_layouts(err);
  if (rc == RAYCA_OK) rc = selftest_kernel_selection(err);
  if (rc == RAYCA_OK) rc = selftest_grid_policy(err);
  return rc == RAYCA_OK ? RAYCA_OK : fail(rc, err);
}

int32_t rayca_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void rayca_hip_last_error(char* buf, size_t len) {
  if (!buf || !len) return;
  std::snprintf(buf, len, "%s", g_last_error.c_str());
}

void rayca_hip_config_default(RaycaConfig* out) {  // config.rs:10-49
  if (!out) return;
  std::memset(out, 0, sizeof *out);
  out->bvh = 1;
  out->light_samples = 1;
  out->light_stratify = 0;
  out->samples_per_pixel = 1;
  out->russian_roulette = 0;
  out->direct_sampler = RAYCA_SAMPLER_NEE;
  out->indirect_sampler = RAYCA_SAMPLER_COSINE;
  out->integrator = RAYCA_INTEGRATOR_PATHTRACER;
  out->max_depth = 5;
  out->gamma = 1.0f;
}

uint32_t rayca_hip_tile_rows(const RaycaTile* tile, uint32_t height) {
  if (!tile) return height;
  return tile_rows(*tile, height);
}

}  // extern "C"

#include "scene.inc"

extern "C" {

int32_t rayca_hip_render_device(RaycaScene* s, const RaycaConfig* cfg, uint32_t width, uint32_t height, const RaycaRenderOptions* opts,
                                void* d_rgba8_out, void* d_rgba32f_out, RaycaStats* stats_out) {
  return render_impl(s, cfg, width, height, opts, d_rgba8_out, d_rgba32f_out, stats_out);
}

int32_t rayca_hip_render(RaycaScene* s, const RaycaConfig* cfg, uint32_t width, uint32_t height, const RaycaRenderOptions* opts, uint8_t* rgba8_out,
                         float* rgba32f_out, RaycaStats* stats_out) {
  if (!s) return fail(RAYCA_ERR_BAD_ARG, "null scene");
  RaycaRenderOptions o{};
  if (opts) o = *opts;
  RaycaTile tile = o.tile;
  if (tile.parts == 0) { tile.parts = 1; tile.part = 0; }
  const uint32_t rows = tile_rows(tile, height);
  const size_t npix = (size_t)rows * width;
  HIP_TRY(hipSetDevice(s->device));
  int32_t rc;
  if (o.context >= kMaxContexts) return fail(RAYCA_ERR_BAD_ARG, "context out of range");
  FrameCtx* c = &s->ctx[o.context];
  // the staging buffers belong to the context: held from here until the copies have landed, so that two host threads
  // rendering with one context cannot regrow or overwrite them under each other
  std::lock_guard<std::mutex> lock(c->mu);
  static const bool lap_on = getenv("RAYCA_RENDER_TIMING") != nullptr;   // phase times of this call on stderr
  auto lap_t = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!lap_on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[rayca render] %-28s %8.2f ms\n", what, std::chrono::duration<float, std::milli>(now - lap_t).count());
    lap_t = now;
  };
  if ((rc = ensure_ctx(s, c)) != RAYCA_OK) return rc;
  lap("frame context");
  if (rgba8_out && (rc = grow_behind_pass(c, c->out8, npix * 4 + 16)) != RAYCA_OK) return rc;
  if (rgba32f_out && (rc = grow_behind_pass(c, c->out32, npix * 16 + 16)) != RAYCA_OK) return rc;
  lap("staging buffers");
  // (no statistics unless asked for: they cost two event records per launch, a stream synchronisation and a read-back)
  rc = render_body(s, cfg, width, height, &o, rgba8_out ? c->out8.ptr : nullptr, rgba32f_out ? c->out32.ptr : nullptr, stats_out, true);
  if (rc != RAYCA_OK) return rc;
  lap("render_body (issue)");
  hipStream_t stream = o.stream ? static_cast<hipStream_t>(o.stream) : c->stream;
  if (lap_on) {
    HIP_TRY(hipStreamSynchronize(stream));
    lap("kernels done");
  }
  if (rgba8_out && npix) HIP_TRY(hipMemcpyAsync(rgba8_out, c->out8.ptr, npix * 4, hipMemcpyDeviceToHost, stream));
  if (rgba32f_out && npix) HIP_TRY(hipMemcpyAsync(rgba32f_out, c->out32.ptr, npix * 16, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  lap("copy out");
  return RAYCA_OK;
}

}  // extern "C"

// The resident draw(): the layer that decides, per call, between rendering the resident scene as it is, updating it in place
// and rebuilding it.  The decision is host code (desc_compare, host_scene.cpp): the device holds the flattened world-space
// scene, not the descriptor, so there is nothing on the device to compare a descriptor with.
struct RaycaRenderer {
  std::mutex mu;
  RaycaBuildOptions opts{};
  RaycaScene* scene = nullptr;
  KeptDesc kept;             // the descriptor `scene` was created from (and updated with since)
  bool invalidated = false;  // rayca_hip_renderer_invalidate: the next draw rebuilds
  uint32_t last_action = RAYCA_NONE;
  float last_ms[RAYCA_DRAW_MS_COUNT] = {0, 0, 0, 0};
  uint64_t builds = 0, updates = 0, reuses = 0;
};

extern "C" {

int32_t rayca_hip_renderer_create(const RaycaBuildOptions* opts, RaycaRenderer** out) {
  if (!out) return fail(RAYCA_ERR_BAD_ARG, "null out pointer");
  *out = nullptr;
  RaycaBuildOptions o{};
  o.builder = RAYCA_BUILDER_SAH;
  if (opts) o = *opts;
  if (o.builder != RAYCA_BUILDER_REFERENCE && o.builder != RAYCA_BUILDER_SAH) return fail(RAYCA_ERR_BAD_ARG, "unknown builder");
  RaycaRenderer* r = new RaycaRenderer();
  r->opts = o;
  *out = r;
  return RAYCA_OK;
}

int32_t rayca_hip_renderer_draw(RaycaRenderer* r, const RaycaSceneDesc* desc, const RaycaConfig* cfg, uint32_t width, uint32_t height,
                                const RaycaRenderOptions* opts, uint8_t* rgba8_out, float* rgba32f_out, RaycaStats* stats_out, uint32_t* action_out) {
  if (action_out) *action_out = RAYCA_NONE;
  if (!r || !desc) return fail(RAYCA_ERR_BAD_ARG, "null renderer or descriptor");
  std::lock_guard<std::mutex> lock(r->mu);
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t) { return std::chrono::duration<float, std::milli>(clock::now() - t).count(); };
  const bool use_bvh = cfg ? cfg->bvh != 0 : true;
  float ms[RAYCA_DRAW_MS_COUNT] = {0, 0, 0, 0};
  std::string err;
  uint32_t action = RAYCA_DRAW_REBUILT;
  SceneGraph graph;   // scene_graph_pass(desc), unless REUSED
  const auto t_compare = clock::now();
  if (r->scene && r->kept.valid && !r->invalidated) {
    if (const int32_t rc = desc_compare(r->kept.view, r->kept.bvh, &r->kept.graph, *desc, use_bvh, action, graph, err); rc != RAYCA_OK) return fail(rc, err);
  } else {
    if (const int32_t rc = desc_validate(*desc, err); rc != RAYCA_OK) return fail(rc, err);
    if (const int32_t rc = scene_graph_pass(*desc, graph, err); rc != RAYCA_OK) return fail(rc, err);
  }
  ms[RAYCA_DRAW_MS_COMPARE] = ms_since(t_compare);
  if (action == RAYCA_DRAW_UPDATED) {
    const auto t = clock::now();
    const int32_t rc = rayca_hip_scene_update(r->scene, desc);
    if (rc == RAYCA_ERR_UNSUPPORTED) action = RAYCA_DRAW_REBUILT;   // (the same check said otherwise a moment ago: cannot happen)
    else if (rc != RAYCA_OK) return rc;
    else {
      r->kept.refresh(*desc, std::move(graph));
      r->updates++;
      ms[RAYCA_DRAW_MS_UPDATE] = ms_since(t);
    }
  }
  if (action == RAYCA_DRAW_REBUILT) {
    // what render would refuse in every frame is refused before anything is built: such a descriptor evicts nothing
    if (!graph.has_camera) return fail(RAYCA_ERR_NO_CAMERA, "scene has no camera (scene.rs:109)");
    const auto t = clock::now();
    // (the copy for the comparisons to come is made by a thread of its own, under the build)
    KeptDesc fresh;
    std::thread copier([&] { fresh.assign(*desc, use_bvh, std::move(graph)); });
    RaycaScene* made = nullptr;
    const int32_t rc = rayca_hip_scene_create(desc, cfg, &r->opts, &made);
    const std::string create_err = g_last_error;
    copier.join();
    if (rc != RAYCA_OK) return fail(rc, create_err);   // the old scene stays resident, with its copy
    if (r->scene) (void)rayca_hip_scene_destroy(r->scene);
    r->scene = made;
    r->kept = std::move(fresh);
    r->invalidated = false;
    r->builds++;
    ms[RAYCA_DRAW_MS_BUILD] = ms_since(t);
  }
  const auto t_render = clock::now();
  if (const int32_t rc = rayca_hip_render(r->scene, cfg, width, height, opts, rgba8_out, rgba32f_out, stats_out); rc != RAYCA_OK) return rc;
  ms[RAYCA_DRAW_MS_RENDER] = ms_since(t_render);
  if (action == RAYCA_DRAW_REUSED) r->reuses++;
  r->last_action = action;
  std::copy(ms, ms + RAYCA_DRAW_MS_COUNT, r->last_ms);
  if (action_out) *action_out = action;
  return RAYCA_OK;
}

int32_t rayca_hip_renderer_last_draw(const RaycaRenderer* cr, uint32_t* action_out, float* ms_out, uint64_t* counters_out) {
  if (!cr) return fail(RAYCA_ERR_BAD_ARG, "null renderer");
  RaycaRenderer* r = const_cast<RaycaRenderer*>(cr);   // (its mutex)
  std::lock_guard<std::mutex> lock(r->mu);
  if (action_out) *action_out = r->last_action;
  if (ms_out) std::copy(r->last_ms, r->last_ms + RAYCA_DRAW_MS_COUNT, ms_out);
  if (counters_out) {
    counters_out[RAYCA_DRAW_N_BUILDS] = r->builds;
    counters_out[RAYCA_DRAW_N_UPDATES] = r->updates;
    counters_out[RAYCA_DRAW_N_REUSES] = r->reuses;
    counters_out[RAYCA_DRAW_N_KEPT_BYTES] = r->kept.bytes();
  }
  return RAYCA_OK;
}

int32_t rayca_hip_renderer_scene(RaycaRenderer* r, RaycaScene** out) {
  if (!r || !out) return fail(RAYCA_ERR_BAD_ARG, "null renderer or out pointer");
  std::lock_guard<std::mutex> lock(r->mu);
  *out = r->scene;
  return RAYCA_OK;
}

int32_t rayca_hip_renderer_invalidate(RaycaRenderer* r) {
  if (!r) return fail(RAYCA_ERR_BAD_ARG, "null renderer");
  std::lock_guard<std::mutex> lock(r->mu);
  r->invalidated = true;
  return RAYCA_OK;
}

int32_t rayca_hip_renderer_destroy(RaycaRenderer* r) {
  if (!r) return RAYCA_OK;
  RaycaScene* scene = nullptr;
  {
    std::lock_guard<std::mutex> lock(r->mu);   // (a draw still running on another thread finishes first)
    scene = r->scene;
    r->scene = nullptr;
  }
  delete r;
  return rayca_hip_scene_destroy(scene);
}

int32_t rayca_hip_scene_desc_compare(const RaycaSceneDesc* resident, uint32_t resident_bvh, const RaycaSceneDesc* next, uint32_t next_bvh,
                                     uint32_t* action_out) {
  if (action_out) *action_out = RAYCA_NONE;
  if (!resident || !next || !action_out) return fail(RAYCA_ERR_BAD_ARG, "null descriptor or out pointer");
  std::string err;
  if (const int32_t rc = desc_validate(*resident, err); rc != RAYCA_OK) return fail(rc, "resident: " + err);
  SceneGraph graph;
  uint32_t action = RAYCA_DRAW_REBUILT;
  if (const int32_t rc = desc_compare(*resident, resident_bvh != 0, nullptr, *next, next_bvh != 0, action, graph, err); rc != RAYCA_OK) return fail(rc, err);
  *action_out = action;
  return RAYCA_OK;
}

int32_t rayca_hip_trace_rays(RaycaScene* s, const RaycaRenderOptions* opts, uint32_t count, const float* rays, float* t_out, uint32_t* prim_out,
                             float* uv_out, RaycaStats* stats_out) {
  if (!s || !rays || !t_out || !prim_out || !uv_out) return fail(RAYCA_ERR_BAD_ARG, "null argument");
  if (const int32_t e = refuse_empty_scene(s); e != RAYCA_OK) return e;
  if (count == 0) return RAYCA_OK;
  FrameCtx* c = &s->ctx[0];
  std::lock_guard<std::mutex> lock(c->mu);
  // a pass on context 0 and its own stream, whatever opts names: behind a frame in flight there, which owns the buffers below
  ContextPass pass{};
  int32_t rc = pass_acquire(s, RaycaRenderOptions{}, true, pass);
  if (rc != RAYCA_OK) return rc;
  const bool ordered = !opts || opts->traversal != RAYCA_TRAVERSAL_EXHAUSTIVE;
  const bool stats = opts && opts->collect_stats;
  const size_t in_bytes = (size_t)count * 24, out_bytes = (size_t)count * 16;
  rc = grow_behind_pass(c, c->ray_io, in_bytes + out_bytes);
  if (rc != RAYCA_OK) return rc;
  char* base = static_cast<char*>(c->ray_io.ptr);
  float* d_rays = reinterpret_cast<float*>(base);
  float* d_t = reinterpret_cast<float*>(base + in_bytes);
  uint32_t* d_prim = reinterpret_cast<uint32_t*>(base + in_bytes + (size_t)count * 4);
  float* d_uv = reinterpret_cast<float*>(base + in_bytes + (size_t)count * 8);
  const hipStream_t stream = pass.stream;
  HIP_TRY(hipMemcpyAsync(d_rays, rays, in_bytes, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
  if ((rc = formats_wait(s)) != RAYCA_OK) return rc;
  const TravPlan tp = plan_traversal(s, ordered, 0);
  const StackPlan sp = tp.stack;
  const size_t lds_bytes = sp.lds_bytes;
  TraceKernel k = pick_trace_kernel(tp.trav, s->host.sphere_count != 0, stats);
  const uint32_t tgrid = (count + kBlock - 1) / kBlock;
  TraceLaunch tl{};
  if ((rc = bind_stack(c, sp, tgrid, tl)) != RAYCA_OK) return rc;
  HIP_TRY(hipEventRecord(c->ev_begin, stream));
  hipLaunchKernelGGL(k, dim3(tgrid), dim3(kBlock), lds_bytes, stream, s->dev_full, d_rays, count, d_t, d_prim, d_uv, c->counters, tl);
  HIP_TRY(hipGetLastError());
  if ((rc = pass_retire(pass)) != RAYCA_OK) return rc;   // (the copies below need no event: the call drains the stream itself)
  HIP_TRY(hipMemcpyAsync(t_out, d_t, (size_t)count * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(prim_out, d_prim, (size_t)count * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(uv_out, d_uv, (size_t)count * 8, hipMemcpyDeviceToHost, stream));
  if ((rc = pass_finish(pass, 1, nullptr)) != RAYCA_OK) return rc;
  if (stats_out) {   // (its own few fields, none per kernel class)
    TraceCounters tc{};
    HIP_TRY(hipMemcpy(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost));
    std::memset(stats_out, 0, sizeof *stats_out);
    stats_out->rays_primary = count;
    stats_out->boxes_tested = tc.boxes;
    stats_out->triangles_tested = tc.tris;
    HIP_TRY(hipEventElapsedTime(&stats_out->kernel_ms, c->ev_begin, c->ev_end));
    stats_out->trace_kernel_ms = stats_out->kernel_ms;
    stats_out->kernel_launches = stats_out->trace_kernel_launches = 1;
  }
  return RAYCA_OK;
}

// Ray queries on device memory.  A RAYCA_BUILDER_SAH scene whose node formats are there runs the lane-refill kernel
// (refill.hip k_query_refill, on the 4-wide fp16 nodes k_queue_refill traverses); a RAYCA_BUILDER_REFERENCE scene, exhaustive
// traversal and a SAH scene whose formats thread has not finished (RaycaStats.node_format bit 11) run k_query_rays, one ray
// per lane on the binary f32 nodes.  Same results on every path.  A pass on its context (ContextPass), which clears the work
// counters on the launch stream.
int32_t rayca_hip_query_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaQuery* qin, RaycaStats* stats_out) {
  if (!s || !qin) return fail(RAYCA_ERR_BAD_ARG, "null scene or query");
  const RaycaQuery& rq = *qin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (rq.kind != RAYCA_QUERY_CLOSEST && rq.kind != RAYCA_QUERY_OCCLUDED) return fail(RAYCA_ERR_BAD_ARG, "unknown query kind");
  if (rq.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaQuery.reserved must be zero");
  if (!rq.rays) return fail(RAYCA_ERR_BAD_ARG, "null rays");
  const bool occluded = rq.kind == RAYCA_QUERY_OCCLUDED;
  if (occluded ? !rq.occluded_out : (!rq.t_out && !rq.prim_out && !rq.uv_out)) return fail(RAYCA_ERR_BAD_ARG, "no output for this kind of query");
  int32_t rc = pass_options(o, "a query", kOptTraversal | kOptCollectStats);
  if (rc != RAYCA_OK) return rc;
  const bool ordered = o.traversal != RAYCA_TRAVERSAL_EXHAUSTIVE;
  if (occluded && !ordered) return fail(RAYCA_ERR_UNSUPPORTED, "an occlusion query ends at its first hit: there is no exhaustive form");
  if ((rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  if (rq.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  FrameCtx* c = &s->ctx[o.context];
  std::lock_guard<std::mutex> lock(c->mu);
  ContextPass pass{};
  if ((rc = pass_acquire(s, o, stats_out != nullptr, pass)) != RAYCA_OK) return rc;
  const hipStream_t stream = pass.stream;
  const bool stats = o.collect_stats != 0, timing = pass.timing, sph = s->host.sphere_count != 0;
  const bool fast = s->dev.ref_leaf_of != nullptr;   // the reference-leaf filter is present (RAYCA_BUILDER_SAH)
  const bool all_formats = formats_ready(s);
  const bool refill = ordered && fast && all_formats;
  QueryIo q{};
  q.rays = static_cast<const float*>(rq.rays);
  q.tmax = static_cast<const float*>(rq.tmax);
  q.tmax_all = rq.tmax_all;
  q.count = rq.count;
  if (occluded) {
    q.occluded_out = static_cast<uint8_t*>(rq.occluded_out);
  } else {
    q.t_out = static_cast<float*>(rq.t_out);
    q.prim_out = static_cast<uint32_t*>(rq.prim_out);
    q.uv_out = static_cast<float*>(rq.uv_out);
  }
  const uint32_t batches = (rq.count + 63u) / 64u;
  uint32_t grid = (batches + 3u) / 4u;   // one ray per lane; the persistent grid below replaces it
  StackPlan sp{};
  QueryKernel k = nullptr;
  uint32_t node_format = all_formats ? 0u : 2048u;
  if (refill) {
    sp = plan_stack(std::max(s->host.max_depth, s->host.max_depth4), RAYCA_WF_LDS_ENTRIES);   // (as the wavefront engine plans k_queue_refill's)
    const uint32_t in_flight = frames_in_flight_hint(s, o.context, o.stream != nullptr);
    if ((rc = persistent_grid(s, query_refill_kernel(occluded, sph, stats), sp.lds_bytes, batches, true, in_flight, 0u, grid)) != RAYCA_OK) return rc;
    node_format |= (RAYCA_WF_BOUNCE_WIDE ? 1u : 0u) | (RAYCA_WF_BOUNCE_HALF ? 4u : 0u);
  } else {
    const Trav trav = !ordered ? (fast ? kTravFastAll : kTravExactAll) : (fast ? kTravFastSpill : kTravExact);
    sp = plan_stack(s->host.max_depth);
    k = pick_query_kernel(trav, sph, stats, occluded);
    if (fast && RAYCA_NODE_CH && RAYCA_NODE_CH48 && s->dev.nodes_ch) node_format |= 4096u;
  }
  TraceLaunch tl{};
  if ((rc = bind_stack(c, sp, grid, tl)) != RAYCA_OK) return rc;
  if (timing || stats) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
  if (refill) {
    tl.ticket = 1u;
    HIP_TRY(hipMemsetAsync(c->heads, 0, 8 * kHeadStride * sizeof(uint32_t), stream));
    c->heads_clean &= ~FrameCtx::kCleanHeads;   // the next frame of this context clears them for itself
  }
  if (pass.timing) HIP_TRY(hipEventRecord(c->ev_begin, stream));
  if (refill) launch_query_refill(occluded, sph, stats, grid, sp.lds_bytes, stream, s->dev_full, q, c->heads, c->counters, tl);
  else hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), sp.lds_bytes, stream, all_formats ? s->dev_full : s->dev, q, c->counters, tl);
  HIP_TRY(hipGetLastError());
  if ((rc = pass_retire(pass)) != RAYCA_OK || (rc = pass_finish(pass, 1, stats_out)) != RAYCA_OK || !timing) return rc;
  TraceCounters tc{};
  if (stats) HIP_TRY(hipMemcpy(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost));
  (occluded ? stats_out->rays_shadow : stats_out->rays_primary) = rq.count;
  stats_out->boxes_tested = tc.boxes;
  stats_out->triangles_tested = tc.tris;
  stats_out->wave_box_slots = tc.box_slots;
  stats_out->wave_triangle_slots = tc.tri_slots;
  stats_out->trace_kernel_ms = stats_out->kernel_ms;
  stats_out->trace_kernel_launches = 1;
  stats_out->node_format = node_format;
  return RAYCA_OK;
}

// Nearest-point queries (nearest.inc k_nearest): one point per lane on the binary f32 nodes, which every scene has from
// scene_create on, so the call never waits for the formats thread.  A pass on its context (run_pass), which clears the work
// counters on the launch stream when they are read.
int32_t rayca_hip_nearest_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaNearest* nin, RaycaStats* stats_out) {
  if (!s || !nin) return fail(RAYCA_ERR_BAD_ARG, "null scene or RaycaNearest");
  const RaycaNearest& rn = *nin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if (!rn.points) return fail(RAYCA_ERR_BAD_ARG, "RaycaNearest.points: null points");
  if (rn.kind != RAYCA_NEAREST_CLOSEST && rn.kind != RAYCA_NEAREST_WITHIN) return fail(RAYCA_ERR_BAD_ARG, "RaycaNearest.kind: unknown kind");
  if (rn.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaNearest.reserved must be zero");
  const bool within = rn.kind == RAYCA_NEAREST_WITHIN;
  if (within ? !rn.within_out : (!rn.dist2_out && !rn.prim_out && !rn.point_out && !rn.uv_out))
    return fail(RAYCA_ERR_BAD_ARG, "no output for this kind of nearest-point query");
  int32_t rc = pass_options(o, "a nearest-point query", kOptTraversal | kOptCollectStats);
  if (rc != RAYCA_OK) return rc;
  const bool cull = o.traversal != RAYCA_TRAVERSAL_EXHAUSTIVE;
  if (within && !cull) return fail(RAYCA_ERR_UNSUPPORTED, "RaycaRenderOptions.traversal: RAYCA_NEAREST_WITHIN ends at its first candidate: there is no exhaustive form");
  if (rn.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if ((rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  if (s->host.sphere_count != 0)
    return fail(RAYCA_ERR_UNSUPPORTED, "a scene with spheres has no nearest-point query: a sphere under a non-uniform scale is an ellipsoid, whose nearest point has no closed form");
  NearestIo io{};
  io.points = static_cast<const float*>(rn.points);
  io.radius = static_cast<const float*>(rn.radius);
  io.radius_all = rn.radius_all;
  io.count = rn.count;
  if (within) {
    io.within_out = static_cast<uint8_t*>(rn.within_out);
  } else {
    io.dist2_out = static_cast<float*>(rn.dist2_out);
    io.prim_out = static_cast<uint32_t*>(rn.prim_out);
    io.point_out = static_cast<float*>(rn.point_out);
    io.uv_out = static_cast<float*>(rn.uv_out);
  }
  const bool stats = o.collect_stats != 0;
  const StackPlan sp = plan_stack(s->host.max_depth);   // (as k_query_rays is launched: one pending sibling per level)
  const uint32_t grid = (uint32_t)(((uint64_t)rn.count + kBlock - 1u) / kBlock);
  FrameCtx* c = &s->ctx[o.context];
  TraceCounters tc{};
  rc = run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) -> int32_t {
    TraceLaunch tl{};
    if (const int32_t brc = bind_stack(c, sp, grid, tl); brc != RAYCA_OK) return brc;
    if (stats) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
    hipLaunchKernelGGL(pick_nearest_kernel(within, cull, sp.spill_entries != 0, stats), dim3(grid), dim3(kBlock), sp.lds_bytes, stream,
                       formats_ready(s) ? s->dev_full : s->dev, io, c->counters, tl);
    HIP_TRY(hipGetLastError());
    ++launches;
    // (read back inside the pass, under the context's lock: with stats_out the pass waits for the stream before it returns)
    if (stats && stats_out) HIP_TRY(hipMemcpyAsync(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost, stream));
    return RAYCA_OK;
  });
  if (rc != RAYCA_OK || !stats_out || !stats) return rc;
  stats_out->boxes_tested = tc.boxes;
  stats_out->triangles_tested = tc.tris;
  return RAYCA_OK;
}

// What a surface-sampling call refuses of a scene, behind everything its structs decide: nothing to sample, or spheres.
int32_t refuse_unsampled_scene(const RaycaScene* s) {
  if (const int32_t rc = refuse_empty_scene(s); rc != RAYCA_OK) return rc;
  if (s->host.sphere_count != 0)
    return fail(RAYCA_ERR_UNSUPPORTED, "a scene with spheres has no surface sampling: the table weighs triangle slots, and the area of a sphere under a non-uniform scale has no closed form");
  return RAYCA_OK;
}

// The cumulative area table of a scene's slots (sample.inc): k_cdf_amax -> k_cdf_weights -> k_cdf_scan (one block), each behind
// the other on the pass's stream.  The one scratch word -- the largest area's bits -- is the first of the context's plan_sums,
// cleared on the launch stream in front of the first kernel.  Only the primitive records are read, which every scene has from
// scene_create on, so the call never waits for the formats thread.
int32_t rayca_hip_surface_cdf_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaSurfaceCdf* cin, RaycaStats* stats_out) {
  if (!s || !cin) return fail(RAYCA_ERR_BAD_ARG, "null scene or RaycaSurfaceCdf");
  const RaycaSurfaceCdf& a = *cin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if (a.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceCdf.reserved must be zero");
  if (a.flags != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceCdf.flags must be zero");
  if (!a.cdf_out) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceCdf.cdf_out: null cdf_out");
  if (reinterpret_cast<uintptr_t>(a.cdf_out) & 7u) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceCdf.cdf_out: alignment: the table is written 8 bytes an entry");
  int32_t rc = pass_options(o, "a surface-table call", kOptCollectStats);
  if (rc != RAYCA_OK) return rc;
  if ((rc = refuse_unsampled_scene(s)) != RAYCA_OK) return rc;
  SurfaceCdfIo io{};
  io.include = static_cast<const uint8_t*>(a.include);
  io.cdf = static_cast<unsigned long long*>(a.cdf_out);
  const uint32_t slots = s->prim_count, grid = (slots + kBlock - 1u) / kBlock;   // (slots <= 2^25)
  return run_pass(
      s, o, stats_out,
      [&](FrameCtx* c) -> int32_t {
        HIP_TRY(hipSetDevice(s->device));
        return grow_behind_pass(c, c->plan_sums, sizeof(uint32_t));
      },
      [&](hipStream_t stream, uint32_t& launches) -> int32_t {
        io.amax = static_cast<uint32_t*>(s->ctx[o.context].plan_sums.ptr);
        const DevScene& dev = formats_ready(s) ? s->dev_full : s->dev;
        HIP_TRY(hipMemsetAsync(io.amax, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(k_cdf_amax, dim3(grid), dim3(kBlock), 0, stream, dev, io);
        HIP_TRY(hipGetLastError());
        ++launches;
        hipLaunchKernelGGL(k_cdf_weights, dim3(grid), dim3(kBlock), 0, stream, dev, io);
        HIP_TRY(hipGetLastError());
        ++launches;
        hipLaunchKernelGGL(k_cdf_scan, dim3(1), dim3(kCdfScanBlock), 0, stream, io.cdf + 1, slots);
        HIP_TRY(hipGetLastError());
        ++launches;
        return RAYCA_OK;
      });
}

// Samples drawn from such a table (sample.inc k_sample_surface): one sample per lane, one launch, no scratch.
int32_t rayca_hip_surface_sample_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaSurfaceSample* sin, RaycaStats* stats_out) {
  if (!s || !sin) return fail(RAYCA_ERR_BAD_ARG, "null scene or RaycaSurfaceSample");
  const RaycaSurfaceSample& a = *sin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if (a.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceSample.reserved must be zero");
  if (!a.cdf) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceSample.cdf: null cdf");
  if (reinterpret_cast<uintptr_t>(a.cdf) & 7u) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceSample.cdf: alignment: the table is read 8 bytes an entry");
  if (!a.prim_out && !a.uv_out && !a.point_out && !a.normal_out)
    return fail(RAYCA_ERR_BAD_ARG, "no output for this surface-sampling call: RaycaSurfaceSample.prim_out, uv_out, point_out and normal_out are all null");
  int32_t rc = pass_options(o, "a surface-sampling call", kOptCollectStats);
  if (rc != RAYCA_OK) return rc;
  if (a.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if ((rc = refuse_unsampled_scene(s)) != RAYCA_OK) return rc;
  SurfaceSampleIo io{};
  io.cdf = static_cast<const unsigned long long*>(a.cdf);
  io.count = a.count;
  io.seed = a.seed;
  io.sample = a.sample;
  io.first_index = a.first_index;
  io.prim_out = static_cast<uint32_t*>(a.prim_out);
  io.uv_out = static_cast<float*>(a.uv_out);
  io.point_out = static_cast<float*>(a.point_out);
  io.normal_out = static_cast<float*>(a.normal_out);
  const uint32_t grid = (uint32_t)(((uint64_t)a.count + kBlock - 1u) / kBlock);
  return run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) -> int32_t {
    hipLaunchKernelGGL(pick_sample_kernel(io.point_out || io.normal_out), dim3(grid), dim3(kBlock), 0, stream,
                       formats_ready(s) ? s->dev_full : s->dev, io);
    HIP_TRY(hipGetLastError());
    ++launches;
    return RAYCA_OK;
  });
}

// What RaycaHits alone decides, in the header's order; the first rule broken is the one reported.  No scene, no device.
int32_t check_hits(const RaycaHits& rh) {
  if (!rh.rays) return fail(RAYCA_ERR_BAD_ARG, "RaycaHits.rays: null rays");
  if (rh.k > RAYCA_HITS_MAX) return fail(RAYCA_ERR_BAD_ARG, "RaycaHits.k: more than RAYCA_HITS_MAX hits per ray");
  if (rh.faces != RAYCA_HITS_FRONT && rh.faces != RAYCA_HITS_BOTH) return fail(RAYCA_ERR_BAD_ARG, "RaycaHits.faces: unknown faces");
  if (rh.count_all > 1u) return fail(RAYCA_ERR_BAD_ARG, "RaycaHits.count_all must be 0 or 1");
  if (rh.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaHits.reserved must be zero");
  if (rh.k == 0 && !rh.count_all) return fail(RAYCA_ERR_BAD_ARG, "RaycaHits.k: k == 0 needs count_all");
  const bool records = rh.t_out || rh.prim_out || rh.uv_out || rh.face_out;
  if (!records && !rh.n_out) return fail(RAYCA_ERR_BAD_ARG, "no output for this multi-hit query");
  if (rh.k == 0 && records) return fail(RAYCA_ERR_BAD_ARG, "no output for this multi-hit query: k == 0 writes n_out alone, a record output has no entries");
  return RAYCA_OK;
}

// Multi-hit ray queries (hits.inc k_hits): one ray per lane on the binary f32 nodes, which every scene has from scene_create on,
// so the call never waits for the formats thread.  The kernel's LDS is the node stack's part and the lists' 2 k rows behind it
// (hits_lds_bytes).  A pass on its context (run_pass), which clears the work counters on the launch stream when they are read.
int32_t rayca_hip_hits_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaHits* hin, RaycaStats* stats_out) {
  if (!s || !hin) return fail(RAYCA_ERR_BAD_ARG, "null scene or RaycaHits");
  const RaycaHits& rh = *hin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  int32_t rc = check_hits(rh);
  if (rc != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a multi-hit query", kOptTraversal | kOptCollectStats)) != RAYCA_OK) return rc;
  if (rh.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if ((rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  HitsIo io{};
  io.rays = static_cast<const float*>(rh.rays);
  io.tmax = static_cast<const float*>(rh.tmax);
  io.tmax_all = rh.tmax_all;
  io.count = rh.count;
  io.k = rh.k;
  io.t_out = static_cast<float*>(rh.t_out);
  io.prim_out = static_cast<uint32_t*>(rh.prim_out);
  io.uv_out = static_cast<float*>(rh.uv_out);
  io.face_out = static_cast<uint8_t*>(rh.face_out);
  io.n_out = static_cast<uint32_t*>(rh.n_out);
  const bool stats = o.collect_stats != 0, ordered = o.traversal != RAYCA_TRAVERSAL_EXHAUSTIVE;
  const bool fast = s->dev.ref_leaf_of != nullptr;   // the reference-leaf filter is present (RAYCA_BUILDER_SAH)
  const Trav trav = !ordered ? (fast ? kTravFastAll : kTravExactAll) : (fast ? kTravFastSpill : kTravExact);   // (as k_query_rays is chosen)
  const StackPlan sp = plan_stack(s->host.max_depth);
  const uint32_t grid = (uint32_t)(((uint64_t)rh.count + kBlock - 1u) / kBlock);
  FrameCtx* c = &s->ctx[o.context];
  TraceCounters tc{};
  rc = run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) -> int32_t {
    TraceLaunch tl{};
    if (const int32_t brc = bind_stack(c, sp, grid, tl); brc != RAYCA_OK) return brc;
    if (stats) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
    hipLaunchKernelGGL(pick_hits_kernel(trav, s->host.sphere_count != 0, stats, rh.faces == RAYCA_HITS_BOTH, rh.count_all != 0), dim3(grid), dim3(kBlock),
                       hits_lds_bytes(sp, rh.k), stream, formats_ready(s) ? s->dev_full : s->dev, io, c->counters, tl);
    HIP_TRY(hipGetLastError());
    ++launches;
    // (read back inside the pass, under the context's lock: with stats_out the pass waits for the stream before it returns)
    if (stats && stats_out) HIP_TRY(hipMemcpyAsync(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost, stream));
    return RAYCA_OK;
  });
  if (rc != RAYCA_OK || !stats_out) return rc;
  stats_out->rays_primary = rh.count;
  if (stats) {
    stats_out->boxes_tested = tc.boxes;
    stats_out->triangles_tested = tc.tris;
  }
  return RAYCA_OK;
}

// What RaycaSigned alone decides, in the header's order; the first rule broken is the one reported.  No scene, no device.
int32_t check_signed(const RaycaSigned& rs) {
  if (rs.source != RAYCA_SIGNED_POINTS && rs.source != RAYCA_SIGNED_GRID) return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.source: unknown source");
  if (rs.source == RAYCA_SIGNED_POINTS && !rs.points) return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.points: null points");
  if (rs.source == RAYCA_SIGNED_GRID) {
    if (rs.grid_dims[0] == 0 || rs.grid_dims[1] == 0 || rs.grid_dims[2] == 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.grid_dims: a dimension is zero");
    const uint64_t plane = (uint64_t)rs.grid_dims[0] * rs.grid_dims[1];   // (< 2^64; the second product is checked by division)
    if (plane > 0xFFFFFFFFull || plane * rs.grid_dims[2] != (uint64_t)rs.count)
      return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.grid_dims: nx * ny * nz must equal count (at most 2^32 - 1 points)");
  }
  if (rs.rule != RAYCA_SIGNED_PARITY && rs.rule != RAYCA_SIGNED_WINDING) return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.rule: unknown rule");
  if (rs.n_dirs != 1u && rs.n_dirs != 3u && rs.n_dirs != 5u) return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.n_dirs: 1, 3 or 5 directions");
  for (uint32_t j = 0; j < rs.n_dirs; ++j)
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(rs.dirs[j][a]) || rs.dirs[j][a] == 0.0f)
        return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.dirs: a component of a used direction is zero, NaN or infinite (an axis-aligned ray has no hits)");
  if (rs.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaSigned.reserved must be zero");
  if (!rs.inside_out && !rs.votes_out && !rs.cross_out)
    return fail(RAYCA_ERR_BAD_ARG, "no sign output for a signed query: without inside_out, votes_out and cross_out this is a nearest-point query");
  return RAYCA_OK;
}

// Signed distance and occupancy (signed.inc k_signed): one point per lane on the binary f32 nodes, which every scene has from
// scene_create on, so the call never waits for the formats thread.  One launch: the nearest search where a distance output is
// asked for, then a crossing-count ray per direction.  A pass on its context (run_pass), which clears the work counters on the
// launch stream when they are read.
int32_t rayca_hip_signed_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaSigned* sin, RaycaStats* stats_out) {
  if (!s || !sin) return fail(RAYCA_ERR_BAD_ARG, "null scene or RaycaSigned");
  const RaycaSigned& rs = *sin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  int32_t rc = check_signed(rs);
  if (rc != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a signed query", kOptTraversal | kOptCollectStats)) != RAYCA_OK) return rc;
  if (rs.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if ((rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  if (s->host.sphere_count != 0)
    return fail(RAYCA_ERR_UNSUPPORTED, "a scene with spheres has no signed query: its distance part is a nearest-point query, which has no closed form on an ellipsoid");
  const bool grid_source = rs.source == RAYCA_SIGNED_GRID;
  SignedIo io{};
  io.points = grid_source ? nullptr : static_cast<const float*>(rs.points);
  io.radius = static_cast<const float*>(rs.radius);
  io.radius_all = rs.radius_all;
  io.count = rs.count;
  for (int a = 0; a < 3; ++a) {
    io.grid_origin[a] = rs.grid_origin[a];
    io.grid_step[a] = rs.grid_step[a];
    io.grid_dims[a] = grid_source ? rs.grid_dims[a] : 1u;
  }
  io.rule = rs.rule;
  io.n_dirs = rs.n_dirs;
  std::memcpy(io.dirs, rs.dirs, sizeof io.dirs);
  io.dist2_out = static_cast<float*>(rs.dist2_out);
  io.prim_out = static_cast<uint32_t*>(rs.prim_out);
  io.point_out = static_cast<float*>(rs.point_out);
  io.uv_out = static_cast<float*>(rs.uv_out);
  io.inside_out = static_cast<uint8_t*>(rs.inside_out);
  io.votes_out = static_cast<uint8_t*>(rs.votes_out);
  io.cross_out = static_cast<uint32_t*>(rs.cross_out);
  const bool near = io.dist2_out || io.prim_out || io.point_out || io.uv_out;
  const bool stats = o.collect_stats != 0, cull = o.traversal != RAYCA_TRAVERSAL_EXHAUSTIVE;
  const bool fast = s->dev.ref_leaf_of != nullptr;   // the reference-leaf filter is present (RAYCA_BUILDER_SAH)
  const StackPlan sp = plan_stack(s->host.max_depth);   // (one pending sibling per level in either phase)
  const uint32_t grid = (uint32_t)(((uint64_t)rs.count + kBlock - 1u) / kBlock);
  FrameCtx* c = &s->ctx[o.context];
  TraceCounters tc{};
  rc = run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) -> int32_t {
    TraceLaunch tl{};
    if (const int32_t brc = bind_stack(c, sp, grid, tl); brc != RAYCA_OK) return brc;
    if (stats) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
    hipLaunchKernelGGL(pick_signed_kernel(near, cull, grid_source, fast, stats), dim3(grid), dim3(kBlock), sp.lds_bytes, stream,
                       formats_ready(s) ? s->dev_full : s->dev, io, c->counters, tl);
    HIP_TRY(hipGetLastError());
    ++launches;
    // (read back inside the pass, under the context's lock: with stats_out the pass waits for the stream before it returns)
    if (stats && stats_out) HIP_TRY(hipMemcpyAsync(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost, stream));
    return RAYCA_OK;
  });
  if (rc != RAYCA_OK || !stats_out) return rc;
  stats_out->rays_primary = (uint64_t)rs.count * rs.n_dirs;
  if (stats) {
    stats_out->boxes_tested = tc.boxes;
    stats_out->triangles_tested = tc.tris;
  }
  return RAYCA_OK;
}

// Hemisphere visibility at points (ambient.inc, refill.hip k_ambient_refill): count x samples occlusion rays made in registers, one
// mask word per point, folded by k_ambient_finish.  The trace kernel is chosen as rayca_hip_query_device chooses an OCCLUDED query's:
// the lane-refill form on the 4-wide fp16 nodes for a RAYCA_BUILDER_SAH scene whose formats are there, else one ray per lane on
// the binary f32 nodes.  The mask words live in mask_out, or in the context's scratch (grown before the pass queues its waits);
// they are cleared on the launch stream in front of the trace kernel.  A pass on its context (run_pass).
int32_t rayca_hip_ambient_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaAmbient* ain, RaycaStats* stats_out) {
  if (!s || !ain) return fail(RAYCA_ERR_BAD_ARG, "null scene or RaycaAmbient");
  const RaycaAmbient& ra = *ain;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if (!ra.points) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.points: null points");
  if (!ra.normals) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.normals: null normals");
  if (!ra.dirs) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.dirs: null dirs");
  if (ra.samples == 0 || ra.samples > 64) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.samples: 1 .. 64 samples (one bit of the mask word each)");
  if (ra.dir_first > ra.dir_count || ra.samples > ra.dir_count - ra.dir_first)
    return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.dir_first + samples exceeds dir_count");
  if (ra.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.reserved must be zero");
  if (!ra.mask_out && !ra.hits_out && !ra.open_out && !ra.bent_out) return fail(RAYCA_ERR_BAD_ARG, "no output for an ambient call");
  if (reinterpret_cast<uintptr_t>(ra.mask_out) % 8u != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.mask_out must be aligned to 8 bytes");
  if (!std::isfinite(ra.bias)) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.bias is not finite");
  if ((uint64_t)ra.count * ra.samples >= (1ull << 32)) return fail(RAYCA_ERR_BAD_ARG, "RaycaAmbient.count x samples must stay below 2^32");
  int32_t rc = pass_options(o, "an ambient call", kOptTraversal | kOptCollectStats);
  if (rc != RAYCA_OK) return rc;
  if (o.traversal == RAYCA_TRAVERSAL_EXHAUSTIVE)
    return fail(RAYCA_ERR_UNSUPPORTED, "RaycaRenderOptions.traversal: an occlusion ray ends at its first hit: there is no exhaustive form");
  if (ra.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if ((rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  AmbientIo io{};
  io.points = static_cast<const float*>(ra.points);
  io.normals = static_cast<const float*>(ra.normals);
  io.rotations = static_cast<const float*>(ra.rotations);
  io.radius = static_cast<const float*>(ra.radius);
  io.dirs = static_cast<const float*>(ra.dirs) + 3ull * ra.dir_first;
  io.radius_all = ra.radius_all;
  io.bias = ra.bias;
  io.count = ra.count;
  io.samples = ra.samples;
  io.mask_out = static_cast<unsigned long long*>(ra.mask_out);
  io.hits_out = static_cast<uint32_t*>(ra.hits_out);
  io.open_out = static_cast<float*>(ra.open_out);
  io.bent_out = static_cast<float*>(ra.bent_out);
  const bool stats = o.collect_stats != 0, sph = s->host.sphere_count != 0, rot = ra.rotations != nullptr, bent = ra.bent_out != nullptr;
  const bool fold = ra.hits_out || ra.open_out || bent;   // (mask_out alone is the trace kernel's own work)
  const uint32_t total = ra.count * ra.samples, batches = (total + 63u) / 64u;
  const size_t mask_bytes = (size_t)ra.count * sizeof(unsigned long long);
  FrameCtx* c = &s->ctx[o.context];
  TraceCounters tc{};
  uint32_t node_format = 0;
  rc = run_pass(
      s, o, stats_out,
      [&](FrameCtx* ctx) -> int32_t {
        if (io.mask_out) return RAYCA_OK;
        HIP_TRY(hipSetDevice(s->device));
        return grow_behind_pass(ctx, ctx->ambient_mask, mask_bytes);
      },
      [&](hipStream_t stream, uint32_t& launches) -> int32_t {
        io.mask = io.mask_out ? io.mask_out : static_cast<unsigned long long*>(c->ambient_mask.ptr);
        const bool fast = s->dev.ref_leaf_of != nullptr;   // the reference-leaf filter is present (RAYCA_BUILDER_SAH)
        const bool all_formats = formats_ready(s);
        const bool refill = fast && all_formats;           // (rayca_hip_query_device's rule for an ordered query)
        uint32_t grid = (batches + 3u) / 4u;               // one ray per lane; the persistent grid below replaces it
        StackPlan sp{};
        node_format = all_formats ? 0u : 2048u;
        if (refill) {
          sp = plan_stack(std::max(s->host.max_depth, s->host.max_depth4), RAYCA_WF_LDS_ENTRIES);
          const uint32_t in_flight = frames_in_flight_hint(s, o.context, o.stream != nullptr);
          if (const int32_t grc = persistent_grid(s, ambient_refill_kernel(rot, sph, stats), sp.lds_bytes, batches, true, in_flight, 0u, grid); grc != RAYCA_OK) return grc;
          node_format |= (RAYCA_WF_BOUNCE_WIDE ? 1u : 0u) | (RAYCA_WF_BOUNCE_HALF ? 4u : 0u);
        } else {
          sp = plan_stack(s->host.max_depth);
          if (fast && RAYCA_NODE_CH && RAYCA_NODE_CH48 && s->dev.nodes_ch) node_format |= 4096u;
        }
        TraceLaunch tl{};
        if (const int32_t brc = bind_stack(c, sp, grid, tl); brc != RAYCA_OK) return brc;
        if (stats) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
        HIP_TRY(hipMemsetAsync(io.mask, 0, mask_bytes, stream));
        if (refill) {
          tl.ticket = 1u;
          HIP_TRY(hipMemsetAsync(c->heads, 0, 8 * kHeadStride * sizeof(uint32_t), stream));
          c->heads_clean &= ~FrameCtx::kCleanHeads;   // the next frame of this context clears them for itself
          launch_ambient_refill(rot, sph, stats, grid, sp.lds_bytes, stream, s->dev_full, io, c->heads, c->counters, tl);
        } else {
          hipLaunchKernelGGL(pick_ambient_kernel(fast, sph, stats, rot), dim3(grid), dim3(kBlock), sp.lds_bytes, stream, all_formats ? s->dev_full : s->dev, io,
                             c->counters, tl);
        }
        HIP_TRY(hipGetLastError());
        ++launches;
        if (fold) {
          hipLaunchKernelGGL(pick_ambient_finish(bent, rot), dim3((ra.count + kBlock - 1u) / kBlock), dim3(kBlock), 0, stream, io);
          HIP_TRY(hipGetLastError());
          ++launches;
        }
        // (read back inside the pass, under the context's lock: with stats_out the pass waits for the stream before it returns)
        if (stats && stats_out) HIP_TRY(hipMemcpyAsync(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost, stream));
        return RAYCA_OK;
      });
  if (rc != RAYCA_OK || !stats_out) return rc;
  stats_out->rays_shadow = total;
  stats_out->boxes_tested = tc.boxes;
  stats_out->triangles_tested = tc.tris;
  stats_out->wave_box_slots = tc.box_slots;
  stats_out->wave_triangle_slots = tc.tri_slots;
  stats_out->node_format = node_format;
  return RAYCA_OK;
}

// Irradiance volumes (probes.inc, refill.hip k_probe_refill): with RAYCA_PROBE_VISIBILITY count x 8 occlusion rays made in registers,
// one mask word per point, then k_probe_fold; without it the fold alone, and the scene is not read.  The trace kernel is chosen
// exactly as rayca_hip_ambient_device chooses its own.  The mask words live in mask_out, or in the context's scratch (grown before
// the pass queues its waits); they are cleared on the launch stream in front of the trace kernel.  A pass on its context (run_pass).
int32_t rayca_hip_probe_lookup_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaProbeLookup* pin, RaycaStats* stats_out) {
  if (!s || !pin) return fail(RAYCA_ERR_BAD_ARG, "null scene or RaycaProbeLookup");
  const RaycaProbeLookup& rp = *pin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if (!rp.points) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.points: null points");
  if (!rp.normals) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.normals: null normals");
  if (!rp.sh) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.sh: null sh");
  if (rp.flags & ~(uint32_t)(RAYCA_PROBE_VISIBILITY | RAYCA_PROBE_NORMAL_TERM)) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.flags: unknown flag bits");
  if (rp.dims[0] == 0 || rp.dims[1] == 0 || rp.dims[2] == 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.dims: a zero dim (each axis has at least one probe)");
  if ((uint64_t)rp.dims[0] * rp.dims[1] > (1ull << 24) || (uint64_t)rp.dims[0] * rp.dims[1] * rp.dims[2] > (1ull << 24))
    return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.dims: more than 2^24 probes");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(rp.cell[a]) || !(rp.cell[a] > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.cell is not finite and > 0");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(rp.origin[a])) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.origin is not finite");
  if (!std::isfinite(rp.bias)) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.bias is not finite");
  if (rp.reserved[0] != 0 || rp.reserved[1] != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.reserved must be zero");
  if (!rp.irradiance_out && !rp.sh_out && !rp.mask_out && !rp.radiance_out) return fail(RAYCA_ERR_BAD_ARG, "no output for a probe lookup");
  if (rp.radiance_out && !rp.albedo) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.radiance_out needs albedo");
  const struct { const void* p; const char* name; } aligned[] = {{rp.irradiance_out, "irradiance_out"}, {rp.sh_out, "sh_out"}, {rp.radiance_out, "radiance_out"},
                                                                 {rp.albedo, "albedo"}, {rp.base, "base"}, {rp.sh, "sh"}};
  for (const auto& a : aligned)
    if (reinterpret_cast<uintptr_t>(a.p) & 15u) return fail(RAYCA_ERR_BAD_ARG, std::string("RaycaProbeLookup.") + a.name + " must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(rp.mask_out) & 3u) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.mask_out must be 4-byte aligned");
  if ((uint64_t)rp.count * 8u >= (1ull << 32)) return fail(RAYCA_ERR_BAD_ARG, "RaycaProbeLookup.count x 8 must stay below 2^32");
  int32_t rc = pass_options(o, "a probe lookup", kOptTraversal | kOptCollectStats);
  if (rc != RAYCA_OK) return rc;
  if (o.traversal == RAYCA_TRAVERSAL_EXHAUSTIVE)
    return fail(RAYCA_ERR_UNSUPPORTED, "RaycaRenderOptions.traversal: an occlusion ray ends at its first hit: there is no exhaustive form");
  if (rp.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  const bool vis = (rp.flags & RAYCA_PROBE_VISIBILITY) != 0, normal = (rp.flags & RAYCA_PROBE_NORMAL_TERM) != 0;
  if (vis && (rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  ProbeIo io{};
  io.points = static_cast<const float*>(rp.points);
  io.normals = static_cast<const float*>(rp.normals);
  io.sh = static_cast<const float4*>(rp.sh);
  io.kept = static_cast<const uint32_t*>(rp.kept);
  io.albedo = static_cast<const float4*>(rp.albedo);
  io.base = static_cast<const float4*>(rp.base);
  for (int a = 0; a < 3; ++a) {
    io.origin[a] = rp.origin[a];
    io.cell[a] = rp.cell[a];
    io.dims[a] = rp.dims[a];
  }
  io.bias = rp.bias;
  io.count = rp.count;
  io.irradiance_out = static_cast<float4*>(rp.irradiance_out);
  io.sh_out = static_cast<float4*>(rp.sh_out);
  io.mask_out = static_cast<uint32_t*>(rp.mask_out);
  io.radiance_out = static_cast<float4*>(rp.radiance_out);
  const bool stats = o.collect_stats != 0;
  const uint32_t total = rp.count * 8u, batches = (total + 63u) / 64u;
  const size_t mask_bytes = (size_t)rp.count * sizeof(uint32_t);
  FrameCtx* c = &s->ctx[o.context];
  TraceCounters tc{};
  uint32_t node_format = 0;
  rc = run_pass(
      s, o, stats_out,
      [&](FrameCtx* ctx) -> int32_t {
        if (!vis || io.mask_out) return RAYCA_OK;
        HIP_TRY(hipSetDevice(s->device));
        return grow_behind_pass(ctx, ctx->probe_mask, mask_bytes);
      },
      [&](hipStream_t stream, uint32_t& launches) -> int32_t {
        if (vis) {
          const bool sph = s->host.sphere_count != 0;
          io.mask = io.mask_out ? io.mask_out : static_cast<uint32_t*>(c->probe_mask.ptr);
          const bool fast = s->dev.ref_leaf_of != nullptr;   // the reference-leaf filter is present (RAYCA_BUILDER_SAH)
          const bool all_formats = formats_ready(s);
          const bool refill = fast && all_formats;           // (rayca_hip_ambient_device's rule)
          uint32_t grid = (batches + 3u) / 4u;               // one ray per lane; the persistent grid below replaces it
          StackPlan sp{};
          node_format = all_formats ? 0u : 2048u;
          if (refill) {
            sp = plan_stack(std::max(s->host.max_depth, s->host.max_depth4), RAYCA_WF_LDS_ENTRIES);
            const uint32_t in_flight = frames_in_flight_hint(s, o.context, o.stream != nullptr);
            if (const int32_t grc = persistent_grid(s, probe_refill_kernel(sph, stats), sp.lds_bytes, batches, true, in_flight, 0u, grid); grc != RAYCA_OK) return grc;
            node_format |= (RAYCA_WF_BOUNCE_WIDE ? 1u : 0u) | (RAYCA_WF_BOUNCE_HALF ? 4u : 0u);
          } else {
            sp = plan_stack(s->host.max_depth);
            if (fast && RAYCA_NODE_CH && RAYCA_NODE_CH48 && s->dev.nodes_ch) node_format |= 4096u;
          }
          TraceLaunch tl{};
          if (const int32_t brc = bind_stack(c, sp, grid, tl); brc != RAYCA_OK) return brc;
          if (stats) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
          HIP_TRY(hipMemsetAsync(io.mask, 0, mask_bytes, stream));
          if (refill) {
            tl.ticket = 1u;
            HIP_TRY(hipMemsetAsync(c->heads, 0, 8 * kHeadStride * sizeof(uint32_t), stream));
            c->heads_clean &= ~FrameCtx::kCleanHeads;   // the next frame of this context clears them for itself
            launch_probe_refill(sph, stats, grid, sp.lds_bytes, stream, s->dev_full, io, c->heads, c->counters, tl);
          } else {
            hipLaunchKernelGGL(pick_probe_kernel(fast, sph, stats), dim3(grid), dim3(kBlock), sp.lds_bytes, stream, all_formats ? s->dev_full : s->dev, io, c->counters,
                               tl);
          }
          HIP_TRY(hipGetLastError());
          ++launches;
        }
        hipLaunchKernelGGL(pick_probe_fold(vis, normal, io.kept != nullptr), dim3((rp.count + kProbeFoldBlock - 1u) / kProbeFoldBlock), dim3(kProbeFoldBlock), 0, stream, io);
        HIP_TRY(hipGetLastError());
        ++launches;
        // (read back inside the pass, under the context's lock: with stats_out the pass waits for the stream before it returns)
        if (vis && stats && stats_out) HIP_TRY(hipMemcpyAsync(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost, stream));
        return RAYCA_OK;
      });
  if (rc != RAYCA_OK || !stats_out) return rc;
  stats_out->rays_shadow = vis ? total : 0u;
  stats_out->boxes_tested = tc.boxes;
  stats_out->triangles_tested = tc.tris;
  stats_out->wave_box_slots = tc.box_slots;
  stats_out->wave_triangle_slots = tc.tri_slots;
  stats_out->node_format = node_format;
  return RAYCA_OK;
}

// Direct light at points (direct.inc, refill.hip k_direct_refill): count x N shadow rays made in registers from the points and the
// scene's light records, one mask word per point, folded by k_direct_fold.  The trace kernel is chosen exactly as
// rayca_hip_ambient_device chooses its own.  The mask words live in mask_out, or in the context's scratch (grown before the pass
// queues its waits); they are cleared on the launch stream in front of the trace kernel.  A pass on its context (run_pass), so that
// a rayca_hip_scene_update of lights never overwrites a table these kernels are still reading.
int32_t rayca_hip_direct_device(RaycaScene* s, const RaycaConfig* cfg_in, const RaycaRenderOptions* opts_in, const RaycaDirect* din, RaycaStats* stats_out) {
  if (!s || !cfg_in || !din) return fail(RAYCA_ERR_BAD_ARG, "null scene, config or RaycaDirect");
  const RaycaDirect& rd = *din;
  const RaycaConfig& cfg = *cfg_in;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if (!rd.points) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.points: null points");
  if (rd.light_count == 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.light_count: a range of no lights");
  if (cfg.light_samples == 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaConfig.light_samples must be > 0");
  if ((uint64_t)rd.light_count * cfg.light_samples > 64u)
    return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.light_count x light_samples: 1 .. 64 samples (one bit of the mask word each); chunk over light ranges");
  if (rd.reserved[0] != 0 || rd.reserved[1] != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.reserved must be zero");
  if (!rd.irradiance_out && !rd.sh_out && !rd.mask_out && !rd.counts_out) return fail(RAYCA_ERR_BAD_ARG, "no output for a direct-light call");
  const bool sphere = rd.normals == nullptr;
  if (!sphere && rd.sh_out) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.sh_out is a sphere-mode output: not with normals");
  if (sphere && rd.bias != 0.0f) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.bias must be 0 without normals (sphere mode: o = p)");
  if (reinterpret_cast<uintptr_t>(rd.irradiance_out) & 15u) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.irradiance_out must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(rd.sh_out) & 15u) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.sh_out must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(rd.mask_out) & 7u) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.mask_out must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(rd.counts_out) & 3u) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.counts_out must be 4-byte aligned");
  if (!std::isfinite(rd.bias)) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.bias is not finite");
  if ((uint64_t)rd.first_index + rd.count > (1ull << 32)) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.first_index + count exceeds 2^32");
  const uint32_t samples = rd.light_count * cfg.light_samples;
  if ((uint64_t)rd.count * samples >= (1ull << 32)) return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.count x light_count x light_samples must stay below 2^32");
  int32_t rc = pass_options(o, "a direct-light call", kOptTraversal | kOptCollectStats);
  if (rc != RAYCA_OK) return rc;
  if (o.traversal == RAYCA_TRAVERSAL_EXHAUSTIVE)
    return fail(RAYCA_ERR_UNSUPPORTED, "RaycaRenderOptions.traversal: a shadow ray ends at its first hit: there is no exhaustive form");
  if (rd.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if ((rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  const std::vector<HostLight>& lights = s->host.lights;
  if (rd.light_first > lights.size() || rd.light_count > lights.size() - rd.light_first)
    return fail(RAYCA_ERR_BAD_ARG, "RaycaDirect.light_first + light_count exceeds the scene's " + std::to_string(lights.size()) + " lights");
  DirectIo io{};
  for (uint32_t li = 0; li < rd.light_first + rd.light_count; ++li) {
    const uint32_t kind = lights[li].kind;
    if (li < rd.light_first) {
      if (kind != RAYCA_LIGHT_POINT) ++io.quad_base;   // (what nee_prepare's other branch serves: two dimensions a sample)
      continue;
    }
    if (kind == RAYCA_LIGHT_DIRECTIONAL)
      return fail(RAYCA_ERR_UNSUPPORTED, "light " + std::to_string(li) + " is directional: NEE has no sample for it (todo!() in the reference, nee.rs:178)");
    if (kind != RAYCA_LIGHT_POINT) io.quad_bits |= 1ull << (li - rd.light_first);
  }
  io.points = static_cast<const float*>(rd.points);
  io.normals = static_cast<const float*>(rd.normals);
  io.bias = rd.bias;
  io.count = rd.count;
  io.samples = samples;
  io.light_first = rd.light_first;
  io.light_samples = cfg.light_samples;
  io.light_stratify = cfg.light_stratify;
  io.strate_count = cfg.light_stratify ? (uint32_t)sqrtf((float)cfg.light_samples) : 1u;  // config.rs:73-79, as frame_params
  io.seed = cfg.seed;
  io.sample = rd.sample;
  io.first_index = rd.first_index;
  io.count_traced = stats_out ? 1u : 0u;
  io.irradiance_out = static_cast<float4*>(rd.irradiance_out);
  io.sh_out = static_cast<float4*>(rd.sh_out);
  io.mask_out = static_cast<unsigned long long*>(rd.mask_out);
  io.counts_out = static_cast<uint32_t*>(rd.counts_out);
  const bool stats = o.collect_stats != 0, sph = s->host.sphere_count != 0;
  const bool fold = rd.irradiance_out || rd.sh_out || rd.counts_out;   // (mask_out alone is the trace kernel's own work)
  const uint32_t total = rd.count * samples, batches = (total + 63u) / 64u;
  const size_t mask_bytes = (size_t)rd.count * sizeof(unsigned long long);
  FrameCtx* c = &s->ctx[o.context];
  TraceCounters tc{};
  uint32_t node_format = 0;
  rc = run_pass(
      s, o, stats_out,
      [&](FrameCtx* ctx) -> int32_t {
        if (io.mask_out) return RAYCA_OK;
        HIP_TRY(hipSetDevice(s->device));
        return grow_behind_pass(ctx, ctx->ambient_mask, mask_bytes);
      },
      [&](hipStream_t stream, uint32_t& launches) -> int32_t {
        io.mask = io.mask_out ? io.mask_out : static_cast<unsigned long long*>(c->ambient_mask.ptr);
        const bool fast = s->dev.ref_leaf_of != nullptr;   // the reference-leaf filter is present (RAYCA_BUILDER_SAH)
        const bool all_formats = formats_ready(s);
        const bool refill = fast && all_formats;           // (rayca_hip_ambient_device's rule)
        uint32_t grid = (batches + 3u) / 4u;               // one sample per lane; the persistent grid below replaces it
        StackPlan sp{};
        node_format = all_formats ? 0u : 2048u;
        if (refill) {
          sp = plan_stack(std::max(s->host.max_depth, s->host.max_depth4), RAYCA_WF_LDS_ENTRIES);
          const uint32_t in_flight = frames_in_flight_hint(s, o.context, o.stream != nullptr);
          if (const int32_t grc = persistent_grid(s, direct_refill_kernel(sphere, sph, stats), sp.lds_bytes, batches, true, in_flight, 0u, grid); grc != RAYCA_OK) return grc;
          node_format |= (RAYCA_WF_BOUNCE_WIDE ? 1u : 0u) | (RAYCA_WF_BOUNCE_HALF ? 4u : 0u);
        } else {
          sp = plan_stack(s->host.max_depth);
          if (fast && RAYCA_NODE_CH && RAYCA_NODE_CH48 && s->dev.nodes_ch) node_format |= 4096u;
        }
        TraceLaunch tl{};
        if (const int32_t brc = bind_stack(c, sp, grid, tl); brc != RAYCA_OK) return brc;
        if (stats || io.count_traced) HIP_TRY(hipMemsetAsync(c->counters, 0, sizeof(TraceCounters), stream));
        HIP_TRY(hipMemsetAsync(io.mask, 0, mask_bytes, stream));
        if (refill) {
          tl.ticket = 1u;
          HIP_TRY(hipMemsetAsync(c->heads, 0, 8 * kHeadStride * sizeof(uint32_t), stream));
          c->heads_clean &= ~FrameCtx::kCleanHeads;   // the next frame of this context clears them for itself
          launch_direct_refill(sphere, sph, stats, grid, sp.lds_bytes, stream, s->dev_full, io, c->heads, c->counters, tl);
        } else {
          hipLaunchKernelGGL(pick_direct_kernel(sphere, fast, sph, stats), dim3(grid), dim3(kBlock), sp.lds_bytes, stream, all_formats ? s->dev_full : s->dev, io,
                             c->counters, tl);
        }
        HIP_TRY(hipGetLastError());
        ++launches;
        if (fold) {
          hipLaunchKernelGGL(pick_direct_fold(sphere, io.sh_out != nullptr), dim3((rd.count + kDirectFoldBlock - 1u) / kDirectFoldBlock), dim3(kDirectFoldBlock), 0, stream,
                             s->dev.lights, io);
          HIP_TRY(hipGetLastError());
          ++launches;
        }
        // (read back inside the pass, under the context's lock: with stats_out the pass waits for the stream before it returns)
        if (stats_out) HIP_TRY(hipMemcpyAsync(&tc, c->counters, sizeof tc, hipMemcpyDeviceToHost, stream));
        return RAYCA_OK;
      });
  if (rc != RAYCA_OK || !stats_out) return rc;
  stats_out->rays_shadow = tc.shadow;   // the samples that were traced: dropped and empty samples and inactive points cost no ray
  stats_out->boxes_tested = tc.boxes;
  stats_out->triangles_tested = tc.tris;
  stats_out->wave_box_slots = tc.box_slots;
  stats_out->wave_triangle_slots = tc.tri_slots;
  stats_out->node_format = node_format;
  return RAYCA_OK;
}

// Surface records for hit records (surface.inc k_surface): no traversal, one launch.  A pass on its context (ContextPass), so
// that a rayca_hip_scene_update of materials never overwrites a table this kernel is still reading.
int32_t rayca_hip_surface_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaSurfaceQuery* qin, RaycaStats* stats_out) {
  if (!s || !qin) return fail(RAYCA_ERR_BAD_ARG, "null scene or query");
  const RaycaSurfaceQuery& sq = *qin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (sq.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaSurfaceQuery.reserved must be zero");
  // (an empty batch has no arrays: its pointers are not looked at, everything else is checked as for any batch)
  const bool some = sq.count != 0;
  if (some && (!sq.t || !sq.prim || !sq.uv)) return fail(RAYCA_ERR_BAD_ARG, "null hit records (t, prim and uv are all required)");
  const bool full = sq.point_out || sq.normal_out || sq.diffuse_out || sq.specular_out || sq.rough_out;
  if (some && !full && !sq.color_out && !sq.material_out && !sq.flags_out) return fail(RAYCA_ERR_BAD_ARG, "no output");
  if (some && !sq.rays && (sq.point_out || sq.normal_out)) return fail(RAYCA_ERR_BAD_ARG, "null rays: point_out and normal_out need the rays the records belong to");
  int32_t rc = pass_options(o, "a surface call", 0u);
  if (rc != RAYCA_OK) return rc;
  if ((rc = refuse_empty_scene(s)) != RAYCA_OK) return rc;
  if (sq.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  SurfaceIo io{};
  io.rays = static_cast<const float*>(sq.rays);
  io.t = static_cast<const float*>(sq.t);
  io.prim = static_cast<const uint32_t*>(sq.prim);
  io.uv = static_cast<const float*>(sq.uv);
  io.count = sq.count;
  io.full = full ? 1u : 0u;   // color, material and flags alone: shade_hit stops behind get_color, as for a Flat frame
  io.point_out = static_cast<float*>(sq.point_out);
  io.normal_out = static_cast<float*>(sq.normal_out);
  io.color_out = static_cast<float*>(sq.color_out);
  io.diffuse_out = static_cast<float*>(sq.diffuse_out);
  io.specular_out = static_cast<float*>(sq.specular_out);
  io.rough_out = static_cast<float*>(sq.rough_out);
  io.material_out = static_cast<uint32_t*>(sq.material_out);
  io.flags_out = static_cast<uint32_t*>(sq.flags_out);
  const uint32_t grid = (uint32_t)(((uint64_t)sq.count + kBlock - 1u) / kBlock);
  return run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) -> int32_t {
    hipLaunchKernelGGL(pick_surface_kernel(s->host.sphere_count != 0), dim3(grid), dim3(kBlock), 0, stream, formats_ready(s) ? s->dev_full : s->dev, io);
    HIP_TRY(hipGetLastError());
    ++launches;
    return RAYCA_OK;
  });
}

// The camera rays of one sample of a frame (surface.inc k_camera_rays), from the FrameParams a render call would hand its
// kernels for the same arguments (camera_frame_params, camera_sample_params).
int32_t rayca_hip_camera_rays_device(RaycaScene* s, const RaycaConfig* cfg, uint32_t width, uint32_t height, uint32_t sample,
                                     const RaycaRenderOptions* opts_in, void* d_rays_out) {
  if (!s || !cfg) return fail(RAYCA_ERR_BAD_ARG, "null scene or config");
  if (width == 0 || height == 0) return fail(RAYCA_ERR_BAD_ARG, "empty image");
  if (cfg->samples_per_pixel == 0 || sample >= cfg->samples_per_pixel) return fail(RAYCA_ERR_BAD_ARG, "sample must be below samples_per_pixel");
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  int32_t rc = pass_options(o, "the camera-ray export", kOptTile);
  if (rc != RAYCA_OK) return rc;
  if (!s->host.has_camera) return fail(RAYCA_ERR_NO_CAMERA, "scene has no camera (scene.rs:109)");
  FrameParams fp{};
  uint64_t count = 0;
  return run_pass(s, o, nullptr, [&](FrameCtx*) -> int32_t {   // (the camera is the scene's to move: read under the context's lock)
    const int32_t prc = camera_frame_params(s, width, height, o.tile, fp);
    if (prc != RAYCA_OK) return prc;
    if (fp.rows == 0) return kPassNothing;
    if (!d_rays_out) return fail(RAYCA_ERR_BAD_ARG, "null output");
    count = (uint64_t)fp.rows * width;
    if (count > 0xFFFFFFFFull) return fail(RAYCA_ERR_BAD_ARG, "more than 2^32 - 1 rays");
    fp.spp = cfg->samples_per_pixel;
    camera_sample_params(cfg->samples_per_pixel, sample, fp);
    return RAYCA_OK;
  }, [&](hipStream_t stream, uint32_t& launches) -> int32_t {
    hipLaunchKernelGGL(k_camera_rays, dim3((uint32_t)((count + kBlock - 1u) / kBlock)), dim3(kBlock), 0, stream, fp, static_cast<float*>(d_rays_out));
    HIP_TRY(hipGetLastError());
    ++launches;
    return RAYCA_OK;
  });
}

}  // extern "C"

// ---- what the two ray-fed calls (rayca_hip_radiance_device, rayca_hip_gather_device) check and set up alike ------------------
namespace {

// The Config's values, from the struct alone (RAYCA_ERR_BAD_ARG).
int32_t ray_fed_config_args(const RaycaConfig& cfg) {
  if (cfg.integrator > RAYCA_INTEGRATOR_PATHTRACER) return fail(RAYCA_ERR_BAD_ARG, "RaycaConfig.integrator: unknown integrator");
  if (cfg.direct_sampler > RAYCA_SAMPLER_MIS) return fail(RAYCA_ERR_BAD_ARG, "RaycaConfig.direct_sampler: unknown sampler");
  if (cfg.indirect_sampler > RAYCA_SAMPLER_MIS) return fail(RAYCA_ERR_BAD_ARG, "RaycaConfig.indirect_sampler: unknown sampler");
  if (cfg.light_samples == 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaConfig.light_samples must be > 0");
  return RAYCA_OK;
}
// What the queue-fed generation kernels do not cover (the per-pixel stack machine and the exhaustive instantiations have no
// queue-fed form): RAYCA_ERR_UNSUPPORTED, behind the options.  `what`: "a radiance query", ...
int32_t ray_fed_unsupported(const RaycaRenderOptions& o, const RaycaConfig& cfg, const char* what) {
  if (o.traversal == RAYCA_TRAVERSAL_EXHAUSTIVE) return fail(RAYCA_ERR_UNSUPPORTED, std::string("RaycaRenderOptions.traversal: ") + what + " has no exhaustive form");
  if (const char* field = generation_kernels_gap(cfg))
    return fail(RAYCA_ERR_UNSUPPORTED, std::string("RaycaConfig.") + field + ": " + what + " runs on the generation kernels only (Flat; Pathtracer with NEE or no direct sampler, cosine or hemisphere bounces, no roulette, one light sample where it bounces)");
  return RAYCA_OK;
}
// The scene, behind the empty batch.
int32_t ray_fed_scene(const RaycaScene* s, const RaycaConfig& cfg) {
  if (const int32_t rc = refuse_empty_scene(s); rc != RAYCA_OK) return rc;
  if (nee_meets_directional_light(s, cfg)) return fail(RAYCA_ERR_UNSUPPORTED, "RaycaConfig.direct_sampler: a directional light under NEE is a todo!() of the reference (nee.rs:178)");
  return RAYCA_OK;
}
// The Frame of `count` fed rays, up to frame_begin: a one-sample frame of the wavefront engine, one row of `count` pixels; none of
// the camera's terms is read by a queue-fed kernel.
void ray_fed_frame(Frame& f, RaycaScene* s, const RaycaConfig& cfg, const RaycaRenderOptions& o, const RayFeed* feed, uint32_t count) {
  f.s = s;
  f.cfg = cfg;
  f.cfg.samples_per_pixel = 1;   // (not read from the caller's: a call is one sample of every ray)
  f.opts = o;
  f.rays = feed;
  const bool flat = cfg.integrator == RAYCA_INTEGRATOR_FLAT;
  f.plan = LaunchPlan{flat ? kModeFlat : kModePath, true, o.collect_stats != 0, true, flat ? 1u : cfg.max_depth};
  FrameParams& fp = f.fp;
  fp.width = count; fp.height = 1; fp.rows = 1;
  fp.part = 0; fp.parts = 1; fp.band = 1;
}

}  // namespace

extern "C" {

// Radiance along the caller's rays: a one-sample frame of the wavefront engine, run by the frame driver (frame_begin, frame_run,
// frame_finish) as render_body's is.  What is its own are the driver's three differences, all behind f.rays: generation 0 reads
// its rays from a queue that k_enqueue_rays (wavefront.inc) fills -- queue 1, the queue generation 1 writes over once generation
// 0 has read it, and which is therefore there at every depth -- and the Frame's shape is one row of `count` pixels.  So every
// generation runs the queue-fed kernels: closest hits on k_queue_refill (SAH scenes) or k_wf_trace<false>, shading on
// k_wf_shade<.., RAYS> at depth 0, shadow rays on k_shadow_refill<false> / k_wf_shadow<false>.  "Pixel" i is ray i; k_resolve
// (one sample: it finalises) or the Flat shade kernel writes out[i].
int32_t rayca_hip_radiance_device(RaycaScene* s, const RaycaConfig* cfg_in, const RaycaRenderOptions* opts_in, const RaycaRadiance* rin,
                                  RaycaStats* stats_out) {
  if (!s || !cfg_in || !rin) return fail(RAYCA_ERR_BAD_ARG, "null scene, config or RaycaRadiance");
  const RaycaRadiance& rr = *rin;
  const RaycaConfig& cfg = *cfg_in;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if ((uint64_t)rr.first_index + rr.count > (1ull << 32)) return fail(RAYCA_ERR_BAD_ARG, "RaycaRadiance.first_index + count exceeds 2^32");
  if (rr.count > (1u << 31)) return fail(RAYCA_ERR_BAD_ARG, "RaycaRadiance.count exceeds 2^31");
  if (rr.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaRadiance.reserved must be zero");
  if (!rr.rays) return fail(RAYCA_ERR_BAD_ARG, "RaycaRadiance.rays: null rays");
  if (!rr.rgba32f_out && !rr.rgba8_out) return fail(RAYCA_ERR_BAD_ARG, "no output: RaycaRadiance.rgba32f_out and rgba8_out are both null");
  if (reinterpret_cast<uintptr_t>(rr.rgba32f_out) & 15u) return fail(RAYCA_ERR_BAD_ARG, "RaycaRadiance.rgba32f_out must be 16-byte aligned");
  int32_t rc = ray_fed_config_args(cfg);
  if (rc != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a radiance query", kOptTraversal | kOptCollectStats)) != RAYCA_OK) return rc;
  if ((rc = ray_fed_unsupported(o, cfg, "a radiance query")) != RAYCA_OK) return rc;
  if (rr.count == 0) {
    if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
    return RAYCA_OK;
  }
  if ((rc = ray_fed_scene(s, cfg)) != RAYCA_OK) return rc;

  std::lock_guard<std::mutex> lock(s->ctx[o.context].mu);
  Frame f{};
  const RayFeed feed{static_cast<const float*>(rr.rays), nullptr, rr.first_index, rr.sample};
  ray_fed_frame(f, s, cfg, o, &feed, rr.count);
  ContextPass pass{};
  if ((rc = pass_acquire(s, o, stats_out != nullptr, pass)) != RAYCA_OK) return rc;
  if ((rc = frame_begin(f, pass, rr.rgba8_out, rr.rgba32f_out)) != RAYCA_OK || (rc = frame_run(f)) != RAYCA_OK) return rc;
  return frame_finish(f, pass, stats_out, false);
}

// Irradiance at points (gather.inc): the call's points in internal frames of whole points, each a radiance query's frame whose
// generation 0 is fed by k_enqueue_gather -- ambient.inc's rays, made in registers -- and whose records k_gather_fold folds
// behind k_resolve, on the same stream.  Each internal frame is a pass of its own on the context (so the statistics of each are a
// frame's, and are summed); the caller's wait_event goes in front of the first, its record_event behind the last.  The records live
// in samples_out or in the context's gather_samples, sized by the largest frame: the first.
int32_t rayca_hip_gather_device(RaycaScene* s, const RaycaConfig* cfg_in, const RaycaRenderOptions* opts_in, const RaycaGather* gin,
                                RaycaStats* stats_out) {
  if (!s || !cfg_in || !gin) return fail(RAYCA_ERR_BAD_ARG, "null scene, config or RaycaGather");
  const RaycaGather& rg = *gin;
  const RaycaConfig& cfg = *cfg_in;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  // everything the structs alone decide, before the scene handle is looked at
  if (!rg.points) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.points: null points");
  if (!rg.normals) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.normals: null normals");
  if (!rg.dirs) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.dirs: null dirs");
  if (rg.samples == 0 || rg.samples > 64) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.samples: 1 .. 64 samples a point");
  if (rg.dir_first > rg.dir_count || rg.samples > rg.dir_count - rg.dir_first)
    return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.dir_first + samples exceeds dir_count");
  if (rg.reserved[0] != 0 || rg.reserved[1] != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.reserved must be zero");
  if (!rg.irradiance_out && !rg.sh_out && !rg.kept_out && !rg.samples_out) return fail(RAYCA_ERR_BAD_ARG, "no output for a gather call");
  if (reinterpret_cast<uintptr_t>(rg.irradiance_out) & 15u) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.irradiance_out must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(rg.sh_out) & 15u) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.sh_out must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(rg.samples_out) & 15u) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.samples_out must be 16-byte aligned");
  if (!std::isfinite(rg.bias)) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.bias is not finite");
  const uint64_t total = (uint64_t)rg.count * rg.samples;
  if ((uint64_t)rg.first_index + total > (1ull << 32)) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.first_index + count x samples exceeds 2^32");
  if (total > (1ull << 31)) return fail(RAYCA_ERR_BAD_ARG, "RaycaGather.count x samples exceeds 2^31");
  int32_t rc = ray_fed_config_args(cfg);
  if (rc != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a gather call", kOptTraversal | kOptCollectStats)) != RAYCA_OK) return rc;
  if ((rc = ray_fed_unsupported(o, cfg, "a gather call")) != RAYCA_OK) return rc;
  if (!(cfg.gamma == 1.0f)) return fail(RAYCA_ERR_UNSUPPORTED, "RaycaConfig.gamma: a gather call folds linear radiance: gamma must be exactly 1");
  if (stats_out) std::memset(stats_out, 0, sizeof *stats_out);
  if (rg.count == 0) return RAYCA_OK;
  if ((rc = ray_fed_scene(s, cfg)) != RAYCA_OK) return rc;

  const uint32_t samples = rg.samples;
  uint32_t per_frame = std::max(1u, kGatherFrameRays / samples);
  if (rg.chunk_points != 0 && rg.chunk_points < per_frame) per_frame = rg.chunk_points;
  const bool sh = rg.sh_out != nullptr, weights = rg.weights != nullptr, rot = rg.rotations != nullptr;
  std::lock_guard<std::mutex> lock(s->ctx[o.context].mu);
  for (uint32_t first = 0; first < rg.count;) {
    const uint32_t points = std::min(per_frame, rg.count - first), rays = points * samples;
    const size_t ray0 = (size_t)first * samples;
    RaycaRenderOptions of = o;
    if (first != 0) of.wait_event = nullptr;
    if (first + points != rg.count) of.record_event = nullptr;
    GatherIo io{};
    io.a.points = static_cast<const float*>(rg.points) + 3ull * first;
    io.a.normals = static_cast<const float*>(rg.normals) + 3ull * first;
    io.a.rotations = rot ? static_cast<const float*>(rg.rotations) + 2ull * first : nullptr;
    io.a.dirs = static_cast<const float*>(rg.dirs) + 3ull * rg.dir_first;
    io.a.radius_all = INFINITY;   // (ambient_point's radius: not read by either kernel)
    io.a.bias = rg.bias;
    io.a.count = points;
    io.a.samples = samples;
    io.weights = weights ? static_cast<const float*>(rg.weights) + rg.dir_first : nullptr;
    io.first_index = rg.first_index + (uint32_t)ray0;
    io.irradiance_out = rg.irradiance_out ? static_cast<float4*>(rg.irradiance_out) + first : nullptr;
    io.sh_out = sh ? static_cast<float4*>(rg.sh_out) + 9ull * first : nullptr;
    io.kept_out = rg.kept_out ? static_cast<uint32_t*>(rg.kept_out) + first : nullptr;
    io.samples_out = rg.samples_out ? static_cast<float4*>(rg.samples_out) + ray0 : nullptr;
    Frame f{};
    const RayFeed feed{nullptr, &io, io.first_index, rg.sample};
    ray_fed_frame(f, s, cfg, of, &feed, rays);
    ContextPass pass{};
    if ((rc = pass_acquire(s, of, stats_out != nullptr, pass)) != RAYCA_OK) return rc;
    if (!io.samples_out && (rc = grow_behind_pass(pass.c, pass.c->gather_samples, (size_t)rays * sizeof(float4))) != RAYCA_OK) return rc;
    io.samples = io.samples_out ? io.samples_out : static_cast<float4*>(pass.c->gather_samples.ptr);
    if ((rc = frame_begin(f, pass, nullptr, io.samples)) != RAYCA_OK || (rc = frame_run(f)) != RAYCA_OK) return rc;
    rc = timed_launch(f.log, f.stream, RAYCA_KERNEL_OTHER, f.timing, false, [&] {
      hipLaunchKernelGGL(pick_gather_fold(sh, weights, rot), dim3((points + kGatherFoldBlock - 1u) / kGatherFoldBlock), dim3(kGatherFoldBlock), 0, f.stream, io);
      return RAYCA_OK;
    });
    if (rc != RAYCA_OK) return rc;
    RaycaStats st{};
    if ((rc = frame_finish(f, pass, stats_out ? &st : nullptr, false)) != RAYCA_OK) return rc;
    if (stats_out) stats_add(*stats_out, st);
    first += points;
  }
  return RAYCA_OK;
}

}  // extern "C"

#include "post.inc"
