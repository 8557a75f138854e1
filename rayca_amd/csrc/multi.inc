// multi.inc -- one frame on several devices of one process: rayca_hip_render_multi, its _issue / _wait forms and
// rayca_hip_rccl_status (declared in include/rayca_hip.h).  Included from api.inc behind the frame driver, whose render_body
// every part runs; k_deinterleave is in aux_kernels.inc.  The state lives in the scene that assembles the frame (MultiCtx and
// MultiFrame, defined above RaycaScene in api.inc); here is how it is released, how a frame is issued -- MultiIssue, a list of
// named steps over one struct with one way out on failure -- and how it is waited for.
namespace {

// RCCL is opened at first use: the library has no link-time dependency on it, and a process that already has one loaded
// (PyTorch ships its own librccl) keeps using that one.
struct Rccl {
  using Comm = void*;
  int (*CommInitAll)(Comm*, int, const int*) = nullptr;
  int (*CommDestroy)(Comm) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, Comm, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, Comm, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
  std::string why;
  static constexpr int kUint8 = 1;  // ncclUint8 (rccl.h)
  Rccl() {
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
    if (!h) {
      const char* e = dlerror();
      why = std::string("librccl could not be opened: ") + (e ? e : "?");
      return;
    }
    auto sym = [&](const char* n) { return dlsym(h, n); };
    CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
    GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
    GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
    Send = reinterpret_cast<decltype(Send)>(sym("ncclSend"));
    Recv = reinterpret_cast<decltype(Recv)>(sym("ncclRecv"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
    ok = CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetErrorString;
    if (!ok) why = "librccl lacks one of ncclCommInitAll / ncclGroupStart / ncclSend / ncclRecv";
  }
};
Rccl& rccl() {
  static Rccl r;
  return r;
}
#define RCCL_TRY(expr)                                                                                         \
  do {                                                                                                         \
    const int r__ = (expr);                                                                                    \
    if (r__ != 0) return fail(RAYCA_ERR_RCCL, std::string(#expr) + ": " + rccl().GetErrorString(r__));        \
  } while (0)

}  // namespace

// ---- the owners: what a set of devices was given is given back in one place ---------------------------------------------------
// One context's frame: the parts' events on their own devices, then -- on the assembling device, devices[0] -- the event and the
// two buffers of the assembly.
void MultiFrame::release(const std::vector<int>& devices) {
  for (size_t i = 0; i < done.size(); ++i) {
    if (i < devices.size()) (void)hipSetDevice(devices[i]);
    if (done[i]) (void)hipEventDestroy(done[i]);
  }
  done.clear();
  if (!devices.empty()) (void)hipSetDevice(devices[0]);
  if (gathered) (void)hipEventDestroy(gathered);
  gathered = nullptr;
  gathered_valid = false;
  gather.release();
  frame.release();
  pending = false;
  rccl = false;
}
// Everything made for the current set of devices: issue threads, communicators, every context's frame.  Leaves the assembling
// device current.  Called when another set is adopted (MultiIssue::adopt_device_set) and by scene_destroy_now.
void MultiCtx::release() {
  workers.clear();   // (joins the issue threads)
  if (!comms.empty() && rccl().ok)
    for (void* c : comms)
      if (c) (void)rccl().CommDestroy(c);
  comms.clear();
  for (MultiFrame& f : frames) f.release(devices);
  devices.clear();
  peer_enabled = false;
}

namespace {

// Frame context `context` of every scene, locked in ADDRESS order: two calls that share scenes in different orders (or
// with a different scenes[0]) cannot wait for each other in a cycle.
std::vector<std::unique_lock<std::mutex>> lock_contexts(RaycaScene* const* scenes, uint32_t count, uint32_t context) {
  std::vector<RaycaScene*> order(scenes, scenes + count);
  std::sort(order.begin(), order.end(), [](const RaycaScene* a, const RaycaScene* b) { return std::less<const RaycaScene*>()(a, b); });
  std::vector<std::unique_lock<std::mutex>> locks;
  for (RaycaScene* sc : order) locks.emplace_back(sc->ctx[context].mu);
  return locks;
}

// The handles of a call and its frame context: what issue and wait both need to be true.
int32_t multi_check_handles(RaycaScene* const* scenes, uint32_t count, uint32_t context) {
  if (!scenes || count == 0) return fail(RAYCA_ERR_BAD_ARG, "null argument");
  if (count > 64) return fail(RAYCA_ERR_BAD_ARG, "more than 64 devices");
  if (context >= kMaxContexts) return fail(RAYCA_ERR_BAD_ARG, "context out of range");
  for (uint32_t i = 0; i < count; ++i)
    if (!scenes[i]) return fail(RAYCA_ERR_BAD_ARG, "null scene");
  for (uint32_t i = 0; i < count; ++i)
    for (uint32_t j = i + 1; j < count; ++j)
      if (scenes[i] == scenes[j]) return fail(RAYCA_ERR_BAD_ARG, "the same scene handle twice");
  return RAYCA_OK;
}
// The options of an issue, on handles that multi_check_handles has passed.
int32_t multi_check_options(RaycaScene* const* scenes, uint32_t count, const RaycaMultiOptions& mo) {
  if (mo.gather > RAYCA_GATHER_PEER_COPY) return fail(RAYCA_ERR_BAD_ARG, "unknown gather transport");
  if (mo.gather != RAYCA_GATHER_RCCL) return RAYCA_OK;
  for (uint32_t i = 0; i < count; ++i)
    for (uint32_t j = i + 1; j < count; ++j)
      if (scenes[i]->device == scenes[j]->device) return fail(RAYCA_ERR_BAD_ARG, "RCCL needs every part on its own device (two scenes share one)");
  return RAYCA_OK;
}

// every part's stream of this context drained: nothing of a frame that failed half-way may still be writing the gather /
// staging buffers when the caller gets the error (the next call may free and regrow them)
void multi_drain(RaycaScene* const* scenes, uint32_t count, uint32_t context) {
  for (uint32_t i = 0; i < count; ++i) {
    if (hipSetDevice(scenes[i]->device) != hipSuccess) continue;
    if (scenes[i]->ctx[context].stream) (void)hipStreamSynchronize(scenes[i]->ctx[context].stream);
  }
  (void)hipSetDevice(scenes[0]->device);
  (void)hipGetLastError();
}

// ---- issuing a frame --------------------------------------------------------------------------------------------------------
// The whole frame queued on the devices: every part's kernels, the one exchange, the de-interleave, the copy-out.  What the
// steps share; multi_issue below runs them in the order they stand here, holding scenes[0]'s multi_mu and context `ctx` of every
// scene.  Every step returns a status and cleans nothing up: what a failure costs is multi_issue's to decide, by `started`.
struct MultiIssue {
  // the call
  RaycaScene* const* scenes;
  uint32_t count;
  const RaycaConfig* cfg;
  uint32_t width, height;
  RaycaMultiOptions mo;
  void* rgba8_out;
  RaycaStats* stats_out;   // rayca_hip_render_multi with statistics: every part's render call waits for its own kernels to read its counters
  bool asynchronous;
  // the row split (rayca_hip_tile_rows: the same arithmetic the kernels and rayca_amd/distributed.py use)
  uint32_t band = 0, ctx = 0, max_rows = 0;
  std::vector<uint32_t> rows;
  std::vector<int> devices;   // device of every part
  // the assembling scene, its state for the set of devices and for this frame context
  RaycaScene* s0 = nullptr;
  MultiCtx* m = nullptr;
  MultiFrame* f = nullptr;
  // per part: where it renders to, and what its render call returned
  std::vector<void*> part_dst;
  std::vector<int32_t> part_rc;
  std::vector<std::string> part_err;
  bool started = false;   // work of this frame may be queued on a device: a failure from here on drains before it returns

  hipStream_t part_stream(uint32_t i) const { return scenes[i]->ctx[ctx].stream; }
  bool by_rccl() const { return count > 1 && mo.gather == RAYCA_GATHER_RCCL; }

  int32_t part_geometry() {
    band = mo.band_rows ? mo.band_rows : 8u;
    ctx = mo.context;
    rows.resize(count);
    devices.resize(count);
    for (uint32_t i = 0; i < count; ++i) {
      rows[i] = tile_rows(RaycaTile{i, count, band, 0}, height);
      max_rows = std::max(max_rows, rows[i]);
      devices[i] = scenes[i]->device;
    }
    return RAYCA_OK;
  }

  // First call, or another set of devices: communicators, events, buffers and issue threads are per set.
  int32_t adopt_device_set() {
    s0 = scenes[0];
    m = &s0->multi;
    f = &m->frames[ctx];
    if (m->devices == devices) return RAYCA_OK;
    // (frames of the previous set still in flight: their exchange and copy-out end with `gathered`, an event of this scene)
    (void)hipSetDevice(s0->device);
    for (MultiFrame& old : m->frames)
      if (old.pending && old.gathered) (void)hipEventSynchronize(old.gathered);
    m->release();
    m->devices = devices;
    for (uint32_t i = 1; i < count; ++i) m->workers.emplace_back(new PartWorker());
    return RAYCA_OK;
  }

  // This context's events and its two buffers on the assembling device.  No context pass uses those buffers -- the exchange and the
  // de-interleave are queued by this call alone -- so they grow by plain ensure, behind a drain of the frame that may still use them.
  int32_t frame_resources() {
    if (f->done.size() != count) {
      f->done.assign(count, nullptr);
      for (uint32_t i = 0; i < count; ++i) {
        HIP_TRY(hipSetDevice(devices[i]));
        HIP_TRY(hipEventCreateWithFlags(&f->done[i], hipEventDisableTiming));
      }
    }
    HIP_TRY(hipSetDevice(s0->device));
    if (!f->gathered) HIP_TRY(hipEventCreateWithFlags(&f->gathered, hipEventDisableTiming));
    const size_t frame_bytes = (size_t)width * height * 4u, gather_bytes = (size_t)count * max_rows * width * 4u;
    if (f->pending && (f->frame.bytes < frame_bytes || (count > 1 && f->gather.bytes < gather_bytes))) multi_drain(scenes, count, ctx);
    int32_t rc = ensure(f->frame, frame_bytes);
    if (rc == RAYCA_OK && count > 1) rc = ensure(f->gather, gather_bytes);
    return rc;
  }

  int32_t open_transport() {
    if (by_rccl() && m->comms.empty()) {
      if (!rccl().ok) return fail(RAYCA_ERR_RCCL, rccl().why);
      m->comms.assign(count, nullptr);
      RCCL_TRY(rccl().CommInitAll(m->comms.data(), (int)count, devices.data()));
    }
    if (count > 1 && mo.gather == RAYCA_GATHER_PEER_COPY && !m->peer_enabled) {
      for (uint32_t i = 1; i < count; ++i) {
        if (devices[i] == s0->device) continue;
        int can = 0;
        HIP_TRY(hipDeviceCanAccessPeer(&can, s0->device, devices[i]));
        if (can) {
          const hipError_t e = hipDeviceEnablePeerAccess(devices[i], 0);
          if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(e);
          (void)hipGetLastError();
        }
      }
      m->peer_enabled = true;
    }
    return RAYCA_OK;
  }

  // Part 0 renders straight into its slot of the gather buffer (or, alone, into the frame); the others into their own
  // context's staging buffer, which the exchange reads: their next frame of this context must not start before it has.
  // (That wait is all this step queues: it is for the previous frame, nothing of this one.)
  int32_t stage_parts() {
    part_dst.assign(count, nullptr);
    for (uint32_t i = 0; i < count; ++i) {
      FrameCtx* c = &scenes[i]->ctx[ctx];
      HIP_TRY(hipSetDevice(devices[i]));
      int32_t rc = ensure_ctx(scenes[i], c);
      if (rc != RAYCA_OK) return rc;
      if (i == 0) {
        part_dst[0] = count == 1 ? f->frame.ptr : f->gather.ptr;
        continue;
      }
      if ((rc = grow_behind_pass(c, c->out8, (size_t)max_rows * width * 4u + 16u)) != RAYCA_OK) return rc;
      part_dst[i] = c->out8.ptr;
      if (f->gathered_valid) HIP_TRY(hipStreamWaitEvent(c->stream, f->gathered, 0));
    }
    return RAYCA_OK;
  }

  // One part's frame, on the thread that issues it: render_body on the part's own stream, then the part's `done` event.
  void render_part(uint32_t i) {
    RaycaRenderOptions o{};
    o.traversal = mo.traversal;
    o.collect_stats = mo.collect_stats;
    o.engine = mo.engine;
    o.context = ctx;
    o.tile = RaycaTile{i, count, band, 0};
    // an asynchronous frame names its stream, so that the scene sees the frames the host keeps in flight (frames_in_flight_hint)
    o.stream = asynchronous ? static_cast<void*>(part_stream(i)) : nullptr;
    if (hipSetDevice(devices[i]) != hipSuccess) {
      part_rc[i] = RAYCA_ERR_HIP;
      part_err[i] = "hipSetDevice failed";
      return;
    }
    part_rc[i] = render_body(scenes[i], cfg, width, height, &o, rows[i] ? part_dst[i] : nullptr, nullptr, stats_out ? &stats_out[i] : nullptr, true);
    if (part_rc[i] != RAYCA_OK) part_err[i] = g_last_error;
    else if (hipEventRecord(f->done[i], part_stream(i)) != hipSuccess) {
      part_rc[i] = RAYCA_ERR_HIP;
      part_err[i] = "hipEventRecord failed";
    }
  }
  // Parts 1.. on the set's issue threads, part 0 on this one; the first part that failed is the frame's error.
  int32_t render_parts() {
    part_rc.assign(count, RAYCA_OK);
    part_err.assign(count, std::string());
    started = true;
    for (uint32_t i = 1; i < count; ++i) m->workers[i - 1]->post([this, i] { render_part(i); });
    render_part(0);
    for (uint32_t i = 1; i < count; ++i) m->workers[i - 1]->wait();
    for (uint32_t i = 0; i < count; ++i)
      if (part_rc[i] != RAYCA_OK) return fail(part_rc[i], "part " + std::to_string(i) + ": " + part_err[i]);
    return RAYCA_OK;
  }

  // The single exchange of the frame into the gather buffer's slots, then the de-interleave into the frame -- on part 0's stream.
  int32_t queue_exchange() {
    HIP_TRY(hipSetDevice(s0->device));
    if (count == 1) return RAYCA_OK;
    const hipStream_t stream0 = part_stream(0);
    char* gather = static_cast<char*>(f->gather.ptr);
    const size_t slot = (size_t)max_rows * width * 4u;
    if (mo.gather == RAYCA_GATHER_RCCL) {
      // every other part sends its packed rows, part 0 receives them into their slots
      RCCL_TRY(rccl().GroupStart());
      for (uint32_t i = 1; i < count; ++i) {
        if (!rows[i]) continue;
        const size_t bytes = (size_t)rows[i] * width * 4u;
        RCCL_TRY(rccl().Send(part_dst[i], bytes, Rccl::kUint8, 0, m->comms[i], part_stream(i)));
        RCCL_TRY(rccl().Recv(gather + i * slot, bytes, Rccl::kUint8, (int)i, m->comms[0], stream0));
      }
      RCCL_TRY(rccl().GroupEnd());
      HIP_TRY(hipSetDevice(s0->device));
    } else {
      for (uint32_t i = 1; i < count; ++i) {
        if (!rows[i]) continue;
        HIP_TRY(hipStreamWaitEvent(stream0, f->done[i], 0));
        HIP_TRY(hipMemcpyPeerAsync(gather + i * slot, s0->device, part_dst[i], devices[i], (size_t)rows[i] * width * 4u, stream0));
      }
    }
    const uint32_t npix = width * height;
    hipLaunchKernelGGL(k_deinterleave, dim3((npix + 255u) / 256u), dim3(256), 0, stream0, static_cast<const uint32_t*>(f->gather.ptr),
                       static_cast<uint32_t*>(f->frame.ptr), width, height, count, band, max_rows);
    HIP_TRY(hipGetLastError());
    return RAYCA_OK;
  }

  // The frame to the caller's memory, and `gathered` behind it: what the wait, the next frame's parts and a regrowth wait for.
  int32_t copy_out() {
    const hipStream_t stream0 = part_stream(0);
    HIP_TRY(hipMemcpyAsync(rgba8_out, f->frame.ptr, (size_t)width * height * 4u, mo.output_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream0));
    HIP_TRY(hipEventRecord(f->gathered, stream0));
    return RAYCA_OK;
  }
};

// The driver, and the one failure path.  Before anything of this frame may be queued a failure is a plain return.  From then on
// parts may be running into the staging and gather buffers: every part's stream is drained, nothing is pending on the context,
// and the caller gets the first error with its message (a part's starts "part i: ").
int32_t multi_issue(RaycaScene* const* scenes, uint32_t count, const RaycaConfig* cfg, uint32_t width, uint32_t height, const RaycaMultiOptions& mo,
                    void* rgba8_out, RaycaStats* stats_out, bool asynchronous) {
  if (!cfg || !rgba8_out) return fail(RAYCA_ERR_BAD_ARG, "null argument");
  if (width == 0 || height == 0) return fail(RAYCA_ERR_BAD_ARG, "empty image");
  MultiIssue mi{scenes, count, cfg, width, height, mo, rgba8_out, stats_out, asynchronous};
  std::lock_guard<std::mutex> multi_lock(scenes[0]->multi_mu);
  std::vector<std::unique_lock<std::mutex>> ctx_locks = lock_contexts(scenes, count, mo.context);
  using Step = int32_t (MultiIssue::*)();
  int32_t rc = RAYCA_OK;
  for (Step step : {&MultiIssue::part_geometry, &MultiIssue::adopt_device_set, &MultiIssue::frame_resources, &MultiIssue::open_transport,
                    &MultiIssue::stage_parts, &MultiIssue::render_parts, &MultiIssue::queue_exchange, &MultiIssue::copy_out})
    if ((rc = (mi.*step)()) != RAYCA_OK) break;
  if (rc != RAYCA_OK) {
    if (!mi.started) return rc;
    const std::string why = g_last_error;
    multi_drain(scenes, count, mi.ctx);
    mi.f->pending = false;
    return fail(rc, why);
  }
  mi.f->gathered_valid = true;
  mi.f->pending = true;
  mi.f->rccl = mi.by_rccl();
  return RAYCA_OK;
}

// The frame last issued on `context` has landed in its rgba8_out.  Its errors were its issue's to return; this returns an error of the
// synchronisation alone, and then the frame stays pending: the caller may wait again.
int32_t multi_wait(RaycaScene* const* scenes, uint32_t count, uint32_t context) {
  RaycaScene* s0 = scenes[0];
  std::lock_guard<std::mutex> multi_lock(s0->multi_mu);
  MultiFrame& f = s0->multi.frames[context];
  if (!f.pending) return RAYCA_OK;
  HIP_TRY(hipSetDevice(s0->device));
  HIP_TRY(hipEventSynchronize(f.gathered));
  if (f.rccl) {  // the senders' streams have finished too once the receives have (grouped send/recv complete together); make it explicit
    for (uint32_t i = 1; i < count; ++i) {
      HIP_TRY(hipSetDevice(scenes[i]->device));
      if (scenes[i]->ctx[context].stream) HIP_TRY(hipStreamSynchronize(scenes[i]->ctx[context].stream));
    }
    HIP_TRY(hipSetDevice(s0->device));
  }
  f.pending = false;
  return RAYCA_OK;
}

}  // namespace

extern "C" {

int32_t rayca_hip_rccl_status(void) { return rccl().ok ? RAYCA_OK : fail(RAYCA_ERR_RCCL, rccl().why); }

int32_t rayca_hip_render_multi(RaycaScene* const* scenes, uint32_t count, const RaycaConfig* cfg, uint32_t width, uint32_t height,
                               const RaycaMultiOptions* opts_in, void* rgba8_out, RaycaStats* stats_out) {
  RaycaMultiOptions mo{};
  if (opts_in) mo = *opts_in;
  int32_t rc = multi_check_handles(scenes, count, mo.context);
  if (rc != RAYCA_OK || (rc = multi_check_options(scenes, count, mo)) != RAYCA_OK) return rc;
  if ((rc = multi_issue(scenes, count, cfg, width, height, mo, rgba8_out, stats_out, false)) != RAYCA_OK) return rc;
  return multi_wait(scenes, count, mo.context);
}

int32_t rayca_hip_render_multi_issue(RaycaScene* const* scenes, uint32_t count, const RaycaConfig* cfg, uint32_t width, uint32_t height,
                                     const RaycaMultiOptions* opts_in, void* rgba8_out) {
  RaycaMultiOptions mo{};
  if (opts_in) mo = *opts_in;
  int32_t rc = multi_check_handles(scenes, count, mo.context);
  if (rc != RAYCA_OK || (rc = multi_check_options(scenes, count, mo)) != RAYCA_OK) return rc;
  if (mo.collect_stats) return fail(RAYCA_ERR_BAD_ARG, "statistics need a synchronisation per frame: rayca_hip_render_multi");
  return multi_issue(scenes, count, cfg, width, height, mo, rgba8_out, nullptr, true);
}

int32_t rayca_hip_render_multi_wait(RaycaScene* const* scenes, uint32_t count, uint32_t context) {
  const int32_t rc = multi_check_handles(scenes, count, context);
  if (rc != RAYCA_OK) return rc;
  return multi_wait(scenes, count, context);
}

}  // extern "C"
