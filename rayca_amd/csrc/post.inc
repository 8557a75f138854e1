// post.inc -- the entry points of the image-space post passes (included from api.inc behind its last entry point): denoise,
// accumulate, denoise_variance, upsample, meter, tonemap, sample_plan and film_fold, their kernel pickers, and the checks they share.  A pass reads
// and writes images in device memory; its scene handle gives the device and the frame context (stream, scratch, ordering
// against the context's frames and queries), and nothing is read through it before the pass runs.
//
// One order of checks (DESIGN 4.7): the argument struct's own fields -- `reserved`, the frame's size and tile count
// (frame_tiles), then the pointers and parameters, their alignment and aliasing -- and RaycaRenderOptions last (pass_options).
// Every check stands in front of any GPU work.  run_pass (api.inc) does the rest.

namespace {

// A frame's pixel count and the grid of the 64 x 4 tiles that cover it (image_pass.inc tile_pixel).
struct FrameTiles {
  uint32_t count;     // width * height
  uint32_t tiles_x;   // blocks per tile row
  uint32_t tiles;     // blocks
};
int32_t frame_tiles(uint32_t width, uint32_t height, const char* type, FrameTiles& f) {
  if (width == 0 || height == 0) return fail(RAYCA_ERR_BAD_ARG, std::string("empty image (") + type + ".width, height)");
  const uint64_t count = (uint64_t)width * height;
  if (count > 0xFFFFFFFFull) return fail(RAYCA_ERR_BAD_ARG, std::string("more than 2^32 - 1 pixels (") + type + ".width x height)");
  const uint32_t tiles_x = (uint32_t)(((uint64_t)width + kDenoiseTileW - 1u) / kDenoiseTileW);
  const uint64_t tiles = (uint64_t)tiles_x * (((uint64_t)height + kDenoiseTileH - 1u) / kDenoiseTileH);
  if (tiles * kBlock > 0xFFFFFFFFull) return fail(RAYCA_ERR_UNSUPPORTED, "the frame's 64 x 4 tiles hold more than 2^32 - 1 lanes: one launch cannot cover it");
  f = FrameTiles{(uint32_t)count, tiles_x, (uint32_t)tiles};
  return RAYCA_OK;
}
uint32_t flat_grid(uint32_t count) { return (uint32_t)(((uint64_t)count + kBlock - 1u) / kBlock); }

bool misaligned(const void* ptr, uintptr_t to) { return (reinterpret_cast<uintptr_t>(ptr) & (to - 1u)) != 0u; }
using Pointers = std::initializer_list<const void*>;
// the images read and written 16 bytes a pixel, then those read and written 4 bytes an element (a NULL pointer is aligned)
int32_t check_alignment(Pointers by16, const char* message16, Pointers by4, const char* message4) {
  for (const void* ptr : by16)
    if (misaligned(ptr, 16)) return fail(RAYCA_ERR_BAD_ARG, message16);
  for (const void* ptr : by4)
    if (misaligned(ptr, 4)) return fail(RAYCA_ERR_BAD_ARG, message4);
  return RAYCA_OK;
}
// true where an output that is given is one of the inputs
bool output_is_input(Pointers outputs, Pointers inputs) {
  for (const void* out : outputs)
    for (const void* in : inputs)
      if (out && out == in) return true;
  return false;
}

bool finite_f32(float x) { return x - x == 0.0f; }

// where the guides of a tap stand in a kernel table: [no guide, normal, normal + point]
int guide_index(bool normal, bool point) { return point ? 2 : (normal ? 1 : 0); }

// ---- what the two denoisers share: their scratch images and the launches around their iterations ----------------------------
// The first `images` scratch images of the context, and with `planes` its two variance planes: run_pass's preparation step,
// since they have to be there before the pass queues its waits.
int32_t denoise_scratch(RaycaScene* s, FrameCtx* c, uint32_t images, size_t image_bytes, bool planes, size_t plane_bytes) {
  HIP_TRY(hipSetDevice(s->device));
  int32_t rc = RAYCA_OK;
  for (uint32_t i = 0; i < images; ++i)
    if ((rc = grow_behind_pass(c, c->denoise[i], image_bytes)) != RAYCA_OK) return rc;
  if (planes)
    for (DeviceBuffer& plane : c->denoise_var)
      if ((rc = grow_behind_pass(c, plane, plane_bytes)) != RAYCA_OK) return rc;
  return rc;
}
// The ping-pong between the two scratch images: no kernel reads the image it writes.
struct PingPong {
  const float4* src;    // what the next kernel reads: `color` at first
  float4* scratch[2];
  uint32_t next;        // the scratch image the next kernel writes (never the one `src` is)
  PingPong(const float4* color, FrameCtx* c) : src(color), scratch{static_cast<float4*>(c->denoise[0].ptr), static_cast<float4*>(c->denoise[1].ptr)}, next(0) {}
  float4* dst() const { return scratch[next]; }
  void advance() {
    src = scratch[next];
    next ^= 1u;
  }
};
int32_t launch_demod(hipStream_t stream, PingPong& images, const float4* albedo, uint32_t count, uint32_t& launches) {
  hipLaunchKernelGGL(k_denoise_demod, dim3(flat_grid(count)), dim3(kBlock), 0, stream, images.src, albedo, images.dst(), count);
  HIP_TRY(hipGetLastError());
  images.advance();
  ++launches;
  return RAYCA_OK;
}
int32_t launch_finish(hipStream_t stream, const float4* src, const float4* albedo, float gamma, void* rgba8_out, float4* rgba32f_out, uint32_t count,
                      uint32_t& launches) {
  const float inv_gamma = 1.0f / gamma;   // (as a frame's: color/mod.rs:175-176)
  hipLaunchKernelGGL(k_denoise_finish, dim3(flat_grid(count)), dim3(kBlock), 0, stream, src, albedo, inv_gamma, static_cast<uint8_t*>(rgba8_out), rgba32f_out, count);
  HIP_TRY(hipGetLastError());
  ++launches;
  return RAYCA_OK;
}
// one launch over the frame's tiles
template <typename Io>
int32_t launch_tiles(hipStream_t stream, void (*kernel)(Io), const FrameTiles& f, const Io& io, uint32_t& launches) {
  hipLaunchKernelGGL(kernel, dim3(f.tiles), dim3(kBlock), 0, stream, io);
  HIP_TRY(hipGetLastError());
  ++launches;
  return RAYCA_OK;
}

// ---- the kernel for the terms, guides and outputs that are present ------------------------------------------------------------
// k_atrous: [colour term][guides][id]
using AtrousKernel = void (*)(AtrousIo);
AtrousKernel pick_atrous_kernel(bool color, bool normal, bool point, bool id) {
#define RAYCA_ATROUS(C, N, P) {k_atrous<C, N, P, false>, k_atrous<C, N, P, true>}
  static const AtrousKernel table[2][3][2] = {{RAYCA_ATROUS(false, false, false), RAYCA_ATROUS(false, true, false), RAYCA_ATROUS(false, true, true)},
                                              {RAYCA_ATROUS(true, false, false), RAYCA_ATROUS(true, true, false), RAYCA_ATROUS(true, true, true)}};
#undef RAYCA_ATROUS
  return table[color ? 1 : 0][guide_index(normal, point)][id ? 1 : 0];
}
// k_accumulate: identity mode [moments], reprojection [id][prev_point][moments]
using AccumulateKernel = void (*)(AccumulateIo);
AccumulateKernel pick_accumulate_kernel(bool reproject, bool id, bool plane, bool moments) {
  if (!reproject) return moments ? k_accumulate<false, false, false, true> : k_accumulate<false, false, false, false>;
#define RAYCA_ACCUMULATE(I, P) {k_accumulate<true, I, P, false>, k_accumulate<true, I, P, true>}
  static const AccumulateKernel table[2][2][2] = {{RAYCA_ACCUMULATE(false, false), RAYCA_ACCUMULATE(false, true)},
                                                  {RAYCA_ACCUMULATE(true, false), RAYCA_ACCUMULATE(true, true)}};
#undef RAYCA_ACCUMULATE
  return table[id ? 1 : 0][plane ? 1 : 0][moments ? 1 : 0];
}
// k_variance_init: [no length, length, length + spatial estimate]; the spatial estimate's [guides][id].  Without the spatial
// estimate no guide is read.
using VarianceInitKernel = void (*)(VarianceInitIo);
VarianceInitKernel pick_variance_init_kernel(bool length, bool spatial, bool normal, bool point, bool id) {
  if (!spatial) return length ? k_variance_init<true, false, false, false, false> : k_variance_init<false, false, false, false, false>;
#define RAYCA_VARIANCE_INIT(N, P) {k_variance_init<true, true, N, P, false>, k_variance_init<true, true, N, P, true>}
  static const VarianceInitKernel table[3][2] = {RAYCA_VARIANCE_INIT(false, false), RAYCA_VARIANCE_INIT(true, false), RAYCA_VARIANCE_INIT(true, true)};
#undef RAYCA_VARIANCE_INIT
  return table[guide_index(normal, point)][id ? 1 : 0];
}
// k_atrous_var: [guides][id]
using AtrousVarKernel = void (*)(AtrousVarIo);
AtrousVarKernel pick_atrous_var_kernel(bool normal, bool point, bool id) {
#define RAYCA_ATROUS_VAR(N, P) {k_atrous_var<N, P, false>, k_atrous_var<N, P, true>}
  static const AtrousVarKernel table[3][2] = {RAYCA_ATROUS_VAR(false, false), RAYCA_ATROUS_VAR(true, false), RAYCA_ATROUS_VAR(true, true)};
#undef RAYCA_ATROUS_VAR
  return table[guide_index(normal, point)][id ? 1 : 0];
}
// k_upsample: [albedo][guides][id]
using UpsampleKernel = void (*)(UpsampleIo);
UpsampleKernel pick_upsample_kernel(bool albedo, bool normal, bool point, bool id) {
#define RAYCA_UPSAMPLE(A, N, P) {k_upsample<A, N, P, false>, k_upsample<A, N, P, true>}
  static const UpsampleKernel table[2][3][2] = {{RAYCA_UPSAMPLE(false, false, false), RAYCA_UPSAMPLE(false, true, false), RAYCA_UPSAMPLE(false, true, true)},
                                                {RAYCA_UPSAMPLE(true, false, false), RAYCA_UPSAMPLE(true, true, false), RAYCA_UPSAMPLE(true, true, true)}};
#undef RAYCA_UPSAMPLE
  return table[albedo ? 1 : 0][guide_index(normal, point)][id ? 1 : 0];
}
// k_tonemap: [op][rgba32f][rgba8]
using TonemapKernel = void (*)(TonemapIo);
TonemapKernel pick_tonemap_kernel(uint32_t op, bool f32, bool u8) {
#define RAYCA_TONEMAP(OP) {{nullptr, k_tonemap<OP, false, true>}, {k_tonemap<OP, true, false>, k_tonemap<OP, true, true>}}
  static const TonemapKernel table[3][2][2] = {RAYCA_TONEMAP(kTonemapLinear), RAYCA_TONEMAP(kTonemapReinhard), RAYCA_TONEMAP(kTonemapAces)};
#undef RAYCA_TONEMAP
  return table[op][f32 ? 1 : 0][u8 ? 1 : 0];
}

}  // namespace

extern "C" {

// The a-trous denoiser (denoise.inc): [k_denoise_demod] -> k_atrous x iterations -> k_denoise_finish, between the context's two
// scratch images.  No kernel reads an image it writes -- every iteration goes from one image to another, and the only kernel
// that writes rgba32f_out reads a scratch image -- which is what lets rgba32f_out be `color` itself.
int32_t rayca_hip_denoise_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaDenoise* din, RaycaStats* stats_out) {
  if (!s || !din) return fail(RAYCA_ERR_BAD_ARG, "null scene or denoise arguments");
  const RaycaDenoise& d = *din;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (d.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaDenoise.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(d.width, d.height, "RaycaDenoise", f);
  if (rc != RAYCA_OK) return rc;
  if (!d.color) return fail(RAYCA_ERR_BAD_ARG, "null color");
  if (!d.rgba32f_out && !d.rgba8_out) return fail(RAYCA_ERR_BAD_ARG, "no output");
  if (d.iterations > 8) return fail(RAYCA_ERR_BAD_ARG, "iterations above 8");
  if (d.normal_power_log2 > 10) return fail(RAYCA_ERR_BAD_ARG, "normal_power_log2 above 10");
  if (d.point && !d.normal) return fail(RAYCA_ERR_BAD_ARG, "point needs normal: the plane distance is measured along p's normal");
  if (d.point && !(d.sigma_plane > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "sigma_plane must be > 0 when point is given");
  if (!(d.gamma > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "gamma must be > 0");
  const char* const alignment = "alignment: color, albedo and rgba32f_out are read and written 16 bytes a pixel, every other image 4 bytes an element";
  if ((rc = check_alignment({d.color, d.albedo, d.rgba32f_out}, alignment, {d.rgba8_out, d.normal, d.point, d.id}, alignment)) != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a denoise call, which filters a whole frame (a tile's packed rows are not neighbours)", 0u)) != RAYCA_OK) return rc;
  const size_t image_bytes = (size_t)f.count * sizeof(float4);
  const float4* color = static_cast<const float4*>(d.color);
  const float4* albedo = d.iterations ? static_cast<const float4*>(d.albedo) : nullptr;   // (no filter: nothing to demodulate for)
  float4* out32 = static_cast<float4*>(d.rgba32f_out);
  // the output stage reads `color` itself only when nothing runs in front of it; then an rgba32f_out that is `color` goes
  // through a scratch image and a copy
  const bool via_copy = d.iterations == 0 && out32 == color;
  const uint32_t scratch_images = d.iterations == 0 ? (via_copy ? 1u : 0u) : ((albedo || d.iterations > 1) ? 2u : 1u);
  return run_pass(
      s, o, stats_out, [&](FrameCtx* c) { return denoise_scratch(s, c, scratch_images, image_bytes, false, 0); },
      [&](hipStream_t stream, uint32_t& launches) -> int32_t {
        PingPong images(color, &s->ctx[o.context]);
        if (albedo && (rc = launch_demod(stream, images, albedo, f.count, launches)) != RAYCA_OK) return rc;
        if (d.iterations) {
          AtrousIo io{};
          io.normal = static_cast<const float*>(d.normal);
          io.point = static_cast<const float*>(d.point);
          io.id = static_cast<const uint32_t*>(d.id);
          io.width = d.width;
          io.height = d.height;
          io.tiles_x = f.tiles_x;
          io.normal_squarings = d.normal_power_log2;
          const bool with_color = d.sigma_color > 0.0f;
          io.kc = with_color ? 1.0f / (d.sigma_color * d.sigma_color) : 0.0f;
          io.kp = io.point ? 1.0f / (d.sigma_plane * d.sigma_plane) : 0.0f;
          const auto kernel = pick_atrous_kernel(with_color, io.normal != nullptr, io.point != nullptr, io.id != nullptr);
          for (uint32_t i = 0; i < d.iterations; ++i) {
            io.in = images.src;
            io.out = images.dst();
            io.step = 1u << i;
            if ((rc = launch_tiles(stream, kernel, f, io, launches)) != RAYCA_OK) return rc;
            images.advance();
          }
        }
        if ((rc = launch_finish(stream, images.src, albedo, d.gamma, d.rgba8_out, via_copy ? images.scratch[0] : out32, f.count, launches)) != RAYCA_OK) return rc;
        if (via_copy) HIP_TRY(hipMemcpyAsync(out32, images.scratch[0], image_bytes, hipMemcpyDeviceToDevice, stream));
        return RAYCA_OK;
      });
}

// Temporal accumulation (temporal.inc): one launch of k_accumulate, no scratch image.  Identity mode (no prev_camera) is
// pixel-local, so an output may be the history it continues; in reprojection mode the taps read neighbours, and an output that
// is one of the images they read is refused.
int32_t rayca_hip_accumulate_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaAccumulate* ain, RaycaStats* stats_out) {
  if (!s || !ain) return fail(RAYCA_ERR_BAD_ARG, "null scene or accumulate arguments");
  const RaycaAccumulate& a = *ain;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (a.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaAccumulate.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(a.width, a.height, "RaycaAccumulate", f);
  if (rc != RAYCA_OK) return rc;
  if (!a.color) return fail(RAYCA_ERR_BAD_ARG, "null color");
  if (!a.color_out) return fail(RAYCA_ERR_BAD_ARG, "null color_out");
  if (!a.length_out) return fail(RAYCA_ERR_BAD_ARG, "null length_out");
  const bool reproject = a.prev_camera != nullptr;
  if (reproject && (!a.point || !a.normal)) return fail(RAYCA_ERR_BAD_ARG, "point and normal are required with prev_camera");
  if (!reproject && (a.point || a.normal)) return fail(RAYCA_ERR_BAD_ARG, "point and normal must be NULL without prev_camera");
  if ((a.id != nullptr) != (a.prev_id != nullptr)) return fail(RAYCA_ERR_BAD_ARG, "id and prev_id: both or neither");
  if ((a.hist_color != nullptr) != (a.hist_length != nullptr)) return fail(RAYCA_ERR_BAD_ARG, "hist_color and hist_length: both or neither");
  const bool history = a.hist_color != nullptr;
  if (a.hist_moments && !history) return fail(RAYCA_ERR_BAD_ARG, "hist_moments needs hist_color and hist_length");
  if (reproject && history && !a.prev_normal) return fail(RAYCA_ERR_BAD_ARG, "prev_normal is required with prev_camera and a history");
  if (a.moments_out && history && !a.hist_moments) return fail(RAYCA_ERR_BAD_ARG, "moments_out needs hist_moments where there is a history");
  if (a.variance_out && !a.moments_out) return fail(RAYCA_ERR_BAD_ARG, "variance_out needs moments_out");
  if (reproject && !(a.normal_min > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "normal_min must be > 0 with prev_camera");
  if (reproject && a.prev_point && !(a.plane_max > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "plane_max must be > 0 when prev_point is given");
  if ((rc = check_alignment({a.color, a.hist_color, a.color_out}, "alignment: color, hist_color and color_out are read and written 16 bytes a pixel",
                               {a.point, a.normal, a.id, a.hist_length, a.hist_moments, a.prev_normal, a.prev_point, a.prev_id, a.length_out, a.moments_out, a.variance_out},
                               "alignment: every image but color, hist_color and color_out is read and written 4 bytes an element")) != RAYCA_OK) return rc;
  if (reproject && output_is_input({a.color_out, a.length_out, a.moments_out, a.variance_out},
                                   {a.hist_color, a.hist_length, a.hist_moments, a.prev_normal, a.prev_point, a.prev_id}))
    return fail(RAYCA_ERR_BAD_ARG, "aliasing: with prev_camera the taps read neighbours, so no output may be a hist_ or prev_ input");
  if ((rc = pass_options(o, "an accumulate call, which reads a whole frame (a tile's packed rows are not neighbours)", 0u)) != RAYCA_OK) return rc;
  AccumulateIo io{};
  io.color = static_cast<const float4*>(a.color);
  io.hist_color = static_cast<const float4*>(a.hist_color);
  io.hist_length = static_cast<const float*>(a.hist_length);
  io.color_out = static_cast<float4*>(a.color_out);
  io.length_out = static_cast<float*>(a.length_out);
  const bool moments = a.moments_out != nullptr;
  if (moments) {
    io.hist_moments = static_cast<const float*>(a.hist_moments);
    io.moments_out = static_cast<float*>(a.moments_out);
    io.variance_out = static_cast<float*>(a.variance_out);
  }
  io.width = a.width;
  io.height = a.height;
  io.tiles_x = f.tiles_x;
  io.cap = (float)a.max_history;
  // without a history no pixel has one, whatever the camera did: the identity kernel with a null history writes the first frame
  const bool taps = reproject && history;
  if (taps) {
    const RaycaCameraPose& cam = *a.prev_camera;   // (HOST memory, copied here)
    io.point = static_cast<const float*>(a.point);
    io.normal = static_cast<const float*>(a.normal);
    io.prev_normal = static_cast<const float*>(a.prev_normal);
    io.prev_point = static_cast<const float*>(a.prev_point);
    io.id = static_cast<const uint32_t*>(a.id);
    io.prev_id = static_cast<const uint32_t*>(a.prev_id);
    io.normal_min = a.normal_min;
    io.plane_max = a.plane_max;
    io.fw = (float)a.width;
    io.fh = (float)a.height;
    io.angle = cam.angle;
    io.angle_aspect = cam.angle * (io.fw / io.fh);   // (aspect as camera_frame_params forms it)
    io.ox = cam.origin[0]; io.oy = cam.origin[1]; io.oz = cam.origin[2];
    io.rx = cam.right[0]; io.ry = cam.right[1]; io.rz = cam.right[2];
    io.ux = cam.up[0]; io.uy = cam.up[1]; io.uz = cam.up[2];
    io.bx = cam.back[0]; io.by = cam.back[1]; io.bz = cam.back[2];
  }
  const auto kernel = pick_accumulate_kernel(taps, taps && io.id != nullptr, taps && io.prev_point != nullptr, moments);
  return run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) { return launch_tiles(stream, kernel, f, io, launches); });
}

// The variance-guided a-trous denoiser (denoise_variance.inc): [k_denoise_demod] -> k_variance_init -> k_atrous_var x iterations
// -> k_denoise_finish, between the context's two scratch images and its two variance planes.  No kernel reads an image it
// writes: every iteration goes from one image and plane to the others, `variance` is read by k_variance_init alone (into a
// plane), and the only writers of rgba32f_out and variance_out run behind every reader of `color` and `variance` -- which is what
// lets rgba32f_out be `color` and variance_out be `variance`.
int32_t rayca_hip_denoise_variance_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaDenoiseVariance* din, RaycaStats* stats_out) {
  if (!s || !din) return fail(RAYCA_ERR_BAD_ARG, "null scene or denoise arguments");
  const RaycaDenoiseVariance& d = *din;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (d.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaDenoiseVariance.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(d.width, d.height, "RaycaDenoiseVariance", f);
  if (rc != RAYCA_OK) return rc;
  if (!d.color) return fail(RAYCA_ERR_BAD_ARG, "null color");
  if (!d.variance) return fail(RAYCA_ERR_BAD_ARG, "null variance");
  if (!d.rgba32f_out && !d.rgba8_out) return fail(RAYCA_ERR_BAD_ARG, "no output (rgba32f_out, rgba8_out)");
  if (d.iterations == 0 || d.iterations > 8) return fail(RAYCA_ERR_BAD_ARG, "iterations must be 1..8");
  if (d.normal_power_log2 > 10) return fail(RAYCA_ERR_BAD_ARG, "normal_power_log2 above 10");
  if (d.min_history > 0 && !d.length) return fail(RAYCA_ERR_BAD_ARG, "min_history > 0 needs length: the history length chooses the spatial estimate");
  if (d.point && !d.normal) return fail(RAYCA_ERR_BAD_ARG, "point needs normal: the plane distance is measured along p's normal");
  if (d.point && !(d.sigma_plane > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "sigma_plane must be > 0 when point is given");
  if (!(d.sigma_luminance > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "sigma_luminance must be > 0");
  if (!(d.variance_floor > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "variance_floor must be > 0");
  if (!(d.gamma > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "gamma must be > 0");
  if ((rc = check_alignment({d.color, d.albedo, d.rgba32f_out}, "alignment: color, albedo and rgba32f_out are read and written 16 bytes a pixel",
                               {d.variance, d.length, d.normal, d.point, d.id, d.rgba8_out, d.variance_out},
                               "alignment: every image but color, albedo and rgba32f_out is read and written 4 bytes an element")) != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a denoise call, which filters a whole frame (a tile's packed rows are not neighbours)", 0u)) != RAYCA_OK) return rc;
  const size_t image_bytes = (size_t)f.count * sizeof(float4), plane_bytes = (size_t)f.count * sizeof(float);
  const float4* albedo = static_cast<const float4*>(d.albedo);
  const uint32_t scratch_images = (albedo || d.iterations > 1) ? 2u : 1u;
  return run_pass(
      s, o, stats_out, [&](FrameCtx* c) { return denoise_scratch(s, c, scratch_images, image_bytes, true, plane_bytes); },
      [&](hipStream_t stream, uint32_t& launches) -> int32_t {
        FrameCtx* c = &s->ctx[o.context];
        PingPong images(static_cast<const float4*>(d.color), c);
        float* const planes[2] = {static_cast<float*>(c->denoise_var[0].ptr), static_cast<float*>(c->denoise_var[1].ptr)};
        if (albedo && (rc = launch_demod(stream, images, albedo, f.count, launches)) != RAYCA_OK) return rc;
        const float* normal = static_cast<const float*>(d.normal);
        const float* point = static_cast<const float*>(d.point);
        const uint32_t* id = static_cast<const uint32_t*>(d.id);
        const float kp = point ? 1.0f / (d.sigma_plane * d.sigma_plane) : 0.0f;
        {
          VarianceInitIo io{};
          io.color = images.src;
          io.albedo = albedo;
          io.variance = static_cast<const float*>(d.variance);
          io.length = static_cast<const float*>(d.length);
          io.var_out = planes[0];
          io.width = d.width;
          io.height = d.height;
          io.tiles_x = f.tiles_x;
          const bool spatial = d.min_history > 0;
          if (spatial) {
            io.normal = normal;
            io.point = point;
            io.id = id;
            io.normal_squarings = d.normal_power_log2;
            io.kp = kp;
            io.min_history = (float)d.min_history;
          }
          const auto kernel = pick_variance_init_kernel(io.length != nullptr, spatial, spatial && normal, spatial && point, spatial && id);
          if ((rc = launch_tiles(stream, kernel, f, io, launches)) != RAYCA_OK) return rc;
        }
        uint32_t plane = 0;   // the variance plane the next iteration reads
        AtrousVarIo io{};
        io.normal = normal;
        io.point = point;
        io.id = id;
        io.width = d.width;
        io.height = d.height;
        io.tiles_x = f.tiles_x;
        io.normal_squarings = d.normal_power_log2;
        io.sl2 = d.sigma_luminance * d.sigma_luminance;
        io.variance_floor = d.variance_floor;
        io.kp = kp;
        const auto kernel = pick_atrous_var_kernel(normal != nullptr, point != nullptr, id != nullptr);
        for (uint32_t i = 0; i < d.iterations; ++i) {
          io.in = images.src;
          io.out = images.dst();
          io.var_in = planes[plane];
          io.var_out = planes[plane ^ 1u];
          io.step = 1u << i;
          if ((rc = launch_tiles(stream, kernel, f, io, launches)) != RAYCA_OK) return rc;
          images.advance();
          plane ^= 1u;
        }
        if ((rc = launch_finish(stream, images.src, albedo, d.gamma, d.rgba8_out, static_cast<float4*>(d.rgba32f_out), f.count, launches)) != RAYCA_OK) return rc;
        if (d.variance_out) HIP_TRY(hipMemcpyAsync(d.variance_out, planes[plane], plane_bytes, hipMemcpyDeviceToDevice, stream));
        return RAYCA_OK;
      });
}

// Guided upsampling (upsample.inc): one launch of k_upsample, no scratch image.  Every tap reads the low images and every
// output is full size, so no output may be an input.
int32_t rayca_hip_upsample_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaUpsample* uin, RaycaStats* stats_out) {
  if (!s || !uin) return fail(RAYCA_ERR_BAD_ARG, "null scene or upsample arguments");
  const RaycaUpsample& u = *uin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (u.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaUpsample.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(u.width, u.height, "RaycaUpsample", f);
  if (rc != RAYCA_OK) return rc;
  if (u.scale == 0 || u.scale > 8) return fail(RAYCA_ERR_BAD_ARG, "scale must be 1..8");
  if (u.width % u.scale != 0 || u.height % u.scale != 0)
    return fail(RAYCA_ERR_BAD_ARG, "width and height must be divisible by scale: the two views share one aspect ratio, bit for bit");
  if (u.normal_power_log2 > 10) return fail(RAYCA_ERR_BAD_ARG, "normal_power_log2 above 10");
  if (!u.color) return fail(RAYCA_ERR_BAD_ARG, "null color");
  if (!u.rgba32f_out && !u.rgba8_out) return fail(RAYCA_ERR_BAD_ARG, "no output (rgba32f_out, rgba8_out)");
  if ((u.albedo != nullptr) != (u.albedo_low != nullptr)) return fail(RAYCA_ERR_BAD_ARG, "albedo and albedo_low: both or neither");
  if ((u.normal != nullptr) != (u.normal_low != nullptr)) return fail(RAYCA_ERR_BAD_ARG, "normal and normal_low: both or neither");
  if ((u.point != nullptr) != (u.point_low != nullptr)) return fail(RAYCA_ERR_BAD_ARG, "point and point_low: both or neither");
  if ((u.id != nullptr) != (u.id_low != nullptr)) return fail(RAYCA_ERR_BAD_ARG, "id and id_low: both or neither");
  if (u.point && !u.normal) return fail(RAYCA_ERR_BAD_ARG, "point needs normal: the plane distance is measured along p's normal");
  if (u.point && !(u.sigma_plane > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "sigma_plane must be > 0 when point is given");
  if (!(u.gamma > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "gamma must be > 0");
  if ((rc = check_alignment({u.color, u.albedo_low, u.albedo, u.rgba32f_out}, "alignment: color, albedo_low, albedo and rgba32f_out are read and written 16 bytes a pixel",
                               {u.normal_low, u.point_low, u.id_low, u.normal, u.point, u.id, u.rgba8_out, u.weight_out},
                               "alignment: every image but color, albedo_low, albedo and rgba32f_out is read and written 4 bytes an element")) != RAYCA_OK) return rc;
  if (output_is_input({u.rgba32f_out, u.rgba8_out, u.weight_out}, {u.color, u.albedo_low, u.normal_low, u.point_low, u.id_low, u.albedo, u.normal, u.point, u.id}))
    return fail(RAYCA_ERR_BAD_ARG, "aliasing: the taps read neighbours and the images differ in size, so no output may be an input");
  if ((rc = pass_options(o, "an upsample call, which resamples a whole frame (a tile's packed rows are not neighbours)", 0u)) != RAYCA_OK) return rc;
  UpsampleIo io{};
  io.color = static_cast<const float4*>(u.color);
  io.albedo_low = static_cast<const float4*>(u.albedo_low);
  io.normal_low = static_cast<const float*>(u.normal_low);
  io.point_low = static_cast<const float*>(u.point_low);
  io.id_low = static_cast<const uint32_t*>(u.id_low);
  io.albedo = static_cast<const float4*>(u.albedo);
  io.normal = static_cast<const float*>(u.normal);
  io.point = static_cast<const float*>(u.point);
  io.id = static_cast<const uint32_t*>(u.id);
  io.rgba32f = static_cast<float4*>(u.rgba32f_out);
  io.rgba8 = static_cast<uint8_t*>(u.rgba8_out);
  io.weight = static_cast<float*>(u.weight_out);
  io.width = u.width;
  io.height = u.height;
  io.low_width = u.width / u.scale;
  io.low_height = u.height / u.scale;
  io.tiles_x = f.tiles_x;
  io.scale = u.scale;
  io.normal_squarings = u.normal_power_log2;
  io.s = (float)u.scale;
  io.kp = io.point ? 1.0f / (u.sigma_plane * u.sigma_plane) : 0.0f;
  io.inv_gamma = 1.0f / u.gamma;   // (as a frame's: color/mod.rs:175-176)
  const auto kernel = pick_upsample_kernel(io.albedo != nullptr, io.normal != nullptr, io.point != nullptr, io.id != nullptr);
  return run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) { return launch_tiles(stream, kernel, f, io, launches); });
}

// Exposure metering (tonemap.inc): the clear of hist_out, k_meter_hist under a capped grid and, with exposure_out, the one-wave
// k_exposure, each behind the other on the pass's stream.
int32_t rayca_hip_meter_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaMeter* m_in, RaycaStats* stats_out) {
  if (!s || !m_in) return fail(RAYCA_ERR_BAD_ARG, "null scene or meter arguments");
  const RaycaMeter& m = *m_in;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (m.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaMeter.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(m.width, m.height, "RaycaMeter", f);
  if (rc != RAYCA_OK) return rc;
  if (!m.color) return fail(RAYCA_ERR_BAD_ARG, "null color");
  if (!m.hist_out) return fail(RAYCA_ERR_BAD_ARG, "null hist_out");
  if (!(m.low_permille < m.high_permille && m.high_permille <= 1000u)) return fail(RAYCA_ERR_BAD_ARG, "low_permille, high_permille: 0 <= low < high <= 1000");
  if (!(m.key > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "key must be > 0");
  if (!(finite_f32(m.min_scale) && m.min_scale > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "min_scale must be finite and > 0");
  if (!(finite_f32(m.max_scale) && m.max_scale >= m.min_scale)) return fail(RAYCA_ERR_BAD_ARG, "max_scale must be finite and >= min_scale");
  if (!(m.rate > 0.0f && m.rate <= 1.0f)) return fail(RAYCA_ERR_BAD_ARG, "rate must be in (0, 1]");
  if ((rc = check_alignment({m.color, m.exposure_out}, "alignment: color and exposure_out are read and written 16 bytes at a time",
                               {m.hist_out, m.exposure_prev}, "alignment: hist_out and exposure_prev are read and written 4 bytes an element")) != RAYCA_OK) return rc;
  if (output_is_input({m.hist_out}, {m.color, m.exposure_out, m.exposure_prev}) || output_is_input({m.exposure_out}, {m.color}))
    return fail(RAYCA_ERR_BAD_ARG, "aliasing: hist_out must differ from color, exposure_out and exposure_prev, and exposure_out from color");
  if ((rc = pass_options(o, "a meter call, which measures a whole frame", 0u)) != RAYCA_OK) return rc;
  MeterIo io{static_cast<const float4*>(m.color), static_cast<uint32_t*>(m.hist_out), f.count};
  const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)f.count + kMeterBlock - 1u) / kMeterBlock, kMeterMaxGrid);
  return run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) -> int32_t {
    HIP_TRY(hipMemsetAsync(m.hist_out, 0, kMeterWords * sizeof(uint32_t), stream));   // (behind ev_begin: the clear is part of what the call costs)
    ++launches;
    hipLaunchKernelGGL(k_meter_hist, dim3(grid), dim3(kMeterBlock), 0, stream, io);
    HIP_TRY(hipGetLastError());
    ++launches;
    if (m.exposure_out) {
      ExposureIo e{io.hist, static_cast<float*>(m.exposure_out), static_cast<const float*>(m.exposure_prev), m.low_permille, m.high_permille,
                   m.key, m.min_scale, m.max_scale, m.rate};
      hipLaunchKernelGGL(k_exposure, dim3(1), dim3(64), 0, stream, e);
      HIP_TRY(hipGetLastError());
      ++launches;
    }
    return RAYCA_OK;
  });
}

// Tone mapping (tonemap.inc): one launch of k_tonemap, pixel-local, no scratch image.
int32_t rayca_hip_tonemap_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaTonemap* tin, RaycaStats* stats_out) {
  if (!s || !tin) return fail(RAYCA_ERR_BAD_ARG, "null scene or tonemap arguments");
  const RaycaTonemap& t = *tin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (t.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaTonemap.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(t.width, t.height, "RaycaTonemap", f);
  if (rc != RAYCA_OK) return rc;
  if (!t.color) return fail(RAYCA_ERR_BAD_ARG, "null color");
  if (!t.rgba32f_out && !t.rgba8_out) return fail(RAYCA_ERR_BAD_ARG, "no output (rgba32f_out, rgba8_out)");
  if (t.op > RAYCA_TONEMAP_ACES) return fail(RAYCA_ERR_BAD_ARG, "unknown op");
  if (!t.exposure && !(finite_f32(t.scale) && t.scale > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "scale must be finite and > 0 when exposure is not given");
  if (!(finite_f32(t.white) && t.white >= 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "white must be 0 (no white point) or finite and > 0");
  if (t.white != 0.0f && t.op != RAYCA_TONEMAP_REINHARD) return fail(RAYCA_ERR_BAD_ARG, "white belongs to RAYCA_TONEMAP_REINHARD: must be 0 for the other operators");
  if (!(t.gamma > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "gamma must be > 0");
  if ((rc = check_alignment({t.color, t.rgba32f_out}, "alignment: color and rgba32f_out are read and written 16 bytes a pixel", {t.exposure, t.rgba8_out},
                               "alignment: exposure and rgba8_out are read and written 4 bytes an element")) != RAYCA_OK) return rc;
  if (output_is_input({t.rgba8_out}, {t.color, t.rgba32f_out, t.exposure}) || output_is_input({t.rgba32f_out}, {t.exposure}) || (t.exposure && t.exposure == t.color))
    return fail(RAYCA_ERR_BAD_ARG, "aliasing: rgba32f_out may be color; no other two of color, exposure, rgba32f_out and rgba8_out may be equal");
  if ((rc = pass_options(o, "a tonemap call, which maps a whole frame", 0u)) != RAYCA_OK) return rc;
  TonemapIo io{};
  io.color = static_cast<const float4*>(t.color);
  io.exposure = static_cast<const float*>(t.exposure);
  io.rgba32f = static_cast<float4*>(t.rgba32f_out);
  io.rgba8 = static_cast<uint8_t*>(t.rgba8_out);
  io.width = t.width;
  io.height = t.height;
  io.tiles_x = f.tiles_x;
  io.scale = t.scale;
  io.inv_white2 = t.white != 0.0f ? 1.0f / (t.white * t.white) : 0.0f;
  io.inv_gamma = 1.0f / t.gamma;   // (as a frame's: color/mod.rs:175-176)
  const auto kernel = pick_tonemap_kernel(t.op, io.rgba32f != nullptr, io.rgba8 != nullptr);
  return run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) { return launch_tiles(stream, kernel, f, io, launches); });
}

// The sample plan (adaptive.inc): k_plan_weights -> k_plan_scan (one block) -> k_plan_offsets over the frame's tiles and, for
// rays_out or pixel_out, k_plan_rays over the budget, each behind the other on the pass's stream.  The weights go through
// weight_out or the context's scratch, the segment sums through the context's scratch; only the ray kernel reads the scene (its
// camera, taken under the context's lock like a camera-ray export's).
int32_t rayca_hip_sample_plan_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaSamplePlan* pin, RaycaStats* stats_out) {
  if (!s || !pin) return fail(RAYCA_ERR_BAD_ARG, "null scene or sample-plan arguments");
  const RaycaSamplePlan& a = *pin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (a.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaSamplePlan.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(a.width, a.height, "RaycaSamplePlan", f);
  if (rc != RAYCA_OK) return rc;
  if ((uint64_t)f.count * 256u > (1ull << 32))
    return fail(RAYCA_ERR_UNSUPPORTED, "RaycaSamplePlan.width x height x 256 exceeds 2^32: the sum of the weights must fit 32 bits, its product with the budget 64");
  if (a.budget > (1u << 31)) return fail(RAYCA_ERR_BAD_ARG, "RaycaSamplePlan.budget exceeds 2^31");
  if (a.jitter == 0 || a.jitter > 8) return fail(RAYCA_ERR_BAD_ARG, "jitter must be 1..8");
  if (a.base_weight > 255) return fail(RAYCA_ERR_BAD_ARG, "base_weight above 255");
  if (a.fresh_weight > 255) return fail(RAYCA_ERR_BAD_ARG, "fresh_weight above 255");
  if (!(a.target > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "target must be > 0");
  if (!(a.lum_floor > 0.0f)) return fail(RAYCA_ERR_BAD_ARG, "lum_floor must be > 0");
  if (!a.color) return fail(RAYCA_ERR_BAD_ARG, "null color");
  if (!a.variance) return fail(RAYCA_ERR_BAD_ARG, "null variance");
  if (!a.length) return fail(RAYCA_ERR_BAD_ARG, "null length");
  if (!a.offset_out) return fail(RAYCA_ERR_BAD_ARG, "null offset_out");
  if ((rc = check_alignment({a.color}, "alignment: color is read 16 bytes a pixel", {a.variance, a.length, a.weight_out, a.offset_out, a.rays_out, a.pixel_out},
                               "alignment: every image but color is read and written 4 bytes an element")) != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a sample-plan call, which weighs a whole frame", 0u)) != RAYCA_OK) return rc;
  if (a.rays_out && !s->host.has_camera) return fail(RAYCA_ERR_NO_CAMERA, "scene has no camera (scene.rs:109): rays_out needs one");
  const uint32_t segments = f.tiles_x * a.height;   // (<= width x height <= 2^24)
  PlanIo io{};
  io.color = static_cast<const float4*>(a.color);
  io.variance = static_cast<const float*>(a.variance);
  io.length = static_cast<const float*>(a.length);
  io.weight = static_cast<uint32_t*>(a.weight_out);
  io.offset = static_cast<uint32_t*>(a.offset_out);
  io.width = a.width;
  io.height = a.height;
  io.tiles_x = f.tiles_x;
  io.count = f.count;
  io.budget = a.budget;
  io.base_weight = a.base_weight;
  io.fresh_weight = a.fresh_weight;
  io.min_history = (float)a.min_history;
  io.target2 = a.target * a.target;
  io.lum_floor = a.lum_floor;
  const bool rays = a.budget != 0 && (a.rays_out || a.pixel_out);
  const SubPixelGrid grid = sub_pixel_grid(a.jitter * a.jitter);
  PlanRaysIo rio{io.offset, static_cast<float*>(a.rays_out), static_cast<uint32_t*>(a.pixel_out), f.count, a.budget, a.jitter, a.jitter * a.jitter,
                 a.first_stratum % (a.jitter * a.jitter), grid.step};
  FrameParams fp{};
  return run_pass(
      s, o, stats_out,
      [&](FrameCtx* c) -> int32_t {
        HIP_TRY(hipSetDevice(s->device));
        int32_t prc = RAYCA_OK;
        if (!io.weight && (prc = grow_behind_pass(c, c->plan_weight, (size_t)f.count * sizeof(uint32_t))) != RAYCA_OK) return prc;
        if ((prc = grow_behind_pass(c, c->plan_sums, ((size_t)segments + 1u) * sizeof(uint32_t))) != RAYCA_OK) return prc;
        if (rays && rio.rays) {   // (the camera is the scene's to move: read under the context's lock)
          if ((prc = camera_frame_params(s, a.width, a.height, RaycaTile{}, fp)) != RAYCA_OK) return prc;
          fp.sub_offset = grid.offset;
        }
        return RAYCA_OK;
      },
      [&](hipStream_t stream, uint32_t& launches) -> int32_t {
        FrameCtx* c = &s->ctx[o.context];
        if (!io.weight) io.weight = static_cast<uint32_t*>(c->plan_weight.ptr);
        io.sums = static_cast<uint32_t*>(c->plan_sums.ptr);
        if ((rc = launch_tiles(stream, k_plan_weights, f, io, launches)) != RAYCA_OK) return rc;
        hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(kPlanScanBlock), 0, stream, io.sums, segments);
        HIP_TRY(hipGetLastError());
        ++launches;
        hipLaunchKernelGGL(k_plan_offsets, dim3(f.tiles), dim3(kBlock), 0, stream, io, segments);
        HIP_TRY(hipGetLastError());
        ++launches;
        if (rays) {
          hipLaunchKernelGGL(k_plan_rays, dim3(flat_grid(a.budget)), dim3(kBlock), 0, stream, fp, rio);
          HIP_TRY(hipGetLastError());
          ++launches;
        }
        return RAYCA_OK;
      });
}

// The fold of a plan's samples into a history (adaptive.inc): one launch of k_film_fold, pixel-local, no scratch image.
int32_t rayca_hip_film_fold_device(RaycaScene* s, const RaycaRenderOptions* opts_in, const RaycaFilmFold* fin, RaycaStats* stats_out) {
  if (!s || !fin) return fail(RAYCA_ERR_BAD_ARG, "null scene or fold arguments");
  const RaycaFilmFold& a = *fin;
  RaycaRenderOptions o{};
  if (opts_in) o = *opts_in;
  if (a.reserved != 0) return fail(RAYCA_ERR_BAD_ARG, "RaycaFilmFold.reserved must be zero");
  FrameTiles f{};
  int32_t rc = frame_tiles(a.width, a.height, "RaycaFilmFold", f);
  if (rc != RAYCA_OK) return rc;
  if (!a.samples) return fail(RAYCA_ERR_BAD_ARG, "null samples");
  if (!a.offset) return fail(RAYCA_ERR_BAD_ARG, "null offset");
  if (!a.color_out) return fail(RAYCA_ERR_BAD_ARG, "null color_out");
  if (!a.length_out) return fail(RAYCA_ERR_BAD_ARG, "null length_out");
  if (!a.hist_color || !a.hist_length) return fail(RAYCA_ERR_BAD_ARG, "hist_color and hist_length are both required: a fold continues a history");
  if (a.moments_out && !a.hist_moments) return fail(RAYCA_ERR_BAD_ARG, "moments_out needs hist_moments");
  if (a.variance_out && !a.moments_out) return fail(RAYCA_ERR_BAD_ARG, "variance_out needs moments_out");
  if ((rc = check_alignment({a.samples, a.hist_color, a.color_out}, "alignment: samples, hist_color and color_out are read and written 16 bytes a pixel",
                               {a.offset, a.hist_length, a.hist_moments, a.length_out, a.moments_out, a.variance_out},
                               "alignment: every image but samples, hist_color and color_out is read and written 4 bytes an element")) != RAYCA_OK) return rc;
  if ((rc = pass_options(o, "a fold call, which continues a whole frame's history", 0u)) != RAYCA_OK) return rc;
  FoldIo io{};
  io.samples = static_cast<const float4*>(a.samples);
  io.offset = static_cast<const uint32_t*>(a.offset);
  io.hist_color = static_cast<const float4*>(a.hist_color);
  io.hist_length = static_cast<const float*>(a.hist_length);
  io.color_out = static_cast<float4*>(a.color_out);
  io.length_out = static_cast<float*>(a.length_out);
  const bool moments = a.moments_out != nullptr;
  if (moments) {
    io.hist_moments = static_cast<const float*>(a.hist_moments);
    io.moments_out = static_cast<float*>(a.moments_out);
    io.variance_out = static_cast<float*>(a.variance_out);
  }
  io.width = a.width;
  io.height = a.height;
  io.tiles_x = f.tiles_x;
  io.cap = (float)a.max_history;
  const auto kernel = moments ? k_film_fold<true> : k_film_fold<false>;
  return run_pass(s, o, stats_out, [&](hipStream_t stream, uint32_t& launches) { return launch_tiles(stream, kernel, f, io, launches); });
}

}  // extern "C"
