// scene.inc -- the lifetime of a scene: rayca_hip_scene_create as a driver over named build steps, the asynchronous destroy
// and its reaper, finish / info / update / primitive_order / read_nodes.  Included from api.inc, between the frame engines
// (whose helpers the steps use) and the render entry points.

namespace {

// The device tables of a scene's materials and lights: what scene_create uploads and what rayca_hip_scene_update compares
// against and overwrites in place.
std::vector<DevMaterial> dev_materials(const RaycaMaterial* m, size_t count) {
  std::vector<DevMaterial> out(count);
  for (size_t i = 0; i < count; ++i) out[i] = dev_material(m[i]);
  return out;
}
std::vector<DevLight> dev_lights(const std::vector<HostLight>& l) {
  std::vector<DevLight> out(l.size());
  for (size_t i = 0; i < out.size(); ++i) out[i] = dev_light(l[i]);
  return out;
}

// one small BVH build, so that every kernel of bvh_build.hip has been launched once (the first launch of a
// kernel sets up its arguments and scratch: ~10 ms over the five of them inside a process's first real build).
// 20 000 boxes on a lattice: more than one workgroup's worth, so the many-workgroup binning runs too.
void warm_device_builder(int device) {
  const uint32_t wn = 20000;
  std::vector<float> w[9];
  for (auto& v : w) v.resize(wn);
  for (uint32_t i = 0; i < wn; ++i) {
    const float c[3] = {(float)(i % 32u), (float)((i / 32u) % 32u), (float)(i / 1024u)};
    for (int a = 0; a < 3; ++a) {
      w[a][i] = c[a];
      w[3 + a][i] = c[a] - 0.25f;
      w[6 + a][i] = c[a] + 0.25f;
    }
  }
  BlasBuildInput in{};
  for (int a = 0; a < 3; ++a) {
    in.cent[a] = w[a].data();
    in.bmin[a] = w[3 + a].data();
    in.bmax[a] = w[6 + a].data();
    in.root_min[a] = -0.25f;
    in.root_max[a] = 32.25f;
  }
  in.count = wn;
  in.seed_origin = false;
  in.max_depth = 255u;
  in.device = (uint32_t)device;
  std::vector<uint32_t> worder;
  std::vector<BuildNode> warena;
  std::string werr;
  (void)gpu_build_blas(in, worder, warena, werr, nullptr);   // (anything wrong here shows up again, reported, in the real build)
}

// Once per process and device, on the device that is current: what the first HIP calls, the first stream, the first copies and
// the first launches of a process set up, so that no scene build pays for it.
int32_t warm_device(int device, bool build_on_host) {
  static std::mutex warm_mu;
  static std::vector<int> warmed;
  std::lock_guard<std::mutex> warm_lock(warm_mu);
  if (std::find(warmed.begin(), warmed.end(), device) != warmed.end()) return RAYCA_OK;
  HIP_TRY(hipFree(nullptr));
  // the three code objects (kernels.hip, refill.hip, bvh_build.hip) are loaded on first use of a kernel of theirs
  hipFuncAttributes fa{};
  HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_resolve)));
  HIP_TRY(hipFuncGetAttributes(&fa, flat_refill_kernel(RefillFlavour{kTravFast, false, false})));
  HIP_TRY(hipFuncGetAttributes(&fa, gpu_builder_any_kernel()));
  // a process's first stream, first asynchronous copies from pageable memory and first device allocation set up
  // runtime-internal staging (measured: ~150 ms inside the first BVH build of a process, nothing afterwards)
  hipStream_t ws = nullptr;
  void* wd = nullptr;
  std::vector<char> wh(256 << 10);   // (small: staged by the runtime; nothing of this library is page-locked in place)
  HIP_TRY(hipStreamCreateWithFlags(&ws, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&wd, 8 << 20));
  HIP_TRY(hipMemcpyAsync(wd, wh.data(), wh.size(), hipMemcpyHostToDevice, ws));
  HIP_TRY(hipMemsetAsync(static_cast<char*>(wd) + (4 << 20), 0, 1 << 16, ws));
  HIP_TRY(hipMemcpyAsync(wh.data(), wd, wh.size(), hipMemcpyDeviceToHost, ws));
  HIP_TRY(hipStreamSynchronize(ws));
  HIP_TRY(hipFree(wd));
  HIP_TRY(hipStreamDestroy(ws));
  StagingCache::prime(6);   // page-locked staging blocks for the scene uploads (staging.hpp): 6 x 8 MiB, once
  {  // the device's four hardware queues (~5 ms each to create, then pooled): four streams alive at once make them all
    hipStream_t q[4] = {};
    for (hipStream_t& x : q)
      if (hipStreamCreateWithFlags(&x, hipStreamNonBlocking) != hipSuccess) x = nullptr;
    for (hipStream_t x : q)
      if (x) (void)hipStreamDestroy(x);
    (void)hipGetLastError();
  }
  if (!build_on_host) warm_device_builder(device);
  warmed.push_back(device);
  return RAYCA_OK;
}

// a sphere's record in the sphere table
DevSphere dev_sphere(const HostPrim& p, const Trs& t) {
  DevSphere d;
  std::memset(&d, 0, sizeof d);
  d.center[0] = p.center.x; d.center[1] = p.center.y; d.center[2] = p.center.z; d.center[3] = p.center.w;
  d.radius2 = p.radius * p.radius;  // Sphere::new  sphere.rs:51-62
  const F4 iq = quat_conj(t.rotation), is = reciprocal(t.scale);
  const float* src[5] = {&t.translation.x, &t.rotation.x, &t.scale.x, &iq.x, &is.x};
  float* dst[5] = {d.translation, d.rotation, d.scale, d.inv_rotation, d.inv_scale};
  for (int a = 0; a < 5; ++a) std::memcpy(dst[a], src[a], 16);
  const Mat4 inv = mat4_from_inverse_trs(t);
  std::memcpy(d.inv_mat4, inv.m, 64);
  const Mat3 nm = mat3_transpose(mat3_from_inverse_trs(t));
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) d.normal_mat[4 * r + c] = nm.m[r][c];
  return d;
}

// The per-primitive device arrays -- world-space triangles (9 floats per slot, 36-B stride), shading records (256 B per
// slot, two lines: host_scene.hpp), the sphere table -- are final, in FLATTEN order, before any BVH work starts:
// build_host_scene calls back then, and a thread of its own packs and uploads them (~100 MB for the atrium) under the
// BVH build, straight from the arrays the flatten threads wrote.  Once the primitive order is known (second call-back)
// one gather kernel puts them into slot order.
struct PrimUpload {
  RaycaScene* s = nullptr;
  int device = 0;
  std::thread thread;
  int32_t rc = RAYCA_OK;
  std::string err;
  hipStream_t stream = nullptr;
  std::vector<DevSphere> spheres;
  float *d_tris = nullptr, *d_tris_flat = nullptr;
  PrimExt *d_ext = nullptr, *d_ext_flat = nullptr;
  uint32_t* d_order = nullptr;
  DevSphere* d_spheres = nullptr;
  size_t tri_bytes = 0, ext_bytes = 0, sphere_bytes = 0;
  bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    if (rc == RAYCA_OK) {
      rc = e == hipErrorOutOfMemory ? RAYCA_ERR_OOM : RAYCA_ERR_HIP;
      err = std::string(what) + ": " + hipGetErrorString(e);
    }
    return false;
  }
  void release_temporaries() {
    if (thread.joinable()) thread.join();
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : {static_cast<void*>(d_tris_flat), static_cast<void*>(d_ext_flat), static_cast<void*>(d_order)})
      if (p) (void)hipFree(p);
    d_tris_flat = nullptr; d_ext_flat = nullptr; d_order = nullptr;
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }
  void pack_and_upload();     // on its own thread, from build_host_scene's first call-back
  void gather_into_order();   // second call-back (the building thread): the primitive order is final
};

void PrimUpload::pack_and_upload() {
  HostScene& h = s->host;   // (h.ext and h.tris are this thread's until the second call-back joins it)
  const uint32_t P = (uint32_t)h.prims.size();
  if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return;
  if (h.ext.size() != P || h.tris.size() != (size_t)P * 9) { rc = RAYCA_ERR_BAD_ARG; err = "flatten arrays out of step"; return; }
  for (uint32_t i = 0; h.sphere_count && i < P; ++i) {   // the sphere table, numbered in flatten order
    const HostPrim& p = h.prims[i];
    if (p.kind != RAYCA_GEOMETRY_SPHERE) continue;
    const uint32_t sid = (uint32_t)spheres.size();
    spheres.push_back(dev_sphere(p, h.world_trs[p.node]));
    float* tv = &h.tris[(size_t)i * 9];   // a sphere's triangle slot: NaN, then its table index
    std::memset(tv, 0, 36);
    const uint32_t nan_bits = 0x7FC00000u;
    std::memcpy(&tv[0], &nan_bits, 4);
    std::memcpy(&tv[1], &sid, 4);
    h.ext[i].node = sid;  // sphere table index for the shading path
  }
  tri_bytes = sizeof(float) * kTriFloats * std::max<size_t>(P, 1);             // slot order: 48-B primitive records
  const size_t tri_flat_bytes = sizeof(float) * std::max<size_t>(h.tris.size(), 1);   // flatten order: nine floats each
  ext_bytes = sizeof(PrimExt) * std::max<size_t>(h.ext.size(), 1);
  sphere_bytes = sizeof(DevSphere) * std::max<size_t>(spheres.size(), 1);
  if (!hip_ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate")) return;
  void* p = nullptr;
  if (!hip_ok(hipMalloc(&p, tri_bytes), "hipMalloc(triangles)")) return;
  d_tris = static_cast<float*>(p);
  if (!hip_ok(hipMalloc(&p, ext_bytes), "hipMalloc(shading records)")) return;
  d_ext = static_cast<PrimExt*>(p);
  if (!hip_ok(hipMalloc(&p, sphere_bytes), "hipMalloc(spheres)")) return;
  d_spheres = static_cast<DevSphere*>(p);
  if (!hip_ok(hipMalloc(&p, tri_flat_bytes), "hipMalloc(triangles, flatten order)")) return;
  d_tris_flat = static_cast<float*>(p);
  if (!hip_ok(hipMalloc(&p, ext_bytes), "hipMalloc(shading records, flatten order)")) return;
  d_ext_flat = static_cast<PrimExt*>(p);
  if (!hip_ok(hipMalloc(&p, sizeof(uint32_t) * std::max<size_t>(P, 1)), "hipMalloc(primitive order)")) return;
  d_order = static_cast<uint32_t*>(p);
  // straight from the arrays the flatten threads wrote
  StagedCopier staged;   // (through page-locked staging blocks: staging.hpp)
  if (P && !hip_ok(staged.copy(d_tris_flat, h.tris.data(), sizeof(float) * h.tris.size(), stream), "copy(triangles)")) return;
  if (P && !hip_ok(staged.copy(d_ext_flat, h.ext.data(), sizeof(PrimExt) * h.ext.size(), stream), "copy(shading records)")) return;
  if (!spheres.empty() && !hip_ok(staged.copy(d_spheres, spheres.data(), sizeof(DevSphere) * spheres.size(), stream), "copy(spheres)")) return;
  (void)hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize(primitive upload)");
  staged.finish();
}

void PrimUpload::gather_into_order() {
  if (thread.joinable()) thread.join();
  if (rc != RAYCA_OK) return;
  const HostScene& h = s->host;
  const uint32_t P = (uint32_t)h.prim_order.size();
  if (P == 0) return;
  if (P != (uint32_t)h.prims.size()) { rc = RAYCA_ERR_BAD_ARG; err = "primitive order does not cover the primitives"; return; }
  if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return;
  {
    StagedCopier staged;
    if (!hip_ok(staged.copy(d_order, h.prim_order.data(), sizeof(uint32_t) * P, stream), "copy(primitive order)")) return;
  }
  hipLaunchKernelGGL(k_gather_prims, dim3((uint32_t)(((size_t)P * 16 + 255) / 256)), dim3(256), 0, stream, d_order, d_tris_flat,
                     reinterpret_cast<const uint4*>(d_ext_flat), d_tris, reinterpret_cast<uint4*>(d_ext), P);
  (void)hip_ok(hipGetLastError(), "k_gather_prims");
}

// What the steps of one rayca_hip_scene_create share.  A step returns RAYCA_OK or a code with last_error set; the driver
// alone cleans up (abandon).
struct SceneBuild {
  RaycaScene* s = nullptr;
  const RaycaSceneDesc* desc = nullptr;
  const RaycaConfig* cfg = nullptr;
  const RaycaBuildOptions* opts = nullptr;
  uint32_t builder = RAYCA_BUILDER_REFERENCE;
  int device = 0;
  PrimUpload pu;
  std::string err;
  std::chrono::steady_clock::time_point t_init, t0;   // before the warm-up (runtime_init_ms), before the build (build_ms)
  std::vector<DevMaterial> mats;   // the small tables: made (and checked) by prepare_tables, uploaded by upload_tables
  std::vector<DevTexture> texs;
  std::vector<DevLight> lights;
  bool build_on_host() const { return opts && opts->build_on_host; }
};

// (device-built trees still held on the device, all owned by host.dev_trees: released by upload_binary_nodes once every
// segment is written, or by abandon on every other way out)
void release_device_trees(RaycaScene* s) {
  for (KeptTree* t : s->host.dev_trees) gpu_release_tree(t);
  s->host.dev_trees.clear();
  for (HostBlas& bl : s->host.blas) bl.dev_tree = nullptr;
  for (DeviceSegment& seg : s->host.dev_segments) seg.tree = nullptr;
}

// The one way out of a scene_create that has failed after `new RaycaScene()`.
int32_t abandon(SceneBuild& b, int32_t rc) {
  release_device_trees(b.s);
  rayca_hip_scene_destroy(b.s);
  return rc;
}

// Flatten, build the BLASes and the TLAS (build_host_scene) with the primitive upload under it; on return the slot-order
// primitive arrays are complete on the device and booked.
int32_t build_trees(SceneBuild& b) {
  RaycaScene* s = b.s;
  PrimUpload& pu = b.pu;
  const int device = b.device;
  BuildHooks hooks;
  // (the scene's streams -- builder's and frame contexts' -- are made by a thread of their own while the host flattens)
  std::thread streams_thread([s, device] {
    if (hipSetDevice(device) == hipSuccess) make_scene_streams(s, false);
    (void)hipGetLastError();
    s->build_streams_ready.store(1, std::memory_order_release);   // (whatever happened: nobody waits for ever)
  });
  hooks.on_prims_ready = [&] {
    // (the builders' streams: made first by the streams thread, which goes on with the frame contexts' while the trees are built)
    while (streams_thread.joinable() && !s->build_streams_ready.load(std::memory_order_acquire)) std::this_thread::yield();
    pu.thread = std::thread([&pu] { pu.pack_and_upload(); });
  };
  hooks.build_streams = reinterpret_cast<void* const*>(s->build_streams);
  hooks.on_order_ready = [&pu] { pu.gather_into_order(); };
  hooks.with_formats = false;
  const int32_t rc = build_host_scene(*b.desc, b.cfg ? b.cfg->bvh != 0 : true, b.builder, s->host, b.err, hooks);
  if (streams_thread.joinable()) streams_thread.join();   // (a build that failed before its first call-back)
  pu.release_temporaries();   // (joins the thread and drains the stream: the slot-order arrays are complete)
  for (void* p : {static_cast<void*>(pu.d_tris), static_cast<void*>(pu.d_ext), static_cast<void*>(pu.d_spheres)})
    if (p) s->allocations.push_back(p);
  s->device_bytes += pu.tri_bytes + pu.ext_bytes + pu.sphere_bytes;
  if (rc != RAYCA_OK) return fail(rc, b.err);
  if (pu.rc != RAYCA_OK) return fail(pu.rc, pu.err);
  return RAYCA_OK;
}

// The material, texture and light tables as the device holds them; a texture without a usable image is refused here.
int32_t prepare_tables(SceneBuild& b) {
  RaycaScene* s = b.s;
  const int device = b.device;
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  s->cu_count = prop.multiProcessorCount;
  const HostScene& h = s->host;
  b.mats = dev_materials(h.materials.data(), h.materials.size());
  b.texs.resize(h.textures.size());
  for (size_t i = 0; i < b.texs.size(); ++i) {
    const uint32_t im = h.textures[i].image;
    if (im >= h.images.size()) return fail(RAYCA_ERR_BAD_ARG, "texture references a missing image");
    b.texs[i] = DevTexture{h.images[im].width, h.images[im].height, h.images[im].color_type, 0, h.images[im].byte_offset};
    if (b.texs[i].width == 0 || b.texs[i].height == 0) return fail(RAYCA_ERR_BAD_ARG, "empty texture image");
  }
  b.lights = dev_lights(h.lights);
  return RAYCA_OK;
}

// binary nodes: what the host laid out is copied, the runs of device-built BLASes are written in place by the device
// from the trees it still holds (gpu_emit_tree, bvh_build.hip) -- the finished tree never travels to the host and back
int32_t upload_binary_nodes(SceneBuild& b) {
  RaycaScene* s = b.s;
  const HostScene& h = s->host;
  const size_t count = h.dev_nodes.size(), bytes = sizeof(DevNode) * (count ? count : 1);
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, bytes));
  s->allocations.push_back(p);
  s->device_bytes += bytes;
  DevNode* dnodes = static_cast<DevNode*>(p);
  std::vector<DeviceSegment> segs = h.dev_segments;
  std::sort(segs.begin(), segs.end(), [](const DeviceSegment& l, const DeviceSegment& r) { return l.first < r.first; });
  size_t at = 0;
  StagedCopier node_copier;
  for (size_t i = 0; i <= segs.size(); ++i) {   // the runs between the segments
    const size_t end = i < segs.size() ? segs[i].first : count;
    if (end > at) {   // (through the staging blocks: no copy of this library lets the runtime page-lock heap memory in place)
      HIP_TRY(node_copier.copy(dnodes + at, h.dev_nodes.data() + at, sizeof(DevNode) * (end - at), nullptr));
    }
    if (i < segs.size()) at = (size_t)segs[i].first + segs[i].count;
  }
  HIP_TRY(hipStreamSynchronize(nullptr));
  node_copier.finish();
  for (const DeviceSegment& seg : h.dev_segments) {
    std::string lerr;
    if (!gpu_emit_tree(seg.tree, dnodes, seg.first, seg.prim_base, h.pad_rel, h.pad_abs, lerr)) return fail(RAYCA_ERR_HIP, lerr);   // (abandon releases the trees)
  }
  release_device_trees(s);
  s->dev.nodes = reinterpret_cast<const float4*>(dnodes);
  return RAYCA_OK;
}

// RAYCA_NODE_CH: the conservative centre / half-extent copy of the binary nodes (k_make_ch_nodes), made on the device
int32_t make_ch_nodes(SceneBuild& b) {
  RaycaScene* s = b.s;
  s->dev.nodes_ch = nullptr;
#if RAYCA_NODE_CH
  const HostScene& h = s->host;
  if (!h.dev_nodes.empty() && !h.ref_leaf_of.empty()) {   // (the kernels that steer by conservative boxes: RAYCA_BUILDER_SAH scenes)
    if ((uint64_t)h.dev_nodes.size() * kChRefScale >= 0x7FFFFFFEull) return fail(RAYCA_ERR_BAD_ARG, "too many BVH nodes for 31-bit node references");
    void* p = nullptr;
    const size_t ch_bytes = 16u * kChNodeQuads * h.dev_nodes.size();
    HIP_TRY(hipMalloc(&p, ch_bytes));
    s->allocations.push_back(p);
    s->device_bytes += ch_bytes;
    hipLaunchKernelGGL(k_make_ch_nodes, dim3(((uint32_t)h.dev_nodes.size() + 255u) / 256u), dim3(256), 0, nullptr,
                       reinterpret_cast<const DevNode*>(s->dev.nodes), p, (uint32_t)h.dev_nodes.size());
    HIP_TRY(hipGetLastError());
    s->dev.nodes_ch = static_cast<const float4*>(p);
  }
#endif
  return RAYCA_OK;
}

// The remaining tables and the scalars of DevScene; on return everything a frame on the binary f32 nodes needs is on the device.
int32_t upload_tables(SceneBuild& b) {
  RaycaScene* s = b.s;
  const PrimUpload& pu = b.pu;
  const HostScene& h = s->host;
  const uint32_t P = (uint32_t)h.prim_order.size();
  DevScene& dv = s->dev;
  int32_t rc;
  dv.nodes4 = nullptr;   // the other three formats: dev_full, formats_thread_body
  dv.root_ref4 = 0;
  dv.nodes_h = dv.nodes4_h = nullptr;
  dv.tris = reinterpret_cast<const float4*>(pu.d_tris);   // assembled and uploaded by the primitive upload's thread
  dv.ext = pu.d_ext;
  dv.tie_rank = nullptr;
  if (!h.tie_rank.empty() && (rc = upload(s, h.tie_rank.data(), h.tie_rank.size(), &dv.tie_rank)) != RAYCA_OK) return rc;
  dv.ref_leaf_of = nullptr;
  dv.ref_leaf_boxes = nullptr;
  if (!h.ref_leaf_of.empty()) {
    const float* boxes = nullptr;
    if ((rc = upload(s, h.ref_leaf_of.data(), h.ref_leaf_of.size(), &dv.ref_leaf_of)) != RAYCA_OK) return rc;
    if ((rc = upload(s, h.ref_leaf_boxes.data(), h.ref_leaf_boxes.size(), &boxes)) != RAYCA_OK) return rc;
    dv.ref_leaf_boxes = reinterpret_cast<const float4*>(boxes);
  }
  if ((rc = upload(s, b.mats.data(), b.mats.size(), &dv.materials)) != RAYCA_OK) return rc;
  if ((rc = upload(s, b.lights.data(), b.lights.size(), &dv.lights)) != RAYCA_OK) return rc;
  dv.spheres = pu.d_spheres;
  if ((rc = upload(s, b.texs.data(), b.texs.size(), &dv.textures)) != RAYCA_OK) return rc;
  if ((rc = upload(s, h.image_bytes.data(), h.image_bytes.size(), &dv.image_bytes)) != RAYCA_OK) return rc;
  dv.material_count = (uint32_t)b.mats.size();
  dv.light_count = (uint32_t)b.lights.size();
  dv.texture_count = (uint32_t)b.texs.size();
  dv.prim_count = P;
  dv.root_ref = h.root_ref;
  dv.root_ref_ch = dv.nodes_ch ? ch_ref(h.root_ref) : h.root_ref;
  dv.root_min[0] = h.root_min.x; dv.root_min[1] = h.root_min.y; dv.root_min[2] = h.root_min.z;
  dv.root_max[0] = h.root_max.x; dv.root_max[1] = h.root_max.y; dv.root_max[2] = h.root_max.z;
  {
    const float dx = h.root_max.x - h.root_min.x, dy = h.root_max.y - h.root_min.y, dz = h.root_max.z - h.root_min.z;
    const float diag = sqrtf(dx * dx + dy * dy + dz * dz);
    dv.cull_abs = (diag == diag && diag < FLT_MAX) ? diag * 9.765625e-4f : 0.0f;
  }
  dv.reserved = 0;
  if (P && (dv.tie_rank || dv.ref_leaf_of)) {   // the filter fields of the primitive records, from the tables just uploaded
    hipLaunchKernelGGL(k_fill_tri_filter, dim3((P + 255u) / 256u), dim3(256), 0, nullptr, pu.d_tris, dv.tie_rank, dv.ref_leaf_of, P);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipDeviceSynchronize());
  s->dev_full = s->dev;
  s->node_count = (uint32_t)s->host.dev_nodes.size();
  s->prim_count = (uint32_t)s->host.prims.size();
  return RAYCA_OK;
}

void drop_flatten_arrays(HostScene& h) {   // on the device now; ~100 MB of host memory the scene has no further use for
  std::vector<PrimExt, DefaultInitAllocator<PrimExt>>().swap(h.ext);
  std::vector<float, DefaultInitAllocator<float>>().swap(h.tris);
}
// and, once the other node formats have been made from them, the flatten-order primitives, the host copies of the node
// arrays and the filter tables (another ~150 MB for the atrium): everything a frame needs is on the device, what the
// entry points report is kept in counts, the primitive order stays
void drop_host_bulk(HostScene& h) {
  std::vector<HostPrim, DefaultInitAllocator<HostPrim>>().swap(h.prims);
  std::vector<DevNode, DefaultInitAllocator<DevNode>>().swap(h.dev_nodes);
  std::vector<DevNode4>().swap(h.dev_nodes4);
  std::vector<DevNodeH, DefaultInitAllocator<DevNodeH>>().swap(h.dev_nodes_h);
  std::vector<DevNode4H, DefaultInitAllocator<DevNode4H>>().swap(h.dev_nodes4_h);
  std::vector<uint32_t>().swap(h.tie_rank);
  std::vector<uint32_t>().swap(h.ref_leaf_of);
  std::vector<float>().swap(h.ref_leaf_boxes);
  for (HostBlas& bl : h.blas) std::vector<BuildNode>().swap(bl.nodes);
}

// 4-wide nodes and the fp16 copies: made and uploaded next to the first frames, which traverse the binary f32 nodes
// meanwhile (same pixels with every format).  The scene's formats thread runs this.
void formats_thread_body(RaycaScene* s, int device) {
  const auto f0 = std::chrono::steady_clock::now();
  drop_flatten_arrays(s->host);   // (here rather than on the caller's thread: unmapping them takes a millisecond or two)
  auto failed = [s](int32_t code, const std::string& what) {
    s->formats_rc = code;
    s->formats_err = what;
    s->formats_state.store(-1, std::memory_order_release);
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return failed(RAYCA_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  HostScene& h = s->host;
  // the 4-wide collapse and the fp16 copies are made on the host from the binary nodes: fetch the runs the device wrote
  auto cancelled = [s, &failed] {
    if (!s->formats_cancel.load(std::memory_order_relaxed)) return false;
    failed(RAYCA_ERR_BAD_ARG, "scene destroyed while its node formats were being made");
    return true;
  };
  if (cancelled()) return;
  hipStream_t up = nullptr;   // (not the null stream: that one would order itself against the caller's streams)
  if ((e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking)) != hipSuccess) return failed(RAYCA_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  StagedCopier staged;   // (both directions through the page-locked staging blocks: staging.hpp)
  if (!h.dev_segments.empty() && !h.dev_nodes.empty() &&
      (e = staged.copy_back(h.dev_nodes.data(), s->dev.nodes, sizeof(DevNode) * h.dev_nodes.size(), up)) != hipSuccess) {
    (void)hipStreamDestroy(up);
    return failed(RAYCA_ERR_HIP, std::string("node download: ") + hipGetErrorString(e));
  }
  if (!cancelled()) finish_node_formats(h, &s->formats_cancel);
  if (cancelled()) {
    staged.finish();
    (void)hipStreamDestroy(up);
    return;
  }
  auto put = [&](const void* src, size_t bytes, const void** dst) {
    void* p = nullptr;
    if ((e = hipMalloc(&p, bytes ? bytes : 16)) != hipSuccess) return false;
    s->formats_allocations.push_back(p);
    s->formats_bytes += bytes ? bytes : 16;
    if (bytes && (e = staged.copy(p, src, bytes, up)) != hipSuccess) return false;
    *dst = p;
    return true;
  };
  const void *d4 = nullptr, *dh = nullptr, *d4h = nullptr;
  const bool ok = put(h.dev_nodes4.data(), h.dev_nodes4.size() * sizeof(DevNode4), &d4) &&
                  put(h.dev_nodes_h.data(), h.dev_nodes_h.size() * sizeof(DevNodeH), &dh) &&
                  put(h.dev_nodes4_h.data(), h.dev_nodes4_h.size() * sizeof(DevNode4H), &d4h) &&
                  (e = hipStreamSynchronize(up)) == hipSuccess;
  if (!ok) (void)hipStreamSynchronize(up);   // (nothing of a failed upload may still be reading a staging block)
  staged.finish();
  (void)hipStreamDestroy(up);
  if (!ok) return failed(e == hipErrorOutOfMemory ? RAYCA_ERR_OOM : RAYCA_ERR_HIP, std::string("node formats: ") + hipGetErrorString(e));
  DevScene& full = s->dev_full;
  full.nodes4 = static_cast<const float4*>(d4);
  full.root_ref4 = h.root_ref4;
  full.nodes_h = static_cast<const uint4*>(dh);
  full.nodes4_h = static_cast<const uint4*>(d4h);
  for (int c = 0; c < 3; ++c) full.half_center[c] = h.half_center[c];
  full.half_inv_scale = 1.0f / h.half_scale;
  s->formats_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - f0).count();
  if (getenv("RAYCA_BUILD_TIMING")) fprintf(stderr, "[rayca build] %-28s %8.1f ms (on their own thread)\n", "other node formats + upload", s->formats_ms);
  s->formats_state.store(1, std::memory_order_release);
  drop_host_bulk(s->host);
}

// RAYCA_SYNC_FORMATS=1 waits for the thread here instead.
int32_t start_formats_thread(RaycaScene* s, int device) {
  s->formats_state.store(0, std::memory_order_release);
  s->formats_thread = std::thread(formats_thread_body, s, device);
  static const bool sync_formats = getenv("RAYCA_SYNC_FORMATS") != nullptr;
  return sync_formats ? formats_wait(s) : RAYCA_OK;
}

// Frame context 0's stream, events and counters -- and with it the frame contexts' streams of this scene (13-16 ms inside
// the first render call otherwise: creating a stream is most of it) -- on a thread of the scene's, from here on: it is
// frame set-up, not scene build, and it used to sit on the build's critical path in a process's first scene (the upload
// thread did it and the build waited for that thread).  A first frame that comes at once waits for it on the context's
// mutex; a failure is left to that frame to report.
void start_ctx_thread(RaycaScene* s) {
  s->ctx_thread = std::thread([s] {
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return; }
    std::lock_guard<std::mutex> lock(s->ctx[0].mu);
    if (ensure_ctx(s, &s->ctx[0]) != RAYCA_OK) (void)hipGetLastError();
  });
}

}  // namespace

extern "C" {

int32_t rayca_hip_scene_create(const RaycaSceneDesc* desc, const RaycaConfig* cfg, const RaycaBuildOptions* opts, RaycaScene** out) {
  if (!desc || !out) return fail(RAYCA_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  // what no scene may hold, refused before any device call: a kernel samples a texture with nothing but `% width` between a UV and an
  // address, so an image whose texels end beyond image_bytes would be read past the allocation
  if (std::string err; desc_validate(*desc, err) != RAYCA_OK) return fail(RAYCA_ERR_BAD_ARG, err);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(RAYCA_ERR_NO_DEVICE, "no HIP device visible: librayca_hip has no CPU fallback");
  const uint32_t builder = opts ? opts->builder : RAYCA_BUILDER_REFERENCE;
  if (builder != RAYCA_BUILDER_REFERENCE && builder != RAYCA_BUILDER_SAH) return fail(RAYCA_ERR_BAD_ARG, "unknown builder");
  (void)rayca_hip_scene_reap();   // scenes destroyed since: their memory is back before this one allocates (nothing to wait for, as a rule)
  const int device = opts ? (int)opts->device : 0;
  if (device >= ndev) return fail(RAYCA_ERR_BAD_ARG, "device ordinal out of range");
  SceneBuild b;
  b.desc = desc;
  b.cfg = cfg;
  b.opts = opts;
  b.builder = builder;
  b.device = device;
  // The first HIP call of a process on a device creates its context and loads the code object (~0.2 s): paid once per
  // process, not per scene, so it is timed on its own (RaycaSceneInfo.runtime_init_ms) and not booked under build_ms.
  b.t_init = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(device));
  int32_t rc = warm_device(device, b.build_on_host());
  if (rc != RAYCA_OK) return rc;
  b.t0 = std::chrono::steady_clock::now();
  RaycaScene* s = new RaycaScene();
  b.s = b.pu.s = s;
  b.pu.device = device;
  s->device = device;
  if (const char* e = getenv("RAYCA_NEE_SKIP")) s->nee_skip = atoi(e) != 0;
  s->counts.node_count = desc->node_count;
  s->counts.mesh_count = desc->mesh_count;
  s->counts.primitive_count = desc->primitive_count;
  s->counts.vertex_count = desc->vertex_count;
  s->counts.index_byte_count = desc->index_byte_count;
  s->counts.material_count = desc->material_count;
  s->counts.texture_count = desc->texture_count;
  s->counts.image_count = desc->image_count;
  s->counts.image_byte_count = desc->image_byte_count;
  s->counts.camera_count = desc->camera_count;
  s->counts.light_count = desc->light_count;
  s->runtime_init_ms = std::chrono::duration<float, std::milli>(b.t0 - b.t_init).count();
  set_device_blas_builder(b.build_on_host() ? nullptr : &gpu_build_blas, (uint32_t)device);
  // every way out from here on goes through abandon
  if ((rc = build_trees(b)) != RAYCA_OK) return abandon(b, rc);
  if ((rc = prepare_tables(b)) != RAYCA_OK) return abandon(b, rc);
  if ((rc = upload_binary_nodes(b)) != RAYCA_OK) return abandon(b, rc);
  if ((rc = make_ch_nodes(b)) != RAYCA_OK) return abandon(b, rc);
  if ((rc = upload_tables(b)) != RAYCA_OK) return abandon(b, rc);
  if (!s->host.other_formats_wanted) {
    drop_flatten_arrays(s->host);
    drop_host_bulk(s->host);
  } else if ((rc = start_formats_thread(s, device)) != RAYCA_OK) {
    return abandon(b, rc);
  }
  if (getenv("RAYCA_BUILD_TIMING"))
    fprintf(stderr, "[rayca build] %-28s %8.1f ms (whole scene_create so far)\n", "device arrays + upload",
            std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - b.t0).count());
  s->build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - b.t0).count();
  start_ctx_thread(s);   // (last, and after build_ms is taken: frame set-up, not scene build)
  *out = s;
  return RAYCA_OK;
}

}  // extern "C"

namespace {

// rayca_hip_scene_destroy hands the scene to a thread of the library and returns: joining the formats thread, waiting for
// the scene's last frames and two dozen hipFree / hipStreamDestroy calls took 7-27 ms, which a host that rebuilds the scene
// for every frame (the literal draw(): scene.rs:90-99) paid on its own thread per frame.  The threads are joined when the
// next scene is created (so that at most one scene's memory is ever waiting to be released when a new one is allocated),
// by rayca_hip_scene_reap, and when the library is unloaded.
struct Reaper {
  std::mutex mu;
  std::vector<std::thread> threads;
  void add(std::thread t) {
    std::lock_guard<std::mutex> lock(mu);
    threads.push_back(std::move(t));
  }
  void drain() {
    std::vector<std::thread> mine;
    {
      std::lock_guard<std::mutex> lock(mu);
      mine.swap(threads);
    }
    for (std::thread& t : mine)
      if (t.joinable()) t.join();
  }
  ~Reaper() { drain(); }
};
Reaper& reaper() {
  static Reaper r;
  return r;
}

int32_t scene_destroy_now(RaycaScene* s);

}  // namespace

extern "C" {

int32_t rayca_hip_scene_destroy(RaycaScene* s) {
  if (!s) return RAYCA_OK;
  s->formats_cancel.store(true, std::memory_order_relaxed);   // (nobody will use them: the thread stops at its next phase boundary)
  static const bool synchronous = getenv("RAYCA_SYNC_DESTROY") != nullptr;
  if (synchronous) return scene_destroy_now(s);
  reaper().add(std::thread([s] { (void)scene_destroy_now(s); }));
  return RAYCA_OK;
}

int32_t rayca_hip_scene_reap(void) {
  reaper().drain();
  return RAYCA_OK;
}

}  // extern "C"

namespace {

int32_t scene_destroy_now(RaycaScene* s) {
  Lap lap("destroy", 26, 2);
  if (s->ctx_thread.joinable()) s->ctx_thread.join();
  {
    s->formats_cancel.store(true, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lock(s->formats_mu);
    if (s->formats_thread.joinable()) s->formats_thread.join();
  }
  lap("formats thread");
  (void)hipSetDevice(s->device);
  // the scene's last frames: every frame records its context's ev_done on the stream it ran on (the caller's or the
  // context's own); the builders' streams are idle since scene_create returned
  for (FrameCtx& cx : s->ctx) {
    std::lock_guard<std::mutex> lock(cx.mu);
    if (cx.frame_pending && cx.ev_done) (void)hipEventSynchronize(cx.ev_done);
    if (cx.stream) (void)hipStreamSynchronize(cx.stream);
  }
  for (uint32_t c = 0; c < kMaxContexts; ++c)   // frames of the several-devices entry still in flight (this scene assembling them)
    if (s->multi.frames[c].pending && s->multi.frames[c].gathered) (void)hipEventSynchronize(s->multi.frames[c].gathered);
  lap("last frames");
  s->multi.release();
  for (void* p : s->allocations) (void)hipFree(p);
  for (void* p : s->formats_allocations) (void)hipFree(p);
  // the streams go to the next scene on this device (make_scene_streams) if their set is complete and there is room
  bool keep_streams = s->streams_made == 2;
  for (hipStream_t b : s->build_streams) keep_streams = keep_streams && b != nullptr;
  for (FrameCtx& cx : s->ctx) keep_streams = keep_streams && cx.stream != nullptr;
  if (keep_streams) {
    for (hipStream_t b : s->build_streams) keep_streams = keep_streams && hipStreamSynchronize(b) == hipSuccess;
    StreamSetPool& pool = stream_set_pool();
    std::lock_guard<std::mutex> plock(pool.mu);
    std::vector<StreamSet>& kept = pool.sets[s->device];
    if (keep_streams && kept.size() < kStreamSetsKept) {
      StreamSet set;
      for (int i = 0; i < 2; ++i) set.build[i] = s->build_streams[i];
      for (uint32_t i = 0; i < kMaxContexts; ++i) set.ctx[i] = s->ctx[i].stream;
      kept.push_back(set);
      // handed over: the scene and its contexts no longer own them
      for (hipStream_t& b : s->build_streams) b = nullptr;
      for (FrameCtx& cx : s->ctx) cx.stream = nullptr;
    }
  }
  (void)hipGetLastError();
  for (hipStream_t b : s->build_streams)   // (what was not handed over)
    if (b) (void)hipStreamDestroy(b);
  for (FrameCtx& cx : s->ctx) cx.release();   // here and not inside `delete s`: device memory is this lap's
  lap("device memory, streams");
  delete s;
  lap("host memory");
  return RAYCA_OK;
}

}  // namespace

extern "C" {

int32_t rayca_hip_scene_finish(RaycaScene* s) {
  if (!s) return fail(RAYCA_ERR_BAD_ARG, "null scene");
  return formats_wait(s);
}

int32_t rayca_hip_scene_info(const RaycaScene* s, RaycaSceneInfo* out) {
  if (!s || !out) return fail(RAYCA_ERR_BAD_ARG, "null argument");
  std::memset(out, 0, sizeof *out);
  out->triangle_count = s->host.triangle_count;
  out->sphere_count = s->host.sphere_count;
  out->blas_count = (uint32_t)s->host.blas.size();
  out->node_count = s->node_count;
  out->max_depth = s->host.max_depth;
  out->light_count = (uint32_t)s->host.lights.size();
  out->device_bytes = s->device_bytes + (formats_ready(s) ? s->formats_bytes : 0u);
  out->build_ms = s->build_ms;
  out->runtime_init_ms = s->runtime_init_ms;
  return RAYCA_OK;
}

// The camera of a frame in the form a reprojection reads it (rayca_hip_accumulate_device): the origin as camera_ray forms it
// from the camera node's world transform, and the rows of (R S)^-1 = S^-1 R^T -- rotate(e_k, rotation) / scale.k -- so that for
// a point x on the ray through (xx, yy, -1), right . (x - origin) = s xx, up . = s yy, back . = -s.  Host only.
int32_t rayca_hip_scene_camera(const RaycaScene* s, RaycaCameraPose* out) {
  if (!s || !out) return fail(RAYCA_ERR_BAD_ARG, "null scene or camera pose");
  if (!s->host.has_camera) return fail(RAYCA_ERR_NO_CAMERA, "scene has no camera (scene.rs:109)");
  const Trs& t = s->host.world_trs[s->host.camera_node];
  std::memset(out, 0, sizeof *out);
  F4 origin = point_rotate(point_scale(point3(0.0f, 0.0f, 0.0f), t.scale), t.rotation);   // (camera_ray: Ray::scale, ::rotate, ::translate)
  origin.w = 1.0f;
  origin = origin + t.translation;
  out->origin[0] = origin.x; out->origin[1] = origin.y; out->origin[2] = origin.z;
  out->angle = tanf(s->host.camera_yfov * 0.5f);   // (camera_frame_params)
  const F4 r = rotate(vec3(1.0f, 0.0f, 0.0f), t.rotation), u = rotate(vec3(0.0f, 1.0f, 0.0f), t.rotation), b = rotate(vec3(0.0f, 0.0f, 1.0f), t.rotation);
  out->right[0] = r.x / t.scale.x; out->right[1] = r.y / t.scale.x; out->right[2] = r.z / t.scale.x;
  out->up[0] = u.x / t.scale.y; out->up[1] = u.y / t.scale.y; out->up[2] = u.z / t.scale.y;
  out->back[0] = b.x / t.scale.z; out->back[1] = b.y / t.scale.z; out->back[2] = b.z / t.scale.z;
  return RAYCA_OK;
}

// What SceneDrawInfo::new reads again per draw (scene.rs:88-115) and leaves the BVH alone: the camera, the light table, the
// material table.  Everything is checked and computed first, into temporaries; a refused edit changes nothing.
//
// Lock order.  A frame context's mutex is taken for one context of one scene by the render calls, trace_rays, the thread that
// sets context 0 up and scene_destroy_now; for ONE context index across several scenes, in address order, by multi_issue
// (lock_contexts); and here for all eight contexts of ONE scene, in index order.  Every thread thus takes context mutexes in
// ascending (context index, scene address) order, so no cycle of waits can form.  multi_mu is taken before any context mutex
// (as multi_issue does), and no thread holds two of those.
int32_t rayca_hip_scene_update(RaycaScene* s, const RaycaSceneDesc* desc) {
  if (!s || !desc) return fail(RAYCA_ERR_BAD_ARG, "null scene or descriptor");
  const RaycaSceneDesc& d = *desc;
  if (d.abi_version != RAYCA_ABI_VERSION) return fail(RAYCA_ERR_BAD_ARG, "abi version mismatch");
  const RaycaSceneDesc& was = s->counts;
  if (d.node_count != was.node_count || d.mesh_count != was.mesh_count || d.primitive_count != was.primitive_count ||
      d.vertex_count != was.vertex_count || d.index_byte_count != was.index_byte_count || d.material_count != was.material_count ||
      d.texture_count != was.texture_count || d.image_count != was.image_count || d.image_byte_count != was.image_byte_count ||
      d.camera_count != was.camera_count || d.light_count != was.light_count)
    return fail(RAYCA_ERR_BAD_ARG, "an update keeps every count of the scene (a different count needs rayca_hip_scene_create)");
  if ((d.node_count && !d.nodes) || (d.material_count && !d.materials) || (d.camera_count && !d.cameras) || (d.light_count && !d.lights))
    return fail(RAYCA_ERR_BAD_ARG, "nodes, materials, cameras or lights is null");
  HostScene& h = s->host;
  for (uint32_t i = 0; i < d.node_count; ++i) {
    const RaycaNode &a = d.nodes[i], &b = h.nodes[i];
    if (a.parent != b.parent || a.model != b.model || a.mesh != b.mesh || a.camera != b.camera || a.light != b.light)
      return fail(RAYCA_ERR_BAD_ARG, "node " + std::to_string(i) + ": an update may change a node's trs only");
  }
  for (uint32_t i = 0; i < d.material_count; ++i) {
    const RaycaMaterial& m = d.materials[i];
    for (const uint32_t t : {m.albedo_texture, m.normal_texture, m.metallic_roughness_texture})
      if (t != RAYCA_NONE && t >= d.texture_count) return fail(RAYCA_ERR_BAD_ARG, "material " + std::to_string(i) + ": texture index out of range");
  }
  SceneGraph g;
  std::string err;
  if (const int32_t rc = scene_graph_pass(d, g, err); rc != RAYCA_OK) return fail(rc, err);
  if (g.lights.size() != h.lights.size()) return fail(RAYCA_ERR_BAD_ARG, "light nodes differ from the scene's");

  // ---- would it move geometry?  The BLASes hold world-space triangles: the meshes' and the quad lights' ----
  if (const int32_t rc = update_moves_geometry(d, g, h.world_trs, h.lights, err); rc != RAYCA_OK) return fail(rc, err);

  // ---- the device tables as scene_create would make them; which of them differ ----
  auto differ = [](const auto& a, const auto& b) { return a.size() != b.size() || (!a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof a[0]) != 0); };
  const std::vector<DevMaterial> mats = dev_materials(d.materials, d.material_count);
  const bool mats_changed = differ(mats, dev_materials(h.materials.data(), h.materials.size()));
  const std::vector<DevLight> lights = dev_lights(g.lights);
  const bool lights_changed = differ(lights, dev_lights(h.lights));

  // ---- apply ----
  const bool tables = mats_changed || lights_changed;
  std::unique_lock<std::mutex> multi_lock(s->multi_mu, std::defer_lock);
  if (tables) multi_lock.lock();
  std::unique_lock<std::mutex> ctx_locks[kMaxContexts];
  for (uint32_t c = 0; c < kMaxContexts; ++c) ctx_locks[c] = std::unique_lock<std::mutex>(s->ctx[c].mu);
  if (tables) {
    // the frames in flight read the tables that are about to be overwritten (as scene_destroy_now waits for them): every
    // frame records its context's ev_done behind its last kernel, and the gathers this scene assembles end with `gathered`
    HIP_TRY(hipSetDevice(s->device));
    for (FrameCtx& cx : s->ctx)
      if (cx.frame_pending && cx.ev_done) HIP_TRY(hipEventSynchronize(cx.ev_done));
    for (MultiFrame& f : s->multi.frames)
      if (f.gathered_valid && f.gathered) HIP_TRY(hipEventSynchronize(f.gathered));
    // in place: `dev` and `dev_full` (and every DevScene a frame takes by value) keep their pointers.  (A HIP error here
    // leaves the tables half written: the handle is then to be recreated.)
    StagedCopier staged;
    if (mats_changed) HIP_TRY(staged.copy(const_cast<DevMaterial*>(s->dev.materials), mats.data(), sizeof(DevMaterial) * mats.size(), nullptr));
    if (lights_changed) HIP_TRY(staged.copy(const_cast<DevLight*>(s->dev.lights), lights.data(), sizeof(DevLight) * lights.size(), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  // what render_body and generation_kernels_cover read (the camera travels to the kernels by value, in FrameParams)
  std::copy(g.local_trs.begin(), g.local_trs.end(), h.local_trs.begin());
  std::copy(g.world_trs.begin(), g.world_trs.end(), h.world_trs.begin());
  h.camera_yfov = g.camera_yfov;
  std::copy(g.lights.begin(), g.lights.end(), h.lights.begin());
  std::copy(d.materials, d.materials + d.material_count, h.materials.begin());
  return RAYCA_OK;
}

int32_t rayca_hip_scene_primitive_order(const RaycaScene* s, uint32_t* prim_order, uint32_t capacity) {
  if (!s || !prim_order) return fail(RAYCA_ERR_BAD_ARG, "null argument");
  if (capacity < s->host.prim_order.size()) return fail(RAYCA_ERR_BAD_ARG, "capacity too small");
  std::memcpy(prim_order, s->host.prim_order.data(), s->host.prim_order.size() * sizeof(uint32_t));
  return RAYCA_OK;
}

int32_t rayca_hip_scene_read_nodes(RaycaScene* s, uint32_t which, void* out, uint64_t capacity_bytes, uint64_t* bytes_out) {
  if (!s || which > 1u) return fail(RAYCA_ERR_BAD_ARG, "null scene or unknown node array");
  const void* src = which == 0u ? static_cast<const void*>(s->dev.nodes) : static_cast<const void*>(s->dev.nodes_ch);
  const uint64_t bytes = (uint64_t)s->node_count * (which == 0u ? sizeof(DevNode) : 16u * kChNodeQuads);
  if (!src || s->node_count == 0) return fail(RAYCA_ERR_BAD_ARG, "the scene has no such node array");
  if (bytes_out) *bytes_out = bytes;
  if (!out) return RAYCA_OK;
  if (capacity_bytes < bytes) return fail(RAYCA_ERR_BAD_ARG, "capacity too small");
  HIP_TRY(hipSetDevice(s->device));
  StagedCopier back;   // (through page-locked blocks, like every other copy of the library: staging.hpp)
  HIP_TRY(back.copy_back(out, src, bytes, nullptr));
  back.finish();
  return RAYCA_OK;
}

// The light table as the kernels read it, back from the device: what scene_create uploaded or the last rayca_hip_scene_update wrote.
// Every context is locked for the copy, as the update locks them, so that the table is never read half written.
int32_t rayca_hip_scene_read_lights(RaycaScene* s, RaycaLightRecord* out, uint32_t capacity, uint32_t* count_out) {
  if (!s) return fail(RAYCA_ERR_BAD_ARG, "null scene");
  if (!out && !count_out) return fail(RAYCA_ERR_BAD_ARG, "neither out nor count_out: nothing to read the lights into");
  const uint32_t n = s->dev.light_count;
  if (count_out) *count_out = n;
  if (!out) return RAYCA_OK;
  if (capacity < n) return fail(RAYCA_ERR_BAD_ARG, "capacity too small");
  if (n == 0) return RAYCA_OK;
  std::vector<DevLight> table(n);
  {
    std::unique_lock<std::mutex> ctx_locks[kMaxContexts];
    for (uint32_t c = 0; c < kMaxContexts; ++c) ctx_locks[c] = std::unique_lock<std::mutex>(s->ctx[c].mu);
    HIP_TRY(hipSetDevice(s->device));
    StagedCopier back;   // (through page-locked blocks, like every other copy of the library: staging.hpp)
    HIP_TRY(back.copy_back(table.data(), s->dev.lights, sizeof(DevLight) * n, nullptr));
    back.finish();
  }
  for (uint32_t i = 0; i < n; ++i) {
    const DevLight& d = table[i];
    RaycaLightRecord& r = out[i];
    std::memset(&r, 0, sizeof r);
    r.kind = d.kind;
    r.material = d.material;
    r.intensity = d.intensity;
    r.area = d.area;
    std::memcpy(r.color, d.color, 16);
    std::memcpy(r.attenuation, d.attenuation, 16);
    std::memcpy(r.position, d.position, 16);
    std::memcpy(r.ab, d.ab, 16);
    std::memcpy(r.ac, d.ac, 16);
    std::memcpy(r.normal, d.normal, 16);
  }
  return RAYCA_OK;
}

}  // extern "C"
