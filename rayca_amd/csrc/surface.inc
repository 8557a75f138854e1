// surface.inc -- the two kernels behind rayca_hip_surface_device and rayca_hip_camera_rays_device (included from
// kernels.hip, inside its namespace).  Neither traverses anything: k_camera_rays writes the rays camera_ray() gives a frame's
// pixels, k_surface evaluates shade_hit() on hit records a query has written.  With rayca_hip_query_device in between they
// give a host the surface under every pixel (or at the ends of its own rays) without a second copy of the shading arithmetic.

// What the caller's arrays look like to k_surface; every pointer is DEVICE memory, any output may be nullptr.
struct SurfaceIo {
  const float* rays;      // count x 6, or nullptr when neither point nor normal is wanted
  const float* t;         // count
  const uint32_t* prim;   // count
  const float* uv;        // count x 2
  uint32_t count;
  uint32_t full;          // 0: only color / material / flags are wanted (shade_hit's `full = false`, what Flat runs)
  float* point_out;       // x 3
  float* normal_out;      // x 3
  float* color_out;       // x 4
  float* diffuse_out;     // x 4
  float* specular_out;    // x 4
  float* rough_out;       // x 2
  uint32_t* material_out;
  uint32_t* flags_out;
};

// A block's kBlock records of N floats each are N * kBlock consecutive floats of the output.  A lane storing its own record
// would make every store instruction of the wave touch 64 addresses N * 4 bytes apart (for the 12-B records a quarter of the
// bytes of each 64-B segment per instruction, three times over); instead the records cross the LDS once (lane i writes floats
// [N i, N i + N): stride N dwords -- conflict-free for the 12-B records; 2-way for N = 2 and 6, 4-way for the unaligned colour
// fallback, a few LDS cycles beside the global stores they feed) and go out as N dword stores whose lanes are 4 bytes apart --
// whole segments, whatever the alignment of the caller's pointer.  `first` = the block's first record; nothing at or beyond
// record `count` is written.  Every lane of the block must call this (barriers).
constexpr int kStageFloats = 6;  // the widest record: a ray
template <int N>
__device__ __forceinline__ void store_records(float* __restrict__ out, uint64_t first, uint32_t count, const float (&v)[N], float* stage) {
  static_assert(N <= kStageFloats, "stage too small");
  __syncthreads();  // the previous output's reads of `stage`
  for (int k = 0; k < N; ++k) stage[rc_tid() * N + k] = v[k];
  __syncthreads();
  const uint64_t left = (uint64_t)count - first;  // records of this block and behind it (the caller has first < count)
  const uint32_t valid = (uint32_t)(left < (uint64_t)kBlock ? left : (uint64_t)kBlock) * N;
  float* base = out + first * N;
  for (int k = 0; k < N; ++k) {
    const uint32_t j = k * kBlock + rc_tid();
    if (j < valid) base[j] = stage[j];
  }
}
// 16-B records: one dwordx4 store per lane where the pointer allows it (1 KiB per wave instruction), else as above
__device__ __forceinline__ void store_color(float* __restrict__ out, uint64_t first, uint32_t i, bool in_range, uint32_t count, Color c, float* stage) {
  if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0u) {  // (uniform)
    if (in_range) reinterpret_cast<float4*>(out)[i] = as_f4(c);
  } else {
    const float v[4] = {c.r, c.g, c.b, c.a};
    store_records<4>(out, first, count, v, stage);
  }
}

// One hit record per lane -> its surface record.  A record whose prim is RAYCA_NONE or not a slot of this scene is a miss:
// zeros, material RAYCA_NONE, flags 0; nothing of the scene is read for it.  The values of a hit are shade_hit()'s -- color
// always, the rest with io.full -- i.e. what a render kernel has in hand at the same hit (primitive.rs:142-190, hit.rs,
// material/mod.rs:107-185; for a sphere point and normal come from the model-space hit, sphere.rs:138-163).
template <bool SPH>
__global__ __launch_bounds__(kBlock) void k_surface(DevScene sc, SurfaceIo io) {
  __shared__ float stage[kBlock * kStageFloats];
  const uint64_t first = (uint64_t)rc_bid() * kBlock;
  const uint32_t i = (uint32_t)first + rc_tid();   // (first < count <= 2^32 - 1; i may wrap only where i >= count would hold anyway)
  const bool in_range = first + rc_tid() < (uint64_t)io.count;
  DHit hit;
  hit.t = FLT_MAX;
  hit.prim = RAYCA_NONE;
  hit.u = hit.v = 0.0f;
  if (in_range) {
    const uint32_t p = io.prim[i];
    if (p < sc.prim_count) {   // (RAYCA_NONE is not below any count)
      hit.prim = p;
      hit.t = io.t[i];
      hit.u = io.uv[2ull * i];
      hit.v = io.uv[2ull * i + 1ull];
    }
  }
  const bool is_hit = hit.prim != RAYCA_NONE;
  Color color = Color{0.0f, 0.0f, 0.0f, 0.0f};
  ShadeCtx cx;
  cx.point = cx.normal = f4(0.0f, 0.0f, 0.0f, 0.0f);
  cx.kd = cx.ks = color;
  cx.roughness = cx.shininess = 0.0f;
  cx.kind = 0u;
  uint32_t material = RAYCA_NONE, flags = 0u;
  if (is_hit) {
    DRay ray = make_ray(point3(0, 0, 0), vec3(0, 0, 1));   // (not read by what is stored when there are no rays)
    if (io.rays) {
      const float* r = io.rays + 6ull * i;
      ray = make_ray(point3(r[0], r[1], r[2]), vec3(r[3], r[4], r[5]));
    }
    bool emissive = false;
    shade_hit<SPH>(sc, ray, hit, io.full != 0u, color, emissive, cx);
    const PrimExt& e = sc.ext[hit.prim];
    const bool has_material = e.material != RAYCA_NONE && e.material < sc.material_count;   // (as shade_hit picks it)
    material = has_material ? e.material : RAYCA_NONE;
    const uint32_t kind = has_material ? sc.materials[e.material].kind : (uint32_t)RAYCA_MATERIAL_PBR;
    flags = (kind & 3u) | (emissive ? 4u : 0u) | (SPH && e.kind == RAYCA_GEOMETRY_SPHERE ? 8u : 0u) | 0x80000000u;
  }
  if (io.point_out) {
    const float v[3] = {cx.point.x, cx.point.y, cx.point.z};
    store_records<3>(io.point_out, first, io.count, v, stage);
  }
  if (io.normal_out) {
    const float v[3] = {cx.normal.x, cx.normal.y, cx.normal.z};
    store_records<3>(io.normal_out, first, io.count, v, stage);
  }
  if (io.color_out) store_color(io.color_out, first, i, in_range, io.count, color, stage);
  if (io.diffuse_out) store_color(io.diffuse_out, first, i, in_range, io.count, cx.kd, stage);
  if (io.specular_out) store_color(io.specular_out, first, i, in_range, io.count, cx.ks, stage);
  if (io.rough_out) {
    const float v[2] = {cx.roughness, cx.shininess};
    store_records<2>(io.rough_out, first, io.count, v, stage);
  }
  if (in_range) {
    if (io.material_out) io.material_out[i] = material;
    if (io.flags_out) io.flags_out[i] = flags;
  }
}

// The ray of fp.sample of every pixel of the rows this call covers (fp.rows packed rows, the tile mapping of the render
// kernels), 6 floats each: origin, direction -- what camera_ray() hands the traversal of a frame with the same FrameParams.
__global__ __launch_bounds__(kBlock) void k_camera_rays(FrameParams fp, float* __restrict__ rays_out) {
  __shared__ float stage[kBlock * kStageFloats];
  const uint32_t count = fp.rows * fp.width;   // (the host refuses frames of 2^32 pixels or more)
  const uint64_t first = (uint64_t)rc_bid() * kBlock;
  const uint32_t i = (uint32_t)first + rc_tid();
  float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (first + rc_tid() < (uint64_t)count) {
    const uint32_t r = i / fp.width, x = i - r * fp.width;
    const uint32_t y = ((r / fp.band) * fp.parts + fp.part) * fp.band + (r % fp.band);
    const DRay ray = camera_ray(fp, x, y);
    v[0] = ray.o.x; v[1] = ray.o.y; v[2] = ray.o.z;
    v[3] = ray.d.x; v[4] = ray.d.y; v[5] = ray.d.z;
  }
  store_records<6>(rays_out, first, count, v, stage);
}
