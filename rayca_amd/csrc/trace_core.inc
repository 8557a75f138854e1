// trace_core.inc -- device functions shared by every kernel translation unit (kernels.hip, refill.hip): ray / box /
// triangle / sphere arithmetic in the reference's operation order, the per-lane node stack, one traversal step and the
// whole-ray traversal, HitInfo shading, the BRDFs, NEE preparation, camera rays, work tickets.  Included INSIDE
// `namespace rayca { namespace {` after <hip/hip_runtime.h> and "device_types.hpp"; everything has internal linkage.
constexpr int kBlock = 256;
// k_generation's workgroup: one wave.  A persistent wave that finds the work counters dry ends on its own, and its registers
// AND its LDS (stack rows + parked context) go to the next frame's waves at once; as one of four waves of a 256-thread block its
// LDS stayed taken until the slowest of the four had ended.  -DRAYCA_GEN_WAVES_PER_BLOCK=4: the 256-thread block, for A/B runs.
#ifndef RAYCA_GEN_WAVES_PER_BLOCK
#define RAYCA_GEN_WAVES_PER_BLOCK 1
#endif
constexpr int kGenWaves = RAYCA_GEN_WAVES_PER_BLOCK;
constexpr int kGenBlock = 64 * kGenWaves;
static_assert(kGenWaves == 1 || kGenWaves == 2 || kGenWaves == 4, "k_generation's workgroup: 1, 2 or 4 waves");
#ifndef RAYCA_TRACE_MIN_WAVES
#define RAYCA_TRACE_MIN_WAVES 1
#endif
#ifndef RAYCA_MIN_WAVES_FLAT
#define RAYCA_MIN_WAVES_FLAT 5
#endif
// the path k_generation's waves per SIMD (its __launch_bounds__): 5 = 96 VGPRs, for which the compiler keeps six registers of the
// bench instantiation in scratch (28 B; its non-SPILL sibling four, 20 B).  None is touched inside a node or leaf loop, but they
// are inside the batch loop: the ray's RNG key is reloaded once behind every trace() call, the lane number and push_ray's
// lanes-below mask once per batch in the tail (profiles/r08_five_waves_resources.txt).  The fifth wave hides more of a node
// fetch's latency.  -DRAYCA_MIN_WAVES=4: 112 registers, the kernel as it was.  path_waves: the bound an instantiation gets --
// the counting and the sphere ones keep four (at five they would need 7 to 45 registers in scratch, and no timed frame runs them);
// the host gives a launch its stack rows by the same function (fused_generation).
#ifndef RAYCA_MIN_WAVES
#define RAYCA_MIN_WAVES 5
#endif
constexpr int path_waves(bool stats, bool sph) { return stats || sph ? 4 : RAYCA_MIN_WAVES; }

// Thread and block indices from the compiler's builtins.  threadIdx.x and its kin go through functions of the device library,
// and a function only inlines into one whose target features contain its own: in the RAYCA_NO_PK_F32 functions (no_pk.hpp)
// every one of them would stay a call.  For the same reason the structs these functions construct are aggregates (no
// implicit constructor to call) and every device function of the project is __forceinline__ or declared inside the region.
__device__ __forceinline__ uint32_t rc_tid() { return __builtin_amdgcn_workitem_id_x(); }
__device__ __forceinline__ uint32_t rc_bid() { return __builtin_amdgcn_workgroup_id_x(); }
__device__ __forceinline__ uint32_t rc_bdim() { return __builtin_amdgcn_workgroup_size_x(); }
__device__ __forceinline__ uint32_t rc_gdim() { return __builtin_amdgcn_grid_size_x() / __builtin_amdgcn_workgroup_size_x(); }

// A kernel argument read where it is used.  A persistent kernel whose arguments add up to more dwords than a wave has SGPRs
// gets them all loaded at entry and kept over its loop: k_generation spilled 72 of them into VGPR lanes and moved them back,
// one v_readlane_b32 each, in the code that runs once per batch, vertex or sample.  cold_arg<T>(offset) is a reference to the
// bytes at `offset` of the kernel-argument segment (offsetof in the kernel's one aggregate argument), in the constant address
// space: what is read through it is a scalar load at the point of use.  The empty asm makes the pointer opaque there, so the
// loads cannot be hoisted to the kernel's entry and merged with the by-value argument.  Only for fields read outside the
// traversal loops; what those read stays an ordinary argument, in SGPRs.
template <class T>
__device__ __forceinline__ const T& cold_arg(uint32_t offset) {
  typedef __attribute__((address_space(4))) const char ConstByte;
  ConstByte* p = (ConstByte*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const T*)(p + offset);
}

struct DRay {
  F4 o, d, rd;  // origin (w=1), direction (w=0), zero-safe reciprocal
};
struct DHit {
  float t;
  uint32_t prim;
  float u, v;
};

__device__ __forceinline__ DRay make_ray(F4 origin, F4 dir) {  // Ray::new  ray.rs:63-72
  DRay r;
  r.rd = reciprocal(dir);
  origin.w = 1.0f;
  r.o = origin;
  r.d = dir;
  return r;
}

// ---- geometry --------------------------------------------------------------------------------
// AABB::intersects  bvh/aabb.rs:74-93.  (a-o)*rdir goes through Point3::scale = fma(x, s, 0).
__device__ __forceinline__ bool slab(float ax, float ay, float az, float bx, float by, float bz, const DRay& r, float& tmin_out) {
  const float t1x = __fmaf_rn(ax - r.o.x, r.rd.x, 0.0f), t2x = __fmaf_rn(bx - r.o.x, r.rd.x, 0.0f);
  const float t1y = __fmaf_rn(ay - r.o.y, r.rd.y, 0.0f), t2y = __fmaf_rn(by - r.o.y, r.rd.y, 0.0f);
  const float t1z = __fmaf_rn(az - r.o.z, r.rd.z, 0.0f), t2z = __fmaf_rn(bz - r.o.z, r.rd.z, 0.0f);
  const float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fminf(fmaxf(t1z, t2z), FLT_MAX));
  const float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fmaxf(fminf(t1z, t2z), -FLT_MAX));
  tmin_out = tmin;
  return tmax >= tmin && tmax > 0.0f;
}

// Conservative box test for trees whose boxes are padded (RAYCA_BUILDER_SAH): t = b*rd - o*rd with one
// FMA per plane.  Not the reference's rounding -- it does not have to be: in that mode a triangle is a
// candidate iff the reference's own leaf box passes `slab` (reference_candidate), this test only steers
// the search.  It must accept every box whose reference box passes `slab`.  Two error terms stand against that:
//   * per plane, 2^-23 |b rd|: the padding of the boxes (2^-16 |b| + 2^-20 diagonal, host_scene.cpp) dominates it;
//   * per ray and axis, 2^-23 |o rd|: c = -(o*rd) is rounded once (2^-24 |c|), the FMA's result lies near c when the
//     origin is far (another 2^-24 |c|), and the reference's own (b - o) * rd carries as much.  The padding is fixed at
//     build time and knows nothing of o: it covers this term while |o| <= 4 scene diagonals on every axis (2^-20 diagonal |rd|
//     >= 2 x 2^-23 |o rd|, whatever the direction: ray_needs_slack) and not beyond.  RAYCA_RAY_SLACK: the tests compare
//     tmax + slack, slack = 2^-21 max |c|, four times the sum; the cull bound of ORDERED searches gets it too (cull_limit).
// Every m, c and slack the tests see is finite, so that no plane distance is a NaN (inf - inf, where the reference has +-inf)
// and a point box -- the unused slots of the 4-wide nodes -- fails as it did without the slack.  fix_axis sees to it:
//   * m or c overflows for a finite origin (a denormal or tiny direction component): on such an axis the ray does not move,
//     and the reference accepts a box only if o lies strictly between its planes.  Restated as m = +-M, c = (centre - o) M with
//     M = min(2^100, 2^120 / |centre - o|): planes on either side of o read -+M x distance (at least M x padding >= 2^104 x
//     2^-16 |o| or 2^100 x padding: beyond every t of the other axes), planes on one side of it read the same sign;
//   * the origin itself is NaN or infinite on the axis: the reference's triangle test then yields a NaN or infinite depth, which
//     never becomes a record (tests/test_ray_edges_cpu.py asserts the miss) -- m = 0, c = -FLT_MAX puts every box
//     far behind the ray, so every box fails and the search ends at the root.
#ifndef RAYCA_RAY_SLACK
#define RAYCA_RAY_SLACK 1
#endif
struct FastRay {
  float mx, my, mz, cx, cy, cz;  // plane distance t = coordinate * m + c
#if RAYCA_RAY_SLACK
  float slack;                   // what the rounding of c can move a plane distance by (in units of t), times four
  bool fixed;                    // an axis went through fix_axis
#endif
};
__device__ __forceinline__ bool fix_axis(float& m, float& c, float o, float centre, float inv_scale) {
  if (fabsf(c) <= FLT_MAX && fabsf(m) <= FLT_MAX) return false;
  const float d = centre - o;
  if (!(fabsf(d) <= FLT_MAX)) {   // NaN or infinite origin
    m = 0.0f;
    c = -FLT_MAX;
    return true;
  }
  const float big = copysignf(fminf(1.2676506002282294e30f, 1.329227995784916e36f / fabsf(d)), m);   // min(2^100, 2^120 / |d|)
  m = big * inv_scale;
  c = d * big;
  return true;
}
// f32 boxes: t = b*rd - o*rd.  fp16 boxes hold (x - centre) * scale: t = h * (rd / scale) + (centre - o) * rd.
__device__ __forceinline__ FastRay make_fast(const DevScene& sc, const DRay& r, bool half) {
  FastRay f;
  if (half) {
    f.mx = r.rd.x * sc.half_inv_scale; f.my = r.rd.y * sc.half_inv_scale; f.mz = r.rd.z * sc.half_inv_scale;
    f.cx = (sc.half_center[0] - r.o.x) * r.rd.x; f.cy = (sc.half_center[1] - r.o.y) * r.rd.y; f.cz = (sc.half_center[2] - r.o.z) * r.rd.z;
  } else {
    f.mx = r.rd.x; f.my = r.rd.y; f.mz = r.rd.z;
    f.cx = -(r.o.x * r.rd.x); f.cy = -(r.o.y * r.rd.y); f.cz = -(r.o.z * r.rd.z);
  }
#if RAYCA_RAY_SLACK
  f.fixed = fix_axis(f.mx, f.cx, r.o.x, half ? sc.half_center[0] : 0.0f, half ? sc.half_inv_scale : 1.0f);
  f.fixed |= fix_axis(f.my, f.cy, r.o.y, half ? sc.half_center[1] : 0.0f, half ? sc.half_inv_scale : 1.0f);
  f.fixed |= fix_axis(f.mz, f.cz, r.o.z, half ? sc.half_center[2] : 0.0f, half ? sc.half_inv_scale : 1.0f);
  f.slack = fmaxf(fmaxf(fabsf(f.cx), fabsf(f.cy)), fabsf(f.cz)) * 4.76837158203125e-07f;   // 2^-21 max |c|
#endif
  return f;
}
// Where the slack is needed.  Per axis the padding of a box is worth at least 2^-20 diagonal |rd| in t, the rounding of c
// 2^-23 |o rd|: with |o| <= 4 diagonals on every axis (and a finite c) the padding covers it twice over, whatever the
// direction.  Shadow and bounce rays start on the scene's surfaces and camera rays usually near them, so trace() takes the
// form with the slack only if a ray of the wave needs it (one wave-uniform branch per ray, nothing in the node loop of the other
// form: the slack as a seventh value per ray -- kept in a register, recomputed from c in every step, or as the wave's maximum in
// an SGPR -- cost the path kernels, which sit at their register limits, 13 to 22 %; profiles/r04_ab_slack.log).  The kernels
// that take the caller's or the camera's rays alone (k_query_refill, k_flat_refill, Flat frames) always carry it: trace()'s SLACK_FORM.
__device__ __forceinline__ bool ray_needs_slack(const DevScene& sc, const DRay& r, const FastRay& f) {
#if RAYCA_RAY_SLACK
  const float radius = sc.cull_abs * 4096.0f;   // cull_abs = 2^-10 diagonal
  return !(fabsf(r.o.x) <= radius && fabsf(r.o.y) <= radius && fabsf(r.o.z) <= radius) || f.fixed;
#else
  return false;
#endif
}
// what a box test reports for tmin / tmax.  (Slack, m and c are finite: a NaN here comes from the NaN planes of an unused
// fp16 slot, and fails.)
template <bool SLACK>
__device__ __forceinline__ bool slab_verdict(float tmin, float tmax, const FastRay& f) {
#if RAYCA_RAY_SLACK
  if (SLACK) {
    const float tp = tmax + f.slack;
    return tp >= tmin && tp > 0.0f;
  }
#endif
  return tmax >= tmin && tmax > 0.0f;
}
// the cull bound of an ORDERED search whose best (or allowed) depth is b: see trace()
template <bool SLACK>
__device__ __forceinline__ float cull_limit(const DevScene& sc, const FastRay& f, float b) {
#if RAYCA_RAY_SLACK
  if (SLACK) return b + fabsf(b) * 9.765625e-4f + sc.cull_abs + f.slack;
#endif
  return b + fabsf(b) * 9.765625e-4f + sc.cull_abs;
}
// fp16 -> f32 is exact and free: fmaf((float)half, a, b) is one v_fma_mix_f32
typedef _Float16 rc_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float lo16(uint32_t w) { return (float)__builtin_bit_cast(rc_h2, w).x; }
__device__ __forceinline__ float hi16(uint32_t w) { return (float)__builtin_bit_cast(rc_h2, w).y; }
template <bool SLACK>
__device__ __forceinline__ bool slab_fast(float ax, float ay, float az, float bx, float by, float bz, const FastRay& f, float& tmin_out) {
  const float t1x = __fmaf_rn(ax, f.mx, f.cx), t2x = __fmaf_rn(bx, f.mx, f.cx);
  const float t1y = __fmaf_rn(ay, f.my, f.cy), t2y = __fmaf_rn(by, f.my, f.cy);
  const float t1z = __fmaf_rn(az, f.mz, f.cz), t2z = __fmaf_rn(bz, f.mz, f.cz);
  const float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
  const float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
  tmin_out = tmin;
  return slab_verdict<SLACK>(tmin, tmax, f);
}
// RAYCA_NODE_CH (round 3): the steering boxes of the binary f32 nodes as centre c and half extent h (DevScene::nodes_ch, made on
// the device from the min / max nodes: k_make_ch_nodes).  t of the centre plane = c*m + k; the near and far planes lie h*|m| before
// and behind it: three v_fma_f32 per axis (|m| is a free source modifier) and no v_min / v_max per axis -- on this chip v_fma issues
// in ~2.4 cycles, v_min / v_max in 4.1 (profiles/peaks_r03.json): 9 fast + 4 slow instructions per box instead of 6 fast + 10 slow.
// Conservative like slab_fast (every centre / half box contains its min / max box; the padding of the steering boxes and the
// ray's slack cover the rounding of the evaluation), so the same pixels; measured with binary f32 nodes pinned, four frames in flight: depth-1 frame
// 0.3669 -> 0.3607 ms, Flat 0.1888 -> 0.1871 (profiles/r03_ab_ch.log).  -DRAYCA_NODE_CH=0 goes back to min / max planes.
#ifndef RAYCA_NODE_CH
#define RAYCA_NODE_CH 1
#endif
// RAYCA_NODE_CH48: the centre / half-extent node in 48 B = three 16-B loads instead of four.  The node loop is bound by vector-L1
// accesses (one per 128-B line and load instruction, DESIGN 4.1), so a fetch of three loads is a quarter fewer of them.  The two
// child references live in the low 16 bits of the x and y half extents of their child's box: a half extent keeps 8 mantissa bits
// (rounded up before the reference is put below them, so the box only grows, by < 2^-6 = 1.6 % of ITS OWN size -- the centre / half form is
// what makes that cheap: the error scales with the box, not with the coordinates), is used by the slab test as it is, and the
// reference comes back with one v_perm_b32.  (The left box of a link of a big leaf's chain grows by one step more, so that it stays
// the one entered first: k_make_ch_nodes.)
// Measured, four frames in flight, same bits (profiles/r03_ab_ch.log): atrium depth-1 frame 0.3604 -> 0.3345 ms (-7.2 %), Flat
// 0.1741 -> 0.1627 (-6.5 %).  The wavefront kernels' incoherent rays stay on 4-wide fp16 nodes (one 16-B load per child box; this
// record is 1.5): with this record under them the 5-deep 1080p frame goes 3.93 -> 4.19 (bounce) -> 4.41 ms (+ shadow).
#ifndef RAYCA_NODE_CH48
#define RAYCA_NODE_CH48 1
#endif
constexpr uint32_t kChNodeQuads = RAYCA_NODE_CH48 ? 3u : 4u;   // float4 per node of DevScene::nodes_ch
constexpr uint32_t kChRefScale = RAYCA_NODE_CH48 ? 48u : 1u;   // an inner reference of that array = node index x this (DevScene::root_ref_ch too)
// Node formats of the wavefront kernels, fixed from measurements with two frames in flight on the atrium
// (tests/gpu_ab_inflight.py, 5-deep path trace): all binary f32 7.89 ms; bounce rays on 4-wide fp16 nodes 7.28;
// + shadow rays on fp16 7.19, on 4-wide fp16 6.88 (camera rays: binary fp16).  Same bits with every format.
#ifndef RAYCA_WF_PRIMARY_WIDE
#define RAYCA_WF_PRIMARY_WIDE 0
#endif
#ifndef RAYCA_WF_PRIMARY_HALF
#define RAYCA_WF_PRIMARY_HALF 1
#endif
#ifndef RAYCA_WF_BOUNCE_WIDE
#define RAYCA_WF_BOUNCE_WIDE 1
#endif
#ifndef RAYCA_WF_BOUNCE_HALF
#define RAYCA_WF_BOUNCE_HALF 1
#endif
#ifndef RAYCA_WF_SHADOW_WIDE
#define RAYCA_WF_SHADOW_WIDE 1
#endif
#ifndef RAYCA_WF_SHADOW_HALF
#define RAYCA_WF_SHADOW_HALF 1
#endif
template <bool SLACK>
__device__ __forceinline__ bool slab_ch(float cx, float cy, float cz, float hx, float hy, float hz, const FastRay& f, float& tmin_out) {
  const float tx = __fmaf_rn(cx, f.mx, f.cx), ty = __fmaf_rn(cy, f.my, f.cy), tz = __fmaf_rn(cz, f.mz, f.cz);
  const float ex = fabsf(f.mx), ey = fabsf(f.my), ez = fabsf(f.mz);
  const float nx = __fmaf_rn(-hx, ex, tx), ny = __fmaf_rn(-hy, ey, ty), nz = __fmaf_rn(-hz, ez, tz);
  const float fx = __fmaf_rn(hx, ex, tx), fy = __fmaf_rn(hy, ey, ty), fz = __fmaf_rn(hz, ez, tz);
  const float tmax = fminf(fminf(fx, fy), fz);
  const float tmin = fmaxf(fmaxf(nx, ny), nz);
  tmin_out = tmin;
  return slab_verdict<SLACK>(tmin, tmax, f);
}
// the same arithmetic on decoded fp16 planes (make_fast folds centre and scale into m and c)
template <bool SLACK>
__device__ __forceinline__ bool slab_half(float ax, float ay, float az, float bx, float by, float bz, const FastRay& f, float& tmin_out) {
  return slab_fast<SLACK>(ax, ay, az, bx, by, bz, f, tmin_out);
}

// Triangle::intersects  rayca-geometry/src/triangle.rs:84-159 on world-space vertices (identical
// bits to `trs * vertex`, computed once on the host with the same operation sequence).
__device__ __forceinline__ bool tri_test(F4 v0, F4 v1, F4 v2, const DRay& r, float& t_out, float& u_out, float& v_out) {
  const F4 v0v1 = v1 - v0;
  const F4 v0v2 = v2 - v0;
  const F4 n = cross(v0v1, v0v2);
  if (dot(r.d, n) > 0.0f) return false;  // back-face cull
  const float denom = dot(n, n);
  const float ndd = dot(n, r.d);
  if (fabsf(ndd) < FLT_EPSILON) return false;
  const float d = -dot(n, v0);
  const float t = -(dot(n, to_vec(r.o)) + d) / ndd;
  if (t < 0.0f) return false;
  const F4 p = r.o + r.d * t;
  F4 c = cross(v1 - v0, to_vec(p - v0));
  if (dot(n, c) < 0.0f) return false;
  c = cross(v2 - v1, to_vec(p - v1));
  const float u = dot(n, c);
  if (u < 0.0f) return false;
  c = cross(v0 - v2, to_vec(p - v2));
  const float v = dot(n, c);
  if (v < 0.0f) return false;
  t_out = t;
  u_out = u / denom;
  v_out = v / denom;
  return true;
}

// Sphere::intersects  rayca-geometry/src/sphere.rs:101-163: the ray is taken to model space by
// Inversed<&Trs> (translate -T, rotate R^-1, scale 1/S; trs.rs:405-414), intersected, and the hit point is
// brought back by the world Trs.  A sphere occupies one primitive slot whose first float is NaN and
// whose second float carries the sphere index.
__device__ __forceinline__ DRay sphere_local_ray(const DevSphere& sp, const DRay& r) {
  F4 o = r.o + (-f4(sp.translation[0], sp.translation[1], sp.translation[2], 0.0f));  // Ray::translate
  F4 d = r.d;
  const F4 iq = f4(sp.inv_rotation[0], sp.inv_rotation[1], sp.inv_rotation[2], sp.inv_rotation[3]);
  d = rotate(d, iq);  // Ray::rotate
  o = point_rotate(o, iq);
  o.w = 1.0f;
  const F4 is = f4(sp.inv_scale[0], sp.inv_scale[1], sp.inv_scale[2], sp.inv_scale[3]);
  d = d * is;  // Ray::scale
  o = point_scale(o, is);
  DRay l;
  l.o = o;
  l.d = d;
  l.rd = reciprocal(d);
  return l;
}
__device__ __forceinline__ bool sphere_test(const DevSphere& sp, const DRay& r, float& t_out) {
  const DRay l = sphere_local_ray(sp, r);
  const F4 center = f4(sp.center[0], sp.center[1], sp.center[2], sp.center[3]);
  const float a = dot(l.d, l.d);
  const F4 c_to_r = as_vec(l.o - center);
  const float b = dot(c_to_r, l.d);
  const float c = dot(c_to_r, c_to_r) - sp.radius2;
  const float det = b * b - a * c;
  if (det < 0.0f) return false;
  const float det_sqrt = sqrtf(det);
  const float t0 = (-b + det_sqrt) / a;
  const float t1 = (-b - det_sqrt) / a;
  if (t0 < 0.0f && t1 < 0.0f) return false;
  float t;
  if (t0 >= 0.0f && t1 >= 0.0f) t = fminf(t0, t1);
  else if (t0 >= 0.0f) t = t0;
  else t = t1;
  t_out = t;
  return true;
}

// Primitive slot i: one aligned 48-B record, three 16-B loads (the packed 36-B triangle took four instructions):
//   q0 = (v0.x, v0.y, v0.z, v1.x)   q1 = (v1.y, v1.z, v2.x, v2.y)   q2 = (v2.z, tie rank, reference leaf, -)
// world-space vertices, then what decides whether a hit on this triangle COUNTS (RAYCA_BUILDER_SAH): its rank in the reference's
// primitive order and the reference leaf it lives in.  Round 2 kept rank and leaf id in arrays of their own: a triangle that
// had just become the best hit then waited for two DEPENDENT fetches (leaf id, then the leaf's box: ~500 cycles each on the
// loaded chip) before the filter's slab test could run; now the record that brings the triangle brings the id, and one fetch is
// left.  (A 64-B record with the leaf's box itself was measured too: no fetch left, but 28 B more per triangle test cost as much
// as the fetch had -- profiles/r03_ab_filter.log.)
struct TriRecord {
  F4 v0, v1, v2;
  uint32_t rank, leaf;
};
constexpr uint32_t kTriQuads = 3, kTriFloats = 12;
__device__ __forceinline__ TriRecord load_tri(const DevScene& sc, uint32_t i) {
  const float4* p = sc.tris + (size_t)kTriQuads * i;
  const float4 q0 = p[0], q1 = p[1], q2 = p[2];
  TriRecord t;
  t.v0 = vec3(q0.x, q0.y, q0.z);
  t.v1 = vec3(q0.w, q1.x, q1.y);
  t.v2 = vec3(q1.z, q1.w, q2.x);
  t.rank = __float_as_uint(q2.y);
  t.leaf = __float_as_uint(q2.z);
  return t;
}

// exact depth tie: the primitive that comes first in the reference's order wins (strict `<` in a
// left-to-right DFS, blas.rs:151,161,169).  `rank_a`: the candidate's, from its record; the holder's is fetched (ties are rare).
__device__ __forceinline__ bool tie_before(const DevScene& sc, uint32_t rank_a, uint32_t b) {
  if (b == RAYCA_NONE) return true;
  const uint32_t rank_b = __float_as_uint(reinterpret_cast<const float*>(sc.tris)[(size_t)kTriFloats * b + 9u]);
  return rank_a < rank_b;
}

// RAYCA_BUILDER_SAH: the reference only ever tests triangle i if the slab test passes for every box
// above it in ITS tree; those boxes are nested and the slab arithmetic is monotone in the corners, so
// that is equivalent to the slab test of the reference LEAF that holds i (bvh/blas.rs:136-139).
__device__ __forceinline__ bool reference_candidate(const DevScene& sc, const TriRecord& t, const DRay& r) {
  if (!sc.ref_leaf_of) return true;
  const float4* b = sc.ref_leaf_boxes + 2ull * t.leaf;
  const float4 lo = b[0], hi = b[1];
  float tmin;
  return slab(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, r, tmin);
}

struct LaneCounters {   // (an aggregate: `LaneCounters cnt{};`)
  uint32_t boxes, tris;
  // STATS only: what the lock-step wave pays -- every trip of the node loop / the leaf loop costs all 64 lanes,
  // booked by the first lane that takes the trip
  unsigned long long slot_boxes, slot_tris;
  __device__ __forceinline__ bool books() const { return __lane_id() == (uint32_t)__ffsll((long long)__ballot(1)) - 1u; }
};

constexpr uint32_t kTerminated = 0x7FFFFFFFu;  // "no node left": an inner index that never exists (== kNoChild)

// Per-lane node stack: the first `lds_entries` entries in LDS (entry-major: entry e of thread t at
// lds[e*STRIDE + t], so the 64 lanes of a wave always hit 64 different banks whatever their depths),
// deeper entries in a global spill area laid out the same way.  STRIDE is the thread count of the kernel's workgroup: kBlock
// everywhere but in k_generation, whose workgroups are kGenBlock threads.  The spill branch is cold: the LDS part
// is sized from the tree on the host and covers every traversal of ordinary trees.
template <bool SPILL, int STRIDE = kBlock>
struct NodeStack {
  uint32_t* lds;
  uint32_t* ovf;       // wave-uniform base of the spill area (a per-lane pointer would be two more registers in every loop)
  uint32_t gthread;    // this lane's column in it
  uint32_t lds_entries, ovf_stride, sp;
  // the newest entry lives in a register: a pop hands it out at once (-3 % on 5-deep paths, neutral on camera rays).  Its
  // successor comes from LDS: pop() waits for it on the spot (the compiled form reads into a temporary, waits and moves), the
  // pipelined node loop of trace_search reads it INTO this register (book / pop_late below), and the wait stands at the next use
  // of `top`, behind the loads of the node that follows.
  uint32_t top;
  __device__ __forceinline__ void clear() { sp = 0; top = kTerminated; }
  // RAYCA_STACK_AS: the two homes of an entry are addressed in their own address spaces.  Through generic pointers the
  // compiler folds `i < lds_entries ? lds[..] : ovf[..]` into ONE flat_load / flat_store of a selected address: every pop of
  // a path frame then goes the flat way (address check in the texture addresser, both wait counters) to reach LDS.
#ifndef RAYCA_STACK_AS
#define RAYCA_STACK_AS 1
#endif
  typedef __attribute__((address_space(3))) uint32_t LdsWord;
  typedef __attribute__((address_space(1))) uint32_t GlobalWord;
  __device__ __forceinline__ void put(uint32_t i, uint32_t v) {
#if RAYCA_STACK_AS
    if (!SPILL || i < lds_entries) ((LdsWord*)lds)[i * STRIDE] = v;
    else ((GlobalWord*)ovf)[(size_t)(i - lds_entries) * ovf_stride + gthread] = v;
#else
    if (!SPILL || i < lds_entries) lds[i * STRIDE] = v;
    else ovf[(size_t)(i - lds_entries) * ovf_stride + gthread] = v;
#endif
  }
  __device__ __forceinline__ uint32_t get(uint32_t i) const {
#if RAYCA_STACK_AS
    uint32_t v;
    if (!SPILL || i < lds_entries) v = ((const LdsWord*)lds)[i * STRIDE];
    else v = ((const GlobalWord*)ovf)[(size_t)(i - lds_entries) * ovf_stride + gthread];
    return v;
#else
    return (!SPILL || i < lds_entries) ? lds[i * STRIDE] : ovf[(size_t)(i - lds_entries) * ovf_stride + gthread];
#endif
  }
  __device__ __forceinline__ void push(uint32_t v) {
    if (top != kTerminated) put(sp++, top);
    top = v;
  }
  __device__ __forceinline__ uint32_t pop() {
    const uint32_t r = top;
    if (sp == 0) top = kTerminated;
    else top = get(--sp);
    return r;
  }
  // ---- the stack operations of the pipelined node loop (trace_search) ----
  // One operation of the lanes that take part, as straight-line code: `wr` lanes store `top` as entry `at`, `rd` lanes fetch
  // entry `at` into `top`; in the other lanes `top` stays (`keep`) or becomes `v` (no lane does both; the callers move sp).
  // Each is one LDS instruction under one exec mask, and nothing waits for the read here.  The spill area (entries >=
  // lds_entries) is one block out of line, entered when some lane of the wave stands at or above the boundary at all
  // (`at` <= sp): it serves the lanes whose entry lies beyond it and takes them out of the two masks.
  // (Always through the address-space pointers: RAYCA_STACK_AS=0 only concerns put / get, i.e. every loop but the pipelined one.
  // That `top` is made in place rests on the empty asm below; it costs speed, never a result, if a compiler decides otherwise --
  // profiles/r06_node_loop_after.txt records the compiled form.)
  __device__ __forceinline__ void transfer(bool wr, bool rd, uint32_t at, bool keep, uint32_t v, uint32_t& out) {
    if (SPILL && __ballot(sp >= lds_entries) != 0ull) {
      const bool deep = at >= lds_entries;
      GlobalWord* const g = (GlobalWord*)ovf + ((size_t)(at - lds_entries) * ovf_stride + gthread);
      if (wr && deep) *g = top;
      if (rd && deep) {
        v = *g;
        asm volatile("" : "+v"(v));   // (no instruction: the wait for this load stands here, in the cold block, not where the paths join)
        keep = false;
      }
      wr = wr && !deep;
      rd = rd && !deep;
    }
    if (wr) ((LdsWord*)lds)[at * STRIDE] = top;
    // (no instruction: `out`, what the caller hands on of the old `top`, is made in front of this point and the new `top` behind
    // it, in the old one's register.  Left to itself the compiler makes the new value beside the old one, which it reads last:
    // the read below then lands in a second register, and a wait for it and a move back stand in front of the next node's loads)
    asm volatile("" : "+v"(top), "+v"(out));
    top = keep ? top : v;
    if (rd) top = ((const LdsWord*)lds)[at * STRIDE];
  }
  // the binary step's bookkeeping, `cur` = none ? top : nearer child already made (and the next node's loads issued with it):
  // both children hit -> `far` becomes the newest entry and the one before it is stored; none -> the successor of the entry
  // handed out is fetched; one hit -> nothing moves
  __device__ __forceinline__ void book(bool both, bool none, uint32_t far, uint32_t& cur) {
    const bool wr = both && top != kTerminated, rd = none && sp != 0u;
    const uint32_t at = rd ? sp - 1u : sp;
    transfer(wr, rd, at, !(both || none), both ? far : kTerminated, cur);
    sp = wr ? sp + 1u : at;
  }
  // pop() for the lanes with `take`; the others keep their stack and get kTerminated (an any-hit ray that has found its occluder)
  __device__ __forceinline__ uint32_t pop_late(bool take) {
    uint32_t r = take ? top : kTerminated;
    const bool rd = take && sp != 0u;
    sp -= rd ? 1u : 0u;
    transfer(false, rd, sp, !take, kTerminated, r);
    return r;
  }
};
template <bool SPILL, int STRIDE = kBlock>
__device__ __forceinline__ NodeStack<SPILL, STRIDE> make_stack(uint32_t* lds_base, const TraceLaunch& tl, uint32_t global_thread) {
  NodeStack<SPILL, STRIDE> st;
  st.lds = lds_base + rc_tid();
  st.ovf = tl.ovf;
  st.gthread = global_thread;
  st.lds_entries = tl.lds_entries;
  st.ovf_stride = tl.ovf_stride;
  st.clear();
  return st;
}

// leaf: test primitives [first, first+count) -- shared by both node formats
template <bool ORDERED, bool SPH, bool STATS, bool SLACK = true>
__device__ __forceinline__ void test_leaf(const DevScene& sc, const DRay& r, const FastRay& fr, uint32_t ref, float t_stop, DHit& hit, float& limit,
                                          LaneCounters& cnt) {
  const uint32_t first = ref & kLeafFirstMask;
  const uint32_t count = ((ref >> 25) & 63u) + 1u;
  for (uint32_t i = first; i < first + count; ++i) {
    const TriRecord tr = load_tri(sc, i);
    if (STATS) {
      cnt.tris++;
      if (cnt.books()) cnt.slot_tris += 64ull;
    }
    float t, u, v;
    bool got;
    if (SPH && tr.v0.x != tr.v0.x) {  // sphere slot
      u = v = 0.0f;
      got = sphere_test(sc.spheres[__float_as_uint(tr.v0.y)], r, t);
    } else {
      got = tri_test(tr.v0, tr.v1, tr.v2, r, t, u, v);
    }
    if (got) {
      if ((t < hit.t || (t == hit.t && tie_before(sc, tr.rank, hit.prim))) && reference_candidate(sc, tr, r)) {
        hit.t = t;
        hit.prim = i;
        hit.u = u;
        hit.v = v;
        if (ORDERED) {
          limit = cull_limit<SLACK>(sc, fr, fminf(t, t_stop));
        }
      }
    }
  }
}

// One trip through the node loop: test the children of inner node `cur`, push what stays pending, return the
// next node (inner, leaf or kTerminated).
template <bool ORDERED, bool FAST, bool WIDE, bool SPILL, bool STATS, bool HALF, bool SLACK = true, int STRIDE = kBlock>
__device__ __forceinline__ uint32_t node_step(const DevScene& sc, const DRay& r, const FastRay& fr, float limit, uint32_t cur, NodeStack<SPILL, STRIDE>& st,
                                              LaneCounters& cnt) {
  if (STATS && cnt.books()) cnt.slot_boxes += WIDE ? 256ull : 128ull;
  if (WIDE) {
    float key[4];
    uint32_t ref[4];
    if (FAST && HALF) {
      const uint4* np = sc.nodes4_h + 4ull * cur;
      const uint4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
      if (STATS) cnt.boxes += 4;
      ref[0] = q3.x; ref[1] = q3.y; ref[2] = q3.z; ref[3] = q3.w;
      const float ax[4] = {lo16(q0.x), hi16(q0.x), lo16(q0.y), hi16(q0.y)}, ay[4] = {lo16(q0.z), hi16(q0.z), lo16(q0.w), hi16(q0.w)};
      const float az[4] = {lo16(q1.x), hi16(q1.x), lo16(q1.y), hi16(q1.y)}, bx[4] = {lo16(q1.z), hi16(q1.z), lo16(q1.w), hi16(q1.w)};
      const float by[4] = {lo16(q2.x), hi16(q2.x), lo16(q2.y), hi16(q2.y)}, bz[4] = {lo16(q2.z), hi16(q2.z), lo16(q2.w), hi16(q2.w)};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float tc;
        bool h = slab_half<SLACK>(ax[c], ay[c], az[c], bx[c], by[c], bz[c], fr, tc);
        if (ORDERED) h = h && tc <= limit;
        key[c] = h ? (ORDERED ? tc : (float)c) : INFINITY;
      }
    } else {
    const float4* np = sc.nodes4 + 8ull * cur;
    const float4 lx = np[0], ly = np[1], lz = np[2], hx = np[3], hy = np[4], hz = np[5], cr = np[6];
    if (STATS) cnt.boxes += 4;
    ref[0] = __float_as_uint(cr.x); ref[1] = __float_as_uint(cr.y); ref[2] = __float_as_uint(cr.z); ref[3] = __float_as_uint(cr.w);
    const float ax[4] = {lx.x, lx.y, lx.z, lx.w}, ay[4] = {ly.x, ly.y, ly.z, ly.w}, az[4] = {lz.x, lz.y, lz.z, lz.w};
    const float bx[4] = {hx.x, hx.y, hx.z, hx.w}, by[4] = {hy.x, hy.y, hy.z, hy.w}, bz[4] = {hz.x, hz.y, hz.z, hz.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float tc;
      bool h = FAST ? slab_fast<SLACK>(ax[c], ay[c], az[c], bx[c], by[c], bz[c], fr, tc) : slab(ax[c], ay[c], az[c], bx[c], by[c], bz[c], r, tc);
      if (ORDERED) h = h && tc <= limit;
      // sort key: entry distance (ORDERED) or the child's index (reference order); misses sort last
      key[c] = h ? (ORDERED ? tc : (float)c) : INFINITY;
    }
    }
    // 5-comparator network, strict `>` so equal keys keep their index order (the chains that
    // split big leaves rely on it: see WideBuilder).  Three leaner or earlier forms of this step were measured (atrium
    // 1080p, two frames in flight; depth-1 / Flat / 5-deep frame in ms, as it is: 0.4215 / 0.2050 / 5.150) and not kept:
    // only the nearest child found, the other hits pending in slot order 0.4258 / 0.2044 / 5.355; pushes without branches
    // (unconditional writes to the free slots, conditional increments) 0.4234 / 0.2039 / 5.243, the soup's refill kernel
    // 7.24 vs 6.25; the next node's words fetched as soon as the nearest child is known (after three comparators), the rest
    // of the sort and the pushes under the load 0.4391 / 0.2035 / 5.277, soup 6.69 vs 6.81
    // (profiles/r02_ab_nosort.log, r02_ab_wpush.log, r02_ab_pipe.log).
#define RC_CE(i, j)                                  \
  {                                                  \
const bool sw = key[i] > key[j];                 \
const float ka = sw ? key[j] : key[i];           \
const float kb = sw ? key[i] : key[j];           \
const uint32_t ra = sw ? ref[j] : ref[i];        \
const uint32_t rb = sw ? ref[i] : ref[j];        \
key[i] = ka; key[j] = kb; ref[i] = ra; ref[j] = rb; \
  }
    RC_CE(0, 1) RC_CE(2, 3) RC_CE(0, 2) RC_CE(1, 3) RC_CE(1, 2)
#undef RC_CE
    // farthest first, so the nearest pending sibling is popped first
    if (key[3] < INFINITY) st.push(ref[3]);
    if (key[2] < INFINITY) st.push(ref[2]);
    if (key[1] < INFINITY) st.push(ref[1]);
    cur = key[0] < INFINITY ? ref[0] : st.pop();
  } else {
    float tl, tr;
    bool hl, hr;
    uint32_t lref, rref;
    if (FAST && HALF) {
      const uint4* nh = sc.nodes_h + 2ull * cur;
      const uint4 a = nh[0], b = nh[1];
      hl = slab_half<SLACK>(lo16(a.x), hi16(a.x), lo16(a.y), hi16(a.y), lo16(a.z), hi16(a.z), fr, tl);
      hr = slab_half<SLACK>(lo16(a.w), hi16(a.w), lo16(b.x), hi16(b.x), lo16(b.y), hi16(b.y), fr, tr);
      lref = b.z;
      rref = b.w;
    } else {
      if (FAST && RAYCA_NODE_CH && RAYCA_NODE_CH48) {
        // (in this array an inner reference IS the record's byte offset, 48 x node index -- kChRefScale; < 2^31 for every tree the
        // 25-bit leaf references allow -- so the loads take the wave-uniform base from SGPRs and the reference as their 32-bit
        // offset: no address arithmetic at all, where a 48-B stride cost a quarter-rate 32- or 64-bit multiply per step)
        const float4* np = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(sc.nodes_ch) + cur);
        const float4 q0 = np[0], q1 = np[1], q2 = np[2];
        hl = slab_ch<SLACK>(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, fr, tl);
        hr = slab_ch<SLACK>(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, fr, tr);
        lref = __builtin_amdgcn_perm(__float_as_uint(q1.x), __float_as_uint(q0.w), 0x05040100u);   // low halves of (hy : hx)
        rref = __builtin_amdgcn_perm(__float_as_uint(q2.z), __float_as_uint(q2.y), 0x05040100u);
      } else {
        const float4* np = (FAST && RAYCA_NODE_CH ? sc.nodes_ch : sc.nodes) + 4ull * cur;
        const float4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
        if (FAST && RAYCA_NODE_CH) {
          hl = slab_ch<SLACK>(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, fr, tl);
          hr = slab_ch<SLACK>(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, fr, tr);
        } else if (FAST) {
          hl = slab_fast<SLACK>(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, fr, tl);
          hr = slab_fast<SLACK>(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, fr, tr);
        } else {
          hl = slab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, r, tl);
          hr = slab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, r, tr);
        }
        lref = __float_as_uint(q3.x);
        rref = __float_as_uint(q3.y);
      }
    }
    if (STATS) cnt.boxes += 2;
    if (ORDERED) {
      hl = hl && tl <= limit;
      hr = hr && tr <= limit;
    }
    if (hl && hr) {
      const bool left_first = !ORDERED || tl <= tr;
      st.push(left_first ? rref : lref);
      cur = left_first ? lref : rref;
    } else if (hl) {
      cur = lref;
    } else if (hr) {
      cur = rref;
    } else {
      cur = st.pop();
    }
  }
  return cur;
}

// Closest hit along `r` (Tlas::intersects).
//   ORDERED    front-to-back descent, subtrees whose entry distance exceeds the current best are
//              skipped.  The winner is the (t, reference order) lexicographic minimum, which is what
//              the reference's strict-< DFS returns (blas.rs:151,161,169).  The skip test carries a
//              slack (relative 2^-10 plus sc.cull_abs, plus the ray's own slack: cull_limit) because a
//              triangle's t and its box's slab entry are computed by different expressions and may
//              disagree in the last bits -- or, with a far origin, in all the bits c's rounding leaves.
//   !ORDERED   visits every leaf the reference visits (no culling), children in the reference's order.
//   FAST       conservative FMA slabs (only with the reference-leaf filter, see slab_fast).
//   WIDE       4-wide nodes: one 128-B fetch tests four boxes and skips every other level of the
//              binary tree (legal because a box that passes implies its ancestors pass).
//   t_stop     any-hit early out: stop as soon as a hit with t < t_stop is found (shadow rays,
//              "occluded iff closest depth < light distance", nee.rs:152-156).  FLT_MAX = never.
// Structure: "while-while" -- all lanes of the wave first descend inner nodes until each holds a leaf
// (or has finished), then the leaf lanes run the triangle tests together, so the expensive leaf code
// is not serialised against node steps of other lanes.  (A speculative variant -- a lane sets its first leaf
// aside and keeps descending until it holds a second -- was measured: soup -5.6 %, atrium +4 % to +10 %: the
// later leaf test delays the cull bound.  Not kept.)
// LEAVE_K: see the early-leave form below.  Per kernel class, measured with two frames in flight (atrium 1080p; K = 0 / 16 /
// 24 / 32): camera rays of a Flat frame 0.2056 / 0.2084 / 0.2088 / 0.2107 ms (coherent: the slowest search is not far behind
// the others, the ballots only cost), depth-1 frame 0.4271 / 0.4234 / 0.4257 / 0.4285, 5-deep frame on the wavefront
// engine 5.82 / 5.34 / 5.58 / 5.75 ms (K = 2 / 4 / 6 / 8 / 12: 5.50 / 5.18 / 5.14 / 5.14 / 5.23); the soup's camera rays on
// k_generation 10.6 / 8.05 / 7.92 / 7.91 ms (the lane-refill kernel, refill.hip, does them in 5.9).
#ifndef RAYCA_LEAVE_K_CAMERA
#define RAYCA_LEAVE_K_CAMERA 0    // camera rays of Flat frames
#endif
// (With the leaves of the cost model -- host_scene.hpp kLeafNodeCost -- and four frames in flight the depth-1 frame reads
// 0.3758 / 0.3796 / 0.3803 / 0.3833 ms for K = 0 / 6 / 12 / 24: the early leave no longer pays for generation 0, which went
// back to 0; profiles/r02_ab_leave_final.log.)
#ifndef RAYCA_LEAVE_K_PATH0
#define RAYCA_LEAVE_K_PATH0 0     // generation 0 of path frames: camera rays + their shadow rays
#endif
#ifndef RAYCA_LEAVE_K_BOUNCE
#define RAYCA_LEAVE_K_BOUNCE 8    // bounce generations, shadow rays of the wavefront engine, the stack machine
#endif
template <bool ORDERED, bool FAST, bool SPH, bool WIDE, bool SPILL, bool STATS, bool HALF, int LEAVE_K, bool SLACK, int STRIDE = kBlock>
__device__ __forceinline__ bool trace_search(const DevScene& sc, const DRay& r, const FastRay& fr, float t_stop, NodeStack<SPILL, STRIDE>& st, DHit& hit, LaneCounters& cnt) {
  hit.t = INFINITY;
  hit.prim = RAYCA_NONE;
  hit.u = hit.v = 0.0f;
  float tmin;
  if (STATS) cnt.boxes++;
  uint32_t cur = WIDE ? sc.root_ref4 : (FAST && !HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref);
  if (!slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], r, tmin)) cur = kTerminated;
  st.clear();
  const bool any_hit = ORDERED && t_stop < FLT_MAX;
  float limit = INFINITY;  // cull bound (ORDERED only)
  if (any_hit) limit = cull_limit<SLACK>(sc, fr, t_stop);
  if constexpr (LEAVE_K > 0) {
  // Early leave: the node phase ends as soon as fewer than LEAVE_K lanes of the wave are still searching and at
  // least one lane holds a leaf; the lanes that have not found theirs yet keep their inner node and go on in the next round.
  // Without it the phase lasts until the slowest search of the wave has found a leaf, with ever fewer lanes taking part.
  // Only the interleaving of lanes changes: every lane still performs its own steps in its own order (same result).
  for (;;) {
    for (;;) {
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<ORDERED, FAST, WIDE, SPILL, STATS, HALF, SLACK>(sc, r, fr, limit, cur, st, cnt);
    }
    if ((cur & kLeafFlag) && cur != kTerminated) {
      test_leaf<ORDERED, SPH, STATS, SLACK>(sc, r, fr, cur, t_stop, hit, limit, cnt);
      cur = (any_hit && hit.t < t_stop) ? kTerminated : st.pop();
    }
    if (__ballot(cur != kTerminated) == 0ull) break;
  }
  } else if constexpr (ORDERED && FAST && !WIDE && !HALF && RAYCA_NODE_CH && RAYCA_NODE_CH48) {
  // The node loop of the 48-B centre / half records, pipelined: node_step's box tests, then the decision as selects -- next
  // node = none ? newest stack entry : nearer child -- the next node's three loads issued AT ONCE, and only then the stack's
  // bookkeeping (NodeStack::book: one LDS write, one LDS read, each under one exec mask), which runs under those loads; the
  // pop's read lands in `top` itself and is waited for at the next decision, a node's worth of arithmetic later.  The same
  // decisions on the same operands as node_step (strict `tl <= tr`: left first on a tie): the same nodes and triangles in the
  // same order.  Measured (atrium depth-1 frame, four in flight; profiles/r06_ab_node_step.log): 0.3020 -> 0.2957 ms.  The
  // decision as selects WITHOUT the early loads (node_step's if / else-if chain replaced, loads at the loop's top as before)
  // is 5 % SLOWER than the chain: a coherent wave skips the chain's arms that no lane takes, the selects run on every step.
  while (cur != kTerminated) {
    if (!(cur & kLeafFlag)) {
      const float4* np = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(sc.nodes_ch) + cur);
      float4 q0 = np[0], q1 = np[1], q2 = np[2];
      bool more;
      do {
        if (STATS && cnt.books()) cnt.slot_boxes += 128ull;
        float tl, tr;
        bool hl = slab_ch<SLACK>(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, fr, tl);
        bool hr = slab_ch<SLACK>(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, fr, tr);
        const uint32_t lref = __builtin_amdgcn_perm(__float_as_uint(q1.x), __float_as_uint(q0.w), 0x05040100u);   // (as in node_step)
        const uint32_t rref = __builtin_amdgcn_perm(__float_as_uint(q2.z), __float_as_uint(q2.y), 0x05040100u);
        if (STATS) cnt.boxes += 2;
        hl = hl && tl <= limit;
        hr = hr && tr <= limit;
        const bool left_first = tl <= tr;
        const bool both = hl && hr, none = !(hl || hr);
        cur = none ? st.top : ((hl && (left_first || !hr)) ? lref : rref);
        more = !(cur & kLeafFlag) && cur != kTerminated;
        if (more) {
          const float4* nn = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(sc.nodes_ch) + cur);
          q0 = nn[0]; q1 = nn[1]; q2 = nn[2];
        }
        st.book(both, none, left_first ? rref : lref, cur);
      } while (more);
    }
    if (cur != kTerminated) {  // a leaf
      test_leaf<ORDERED, SPH, STATS, SLACK>(sc, r, fr, cur, t_stop, hit, limit, cnt);
      cur = st.pop_late(!(any_hit && hit.t < t_stop));   // (kTerminated ends the search of an any-hit ray)
    }
  }
  } else {
  while (cur != kTerminated) {
    while (!(cur & kLeafFlag) && cur != kTerminated) {
      cur = node_step<ORDERED, FAST, WIDE, SPILL, STATS, HALF, SLACK>(sc, r, fr, limit, cur, st, cnt);
    }
    if (cur != kTerminated) {  // a leaf
      test_leaf<ORDERED, SPH, STATS, SLACK>(sc, r, fr, cur, t_stop, hit, limit, cnt);
      if (any_hit && hit.t < t_stop) break;
      cur = st.pop();
    }
  }
  }
  return hit.prim != RAYCA_NONE;
}

// SLACK_FORM: which form of the steering tests the search takes (see ray_needs_slack).  kSlackPerWave: decided per wave, for
// kernels whose loop traces a camera ray and then its shadow rays (both forms are instantiated: the registers of the kernel are
// those of the larger one); kSlackAlways: camera rays alone (Flat frames, generation 0 of the wavefront engine -- measured
// neutral there); kSlackNever: bounce and shadow rays, whose origins lie on the scene's surfaces.
constexpr int kSlackPerWave = 0, kSlackAlways = 1, kSlackNever = 2;
template <bool ORDERED, bool FAST, bool SPH, bool WIDE, bool SPILL, bool STATS, bool HALF = false, int LEAVE_K = 0, int SLACK_FORM = kSlackPerWave, int STRIDE = kBlock>
__device__ __forceinline__ bool trace(const DevScene& sc, const DRay& r, float t_stop, NodeStack<SPILL, STRIDE>& st, DHit& hit, LaneCounters& cnt) {
  const FastRay fr = make_fast(sc, r, HALF);
  if constexpr (!FAST || !RAYCA_RAY_SLACK || SLACK_FORM == kSlackNever) {
    return trace_search<ORDERED, FAST, SPH, WIDE, SPILL, STATS, HALF, LEAVE_K, false>(sc, r, fr, t_stop, st, hit, cnt);
  } else if constexpr (SLACK_FORM == kSlackAlways) {
    return trace_search<ORDERED, FAST, SPH, WIDE, SPILL, STATS, HALF, LEAVE_K, true>(sc, r, fr, t_stop, st, hit, cnt);
  } else {
    if (__ballot(ray_needs_slack(sc, r, fr)) != 0ull)   // (wave-uniform)
      return trace_search<ORDERED, FAST, SPH, WIDE, SPILL, STATS, HALF, LEAVE_K, true>(sc, r, fr, t_stop, st, hit, cnt);
    return trace_search<ORDERED, FAST, SPH, WIDE, SPILL, STATS, HALF, LEAVE_K, false>(sc, r, fr, t_stop, st, hit, cnt);
  }
}

// ---- ray queries (rayca_hip_query_device): the bound of a caller's ray and its result ------------
// A hit counts iff t < tmax, strictly (the comparison trace() makes for t_stop, nee.rs:152-156).  The bound as the
// traversal carries it: FLT_MAX = unbounded (tmax = +inf or FLT_MAX); `dead`: tmax is NaN or <= 0, nothing can count.
__device__ __forceinline__ float query_bound(const QueryIo& q, uint32_t i, bool& dead) {
  const float tm = q.tmax ? q.tmax[i] : q.tmax_all;
  dead = !(tm > 0.0f);
  return tm < FLT_MAX ? tm : FLT_MAX;
}
__device__ __forceinline__ bool query_found(const DHit& hit, float bound) { return hit.prim != RAYCA_NONE && (bound == FLT_MAX || hit.t < bound); }
// the record k_trace_rays writes, or the miss record; one byte for the occlusion form
template <bool OCCLUDED>
__device__ __forceinline__ void query_store(const QueryIo& q, uint32_t i, const DHit& hit, bool found) {
  if (OCCLUDED) {
    q.occluded_out[i] = found ? 1 : 0;
  } else {
    if (q.t_out) q.t_out[i] = found ? hit.t : FLT_MAX;
    if (q.prim_out) q.prim_out[i] = found ? hit.prim : RAYCA_NONE;
    if (q.uv_out) {
      q.uv_out[2ull * i] = found ? hit.u : 0.0f;
      q.uv_out[2ull * i + 1ull] = found ? hit.v : 0.0f;
    }
  }
}

// ---- surface data (HitInfo, rayca-soft/src/hit.rs) ---------------------------------------------
__device__ __forceinline__ Color load_color(const float* c) { return Color{c[0], c[1], c[2], c[3]}; }
__device__ __forceinline__ F4 load_vec3(const float* c) { return vec3(c[0], c[1], c[2]); }

__device__ __forceinline__ uint32_t f32_as_u32_sat(float v) {  // Rust `as u32`
  if (!(v == v) || v <= 0.0f) return 0u;
  if (v >= 4294967296.0f) return 0xFFFFFFFFu;
  return (uint32_t)v;
}
// Sampler::sample  rayca-model/src/sampler.rs:11-30 (nearest, wrap)
__device__ Color sample_texture(const DevScene& sc, uint32_t tex, F2 uv) {
  const DevTexture t = sc.textures[tex];
  const float fx = (uv.x - floorf(uv.x) + 1.0f) * (float)t.width;
  const float fy = (uv.y - floorf(uv.y) + 1.0f) * (float)t.height;
  const uint32_t x = f32_as_u32_sat(fx) % t.width, y = f32_as_u32_sat(fy) % t.height;
  const size_t idx = (size_t)y * t.width + x;
  const uint8_t* base = sc.image_bytes + t.byte_offset;
  if (t.color_type == RAYCA_COLOR_RGBA32F) {
    const float* f = reinterpret_cast<const float*>(base) + idx * 4;
    return Color{f[0] / 255.0f, f[1] / 255.0f, f[2] / 255.0f, f[3] / 255.0f};
  }
  if (t.color_type == RAYCA_COLOR_RGBA8) {
    const uint8_t* p = base + idx * 4;
    return Color{(float)p[0] / 255.0f, (float)p[1] / 255.0f, (float)p[2] / 255.0f, (float)p[3] / 255.0f};
  }
  const uint8_t* p = base + idx * 3;
  return Color{(float)p[0] / 255.0f, (float)p[1] / 255.0f, (float)p[2] / 255.0f, 255.0f / 255.0f};
}

__device__ __forceinline__ bool tex_valid(const DevScene& sc, uint32_t t) { return t != RAYCA_NONE && t < sc.texture_count; }

__device__ __forceinline__ Color pbr_color(const DevScene& sc, const DevMaterial& m, F2 uv) {  // pbr.rs:94-102
  const Color c = load_color(m.color);
  if (tex_valid(sc, m.albedo_texture)) return c * sample_texture(sc, m.albedo_texture, uv);
  return c;
}
__device__ __forceinline__ void pbr_metallic_roughness(const DevScene& sc, const DevMaterial& m, F2 uv, float& metallic, float& roughness) {
  if (tex_valid(sc, m.metallic_roughness_texture)) {  // pbr.rs:125-137: (b, r)
    const Color c = sample_texture(sc, m.metallic_roughness_texture, uv);
    metallic = c.b;
    roughness = c.r;
  } else {
    metallic = m.metallic_factor;
    roughness = m.roughness_factor;
  }
}
__device__ __forceinline__ DevMaterial default_material() {  // Material::DEFAULT -> PbrMaterial::WHITE
  DevMaterial m{};
  m.color[0] = m.color[1] = m.color[2] = m.color[3] = 1.0f;
  m.ambient[3] = m.emission[3] = m.diffuse[3] = m.specular[3] = 1.0f;
  m.kind = RAYCA_MATERIAL_PBR;
  m.albedo_texture = m.normal_texture = m.metallic_roughness_texture = RAYCA_NONE;
  m.metallic_factor = 0.0f;
  m.roughness_factor = 1.0f;
  return m;
}

__device__ __forceinline__ F4 interp3(const float (*a)[3], float bu, float bv) {
  const float w2 = 1.0f - bu - bv;
  return (load_vec3(a[2]) * w2 + load_vec3(a[0]) * bu) + load_vec3(a[1]) * bv;
}

// HitInfo (rayca-soft/src/hit.rs) reduced to the values the rest of the path vertex needs; everything
// here is a pure function of the hit, so evaluating it once instead of lazily gives the same bits.
struct ShadeCtx {
  F4 point, normal, view, next_origin;  // hit point, shading normal, -ray.dir, point + normal*BIAS
  Color kd, ks;                         // get_diffuse(), get_specular()
  float roughness, shininess;
  uint32_t kind;                        // RAYCA_MATERIAL_*
};

// The path kernel keeps a vertex's ShadeCtx in LDS while its shadow rays are traversed (RAYCA_PARK_CTX): the struct is 27
// registers that would otherwise have to survive the traversal loop, which at the 128 VGPRs of four waves per SIMD the
// compiler could only do through scratch (54 spilled VGPRs, 219 MB of scratch writes per 1080p frame).  So do the pending
// sample's contribution and the running sum of direct light.  float4 quads per lane, quantity-major (lane i of quantity q at
// [q * STRIDE + i], STRIDE = the workgroup's threads): a wave's ds_read_b128 / ds_write_b128 touch 64
// consecutive 16-B slots, the conflict-free shape.  next_origin and the w lanes are recomputed (same operations, same bits).
#ifndef RAYCA_PARK_CTX
#define RAYCA_PARK_CTX 1
#endif
// RAYCA_CTX_COMPACT (default 1): the parked words cut to what the vertex still needs, 104 B per lane instead of 112, so that a wave's
// context and four stack rows are 7 680 B and twenty waves fit a CU's 160 KiB (fused_generation).  Five quads and six words:
//   quad 0  point.xyz, roughness OR shininess   surf_brdf reads shininess only for Phong and roughness only otherwise: one word, chosen by kind
//   quad 1  normal.xyz, kind
//   quad 2  view.xyz, (free)
//   quad 3  kd            quad 4  ks
//   words 0-2  the pending sample as x.rgb * x.a -- all operator+ ever reads of it; "not lit" adds +0.0f, which is black()'s 0 * 1
//   words 3-5  the running direct sum's r, g, b -- its alpha is 1.0 throughout (it starts as black() and operator+ keeps the left alpha)
// The words are quantity-major like the quads (word w of lane i at [w * STRIDE + i]): a wave's ds_read / ds_write touch 64 consecutive
// dwords.  With -ffp-contract=off the product and the sum round separately in both layouts: the same bits.
// -DRAYCA_CTX_COMPACT=0: seven whole quads (the context's five, the sample, the sum), the layout as it was, for A/B runs.
#ifndef RAYCA_CTX_COMPACT
#define RAYCA_CTX_COMPACT 1
#endif
#if RAYCA_CTX_COMPACT
constexpr uint32_t kCtxQuads = 5, kCtxWords = 6;
#else
constexpr uint32_t kCtxQuads = 7, kCtxWords = 0;  // ShadeCtx (5) + the pending NEE sample's contribution + the running direct sum
#endif
constexpr uint32_t kCtxBytes = kCtxQuads * 16u + kCtxWords * 4u;  // per lane
// A workgroup's parked contexts: the quads, and the words behind them.  A lane's slot of either is found where it is used,
// from the lane's number made on the spot in a one-wave workgroup (two v_mbcnt; the empty-input asm cannot be hoisted or merged):
// as pointers made at the kernel's entry the two slots were two registers live over the traversal loops, which at 96 registers the
// compiler kept in scratch across every trace() call.
struct CtxSlot {
  uint32_t* base;
};
template <int STRIDE>
__device__ __forceinline__ uint32_t ctx_tid() {
  if (STRIDE != 64) return rc_tid();
  uint32_t l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// The lane's number made where it is read, the same way: __lane_id() at the kernel's entry is one value for the whole kernel, which
// the fused path form, with its pixel tail behind the loop, kept in scratch from the entry to the last counter's `lane == 0`.
__device__ __forceinline__ uint32_t lane_now() {
  uint32_t l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
template <int STRIDE>
__device__ __forceinline__ float4* ctx_quads(const CtxSlot& s) { return reinterpret_cast<float4*>(s.base) + ctx_tid<STRIDE>(); }
template <int STRIDE>
__device__ __forceinline__ float* ctx_words(const CtxSlot& s) { return reinterpret_cast<float*>(s.base + kCtxQuads * 4u * STRIDE) + ctx_tid<STRIDE>(); }
template <int STRIDE = kBlock>
__device__ __forceinline__ void park_ctx(const CtxSlot& s, const ShadeCtx& c) {
  float4* const slot = ctx_quads<STRIDE>(s);
#if RAYCA_CTX_COMPACT
  slot[0 * STRIDE] = make_float4(c.point.x, c.point.y, c.point.z, c.kind == RAYCA_MATERIAL_PHONG ? c.shininess : c.roughness);
  slot[1 * STRIDE] = make_float4(c.normal.x, c.normal.y, c.normal.z, __uint_as_float(c.kind));
  slot[2 * STRIDE] = make_float4(c.view.x, c.view.y, c.view.z, 0.0f);
#else
  slot[0 * STRIDE] = make_float4(c.point.x, c.point.y, c.point.z, c.roughness);
  slot[1 * STRIDE] = make_float4(c.normal.x, c.normal.y, c.normal.z, c.shininess);
  slot[2 * STRIDE] = make_float4(c.view.x, c.view.y, c.view.z, __uint_as_float(c.kind));
#endif
  slot[3 * STRIDE] = make_float4(c.kd.r, c.kd.g, c.kd.b, c.kd.a);
  slot[4 * STRIDE] = make_float4(c.ks.r, c.ks.g, c.ks.b, c.ks.a);
}
template <int STRIDE = kBlock>
__device__ __forceinline__ ShadeCtx unpark_ctx(const CtxSlot& s) {
  const float4* const slot = ctx_quads<STRIDE>(s);
  const float4 q0 = slot[0 * STRIDE], q1 = slot[1 * STRIDE], q2 = slot[2 * STRIDE], q3 = slot[3 * STRIDE], q4 = slot[4 * STRIDE];
  ShadeCtx c;
  c.point = f4(q0.x, q0.y, q0.z, 1.0f);   // Hit.point is a Point3
  c.normal = vec3(q1.x, q1.y, q1.z);
  c.view = vec3(q2.x, q2.y, q2.z);
  c.next_origin = c.point + c.normal * kRayBias;  // hit.rs:164-171, as in shade_hit
  c.kd = Color{q3.x, q3.y, q3.z, q3.w};
  c.ks = Color{q4.x, q4.y, q4.z, q4.w};
#if RAYCA_CTX_COMPACT
  c.roughness = c.shininess = q0.w;   // (the one surf_brdf reads for this kind)
  c.kind = __float_as_uint(q1.w);
#else
  c.roughness = q0.w;
  c.shininess = q1.w;
  c.kind = __float_as_uint(q2.w);
#endif
  return c;
}
// The running sum of a vertex's direct samples and the pending sample, behind the context.
// park_sum_reset: the sum = black().  (Made from a zero the compiler cannot hoist: as a loop-invariant value it sat in registers over
// the whole batch loop, which the counting instantiations could only afford through scratch: with the pipelined node
// loop k_generation<1, true, true, false, true, SPH, false, false, true, HALF> went from 0-2 to 4 spilled VGPRs and
// k_generation<1, true, false, false, FAST, *, false, true, true, false> from 0-4 to 2-5 -- tests/kernel_resources.py)
template <int STRIDE = kBlock>
__device__ __forceinline__ void park_sum_reset(const CtxSlot& s) {
  float zero = 0.0f;
  asm volatile("" : "+v"(zero));
#if RAYCA_CTX_COMPACT
  float* const words = ctx_words<STRIDE>(s);
  words[3 * STRIDE] = zero;
  words[4 * STRIDE] = zero;
  words[5 * STRIDE] = zero;
#else
  ctx_quads<STRIDE>(s)[6 * STRIDE] = make_float4(zero, zero, zero, 1.0f);
#endif
}
// park_sum_set: the sum = c, whose alpha is 1 (black() + x): the fused path frame's pixel sum of a lane that ends without samples
template <int STRIDE = kBlock>
__device__ __forceinline__ void park_sum_set(const CtxSlot& s, Color c) {
#if RAYCA_CTX_COMPACT
  float* const words = ctx_words<STRIDE>(s);
  words[3 * STRIDE] = c.r;
  words[4 * STRIDE] = c.g;
  words[5 * STRIDE] = c.b;
#else
  ctx_quads<STRIDE>(s)[6 * STRIDE] = make_float4(c.r, c.g, c.b, c.a);
#endif
}
// park_sample: the contribution the pending sample makes if its light turns out to be visible
template <int STRIDE = kBlock>
__device__ __forceinline__ void park_sample(const CtxSlot& s, Color x) {
#if RAYCA_CTX_COMPACT
  float* const words = ctx_words<STRIDE>(s);
  words[0 * STRIDE] = x.r * x.a;
  words[1 * STRIDE] = x.g * x.a;
  words[2 * STRIDE] = x.b * x.a;
#else
  ctx_quads<STRIDE>(s)[5 * STRIDE] = make_float4(x.r, x.g, x.b, x.a);
#endif
}
// park_sum_add: sum = sum + (lit ? the pending sample : black())
template <int STRIDE = kBlock>
__device__ __forceinline__ void park_sum_add(const CtxSlot& s, bool lit) {
#if RAYCA_CTX_COMPACT
  float* const words = ctx_words<STRIDE>(s);
  const float r = words[3 * STRIDE] + (lit ? words[0 * STRIDE] : 0.0f);
  const float g = words[4 * STRIDE] + (lit ? words[1 * STRIDE] : 0.0f);
  const float b = words[5 * STRIDE] + (lit ? words[2 * STRIDE] : 0.0f);
  words[3 * STRIDE] = r;
  words[4 * STRIDE] = g;
  words[5 * STRIDE] = b;
#else
  float4* const quads = ctx_quads<STRIDE>(s);
  const float4 a = quads[6 * STRIDE], x = quads[5 * STRIDE];
  const Color sum = Color{a.x, a.y, a.z, a.w} + (lit ? Color{x.x, x.y, x.z, x.w} : black());
  quads[6 * STRIDE] = make_float4(sum.r, sum.g, sum.b, sum.a);
#endif
}
template <int STRIDE = kBlock>
__device__ __forceinline__ Color unpark_sum(const CtxSlot& s) {
#if RAYCA_CTX_COMPACT
  const float* const words = ctx_words<STRIDE>(s);
  // (the alpha made here, like park_sum_reset's zero: as a loop-invariant lane of the colour's register tuple it went to scratch
  // at the kernel's entry and came back, with the whole tuple, once per vertex)
  float one = 1.0f;
  asm volatile("" : "+v"(one));
  return Color{words[3 * STRIDE], words[4 * STRIDE], words[5 * STRIDE], one};
#else
  const float4 a = ctx_quads<STRIDE>(s)[6 * STRIDE];
  return Color{a.x, a.y, a.z, a.w};
#endif
}

// get_color (primitive.rs:142-148) always; the rest only when `full` (Pathtracer).
// barycentrics: u -> vertex 0, v -> vertex 1, 1-u-v -> vertex 2 (bvh/triangle.rs:34-38)
template <bool SPH>
__device__ __forceinline__ void shade_hit(const DevScene& sc, const DRay& ray, const DHit& hit, bool full, Color& color, bool& emissive,
                                          ShadeCtx& cx) {
  const PrimExt& e = sc.ext[hit.prim];
  const float bu = hit.u, bv = hit.v;
  const float w2 = 1.0f - bu - bv;
  const bool is_sphere = SPH && e.kind == RAYCA_GEOMETRY_SPHERE;
  // BvhGeometry::get_color / get_uv: spheres are white with uv (0,0)  (primitive.rs:15-28)
  const Color geom_color = is_sphere ? white() : (load_color(e.color[2]) * w2 + load_color(e.color[0]) * bu) + load_color(e.color[1]) * bv;
  const F2 uv = is_sphere ? F2{0.0f, 0.0f}
                          : F2{(e.uv[2][0] * w2 + e.uv[0][0] * bu) + e.uv[1][0] * bv, (e.uv[2][1] * w2 + e.uv[0][1] * bu) + e.uv[1][1] * bv};
  const DevMaterial m = (e.material != RAYCA_NONE && e.material < sc.material_count) ? sc.materials[e.material] : default_material();
  Color mc;  // Material::get_color  material/mod.rs:107-113
  if (m.kind == RAYCA_MATERIAL_PBR) mc = pbr_color(sc, m, uv);
  else if (m.kind == RAYCA_MATERIAL_PHONG) mc = load_color(m.ambient) + load_color(m.emission);
  else mc = load_color(m.diffuse);
  color = geom_color * mc;
  emissive = m.emissive != 0u;
  if (!full) return;
  // normal: primitive.rs:172-182 -> material/mod.rs:125-139 -> pbr.rs:104-123
  F4 normal;
  F4 point = ray.o + ray.d * hit.t;  // Hit.point  triangle.rs:122
  F4 hit_dir = ray.d;                // Hit.ray.dir
  if (is_sphere) {  // primitive.rs:183-190 and sphere.rs:155-163
    const DevSphere& sp = sc.spheres[e.node];
    const DRay l = sphere_local_ray(sp, ray);
    // Sphere::intersects builds its Hit from the INVERSE-TRANSFORMED ray (sphere.rs:138,157-159): everything
    // HitInfo later derives from hit.ray -- view vector, reflection, the transmitted ray -- is in the sphere's
    // model space.  Reproduced as is.
    hit_dir = l.d;
    const F4 model_point = l.o + l.d * hit.t;
    const Trs wt{f4(sp.translation[0], sp.translation[1], sp.translation[2], 0.0f), f4(sp.rotation[0], sp.rotation[1], sp.rotation[2], sp.rotation[3]),
                 f4(sp.scale[0], sp.scale[1], sp.scale[2], 0.0f)};
    point = trs_apply_point(wt, model_point);
    const F4 hp = mat4_apply_point(reinterpret_cast<const float(*)[4]>(sp.inv_mat4), point);
    const F4 mn = normalized(as_vec(hp - f4(sp.center[0], sp.center[1], sp.center[2], sp.center[3])));
    const float* nm = sp.normal_mat;
    float out[3] = {0.0f, 0.0f, 0.0f};
    const float in[3] = {mn.x, mn.y, mn.z};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) out[i] += nm[4 * i + j] * in[j];
    normal = normalized(vec3(out[0], out[1], out[2]));
  } else {
    normal = normalized(interp3(e.normal, bu, bv));
  }
  if (!is_sphere && m.kind == RAYCA_MATERIAL_PBR && tex_valid(sc, m.normal_texture)) {
    const F4 tangent = normalized(interp3(e.tangent, bu, bv));
    const F4 bitangent = normalized(interp3(e.bitangent, bu, bv));
    F4 sn = premultiplied(sample_texture(sc, m.normal_texture, uv));
    sn = sn * 2.0f - f4(1.0f, 1.0f, 1.0f, 1.0f);
    normal = normalized(mat3_apply(mat3_tbn(tangent, bitangent, normal), sn));
  }
  cx.normal = normal;
  cx.point = point;
  cx.view = -hit_dir;                // ray.rs:149-151
  cx.next_origin = cx.point + normal * kRayBias;  // hit.rs:164-171
  cx.kind = m.kind;
  cx.shininess = m.shininess;
  // get_diffuse  primitive.rs:150-155 ; get_specular / get_roughness  material/mod.rs:141-151,173-185
  if (m.kind == RAYCA_MATERIAL_PBR) {
    float me, ro;
    pbr_metallic_roughness(sc, m, uv, me, ro);
    const Color base = pbr_color(sc, m, uv);
    cx.kd = geom_color * base;
    cx.ks = me * base;
    cx.roughness = ro;
  } else {
    cx.kd = geom_color * load_color(m.diffuse);
    cx.ks = load_color(m.specular);
    cx.roughness = m.kind == RAYCA_MATERIAL_PHONG ? clampf(sqrtf(2.0f / (m.shininess + 2.0f)), 0.0f, 1.0f) : m.roughness_factor;
  }
}

// ---- BRDFs: brdf/ggx.rs:58-129, brdf/lambertian.rs:7-16 -----------------------------------------
// The reference spells these terms with libm compositions -- tan(acos(c))^2, powf(c, 4), powf(x, 5)
// (ggx.rs:58-129) -- ~1500 VALU instructions per BRDF evaluation on this chip, a fifth of the bench frame's
// arithmetic.  RAYCA_GGX_CLOSED_FORM (default) evaluates the same quantities in closed form,
//   tan^2(acos c) = (1-c)(1+c)/c^2,   c^4 (a^2 + tan^2)^2 = (a^2 c^2 + (1-c)(1+c))^2,   x^5 = (x^2)^2 x,
// each within 4e-7 of the exact value (measured over cosines 1e-4 .. 1 - 6e-8 and roughness 1 .. 1e-3: D 3.4e-7, G1 1.6e-7, x^5
// 1.9e-7 relative), where the f32 composition itself is only good to the rounding of acosf amplified by 1/c: D to 4e-3 and G1 to
// 1e-3 on the same cosines, and the CPU restatement's pixels, which keep the reference's spelling, to 2e-3 of the float64 value
// on a telephoto frame along a surface (n.wo 2e-2 .. 1e-4) where these stay within 6e-7 (profiles/shading_edges.log).  Shaded
// pixels are held to a float64 evaluation of the reference's formulas at grazing angles, roughness down to 0 and the special
// cases below (tests/test_gpu_shading_edges.py), and compared with the CPU restatement at the 1e-4 tolerance of the parity tests
// (on those frames within 3e-5 of it); hit records are unaffected.
// Special cases of the composition are kept: c == 0 gives D = 0 (cos^4 underflows first), c > 1 gives NaN (acosf).
#ifndef RAYCA_GGX_CLOSED_FORM
#define RAYCA_GGX_CLOSED_FORM 1
#endif
__device__ __forceinline__ float ggx_d(float a, F4 h, F4 n) {
  const float a2 = a * a;
  const float cos_theta = clampf(dot(h, n), 0.0f, 1.0f);
#if RAYCA_GGX_CLOSED_FORM
  const float q = a2 * (cos_theta * cos_theta) + (1.0f - cos_theta) * (1.0f + cos_theta);
  const float denominator = q * q;
  if (denominator == 0.0f || cos_theta == 0.0f) return 0.0f;
#else
  const float theta = acosf(cos_theta);
  const float denominator = powf(cos_theta, 4.0f) * powf(a2 + powf(tanf(theta), 2.0f), 2.0f);
  if (denominator == 0.0f) return 0.0f;
#endif
  return a2 * kFrac1Pi / denominator;
}
__device__ __forceinline__ float ggx_g1(float a, F4 omega, F4 n) {
  const float cos_theta = dot(omega, n);
  if (cos_theta <= 0.0f) return 0.0f;
#if RAYCA_GGX_CLOSED_FORM
  const float tan2 = cos_theta > 1.0f ? NAN : ((1.0f - cos_theta) * (1.0f + cos_theta)) / (cos_theta * cos_theta);
  return 2.0f / (1.0f + sqrtf(1.0f + a * a * tan2));
#else
  const float theta = acosf(cos_theta);
  return 2.0f / (1.0f + sqrtf(1.0f + a * a * powf(tanf(theta), 2.0f)));
#endif
}
__device__ __forceinline__ Color ggx_f(Color ks, F4 omega_i, F4 h) {
  const float oh = fabsf(dot(omega_i, h));
#if RAYCA_GGX_CLOSED_FORM
  const float x = 1.0f - oh, x2 = x * x;
  return ks + (white() - ks) * ((x2 * x2) * x);
#else
  return ks + (white() - ks) * powf(1.0f - oh, 5.0f);
#endif
}
// inlined: as a call it kept ShadeCtx in scratch and cost 2.6 % of the depth-1 frame
__device__ __forceinline__ Color surf_brdf(const ShadeCtx& s, F4 omega_i) {  // HitInfo::get_brdf  hit.rs:220-227
  if (s.kind == RAYCA_MATERIAL_PHONG) {  // lambertian::get_brdf
    const Color lambertian = s.kd * kFrac1Pi;
    const float sh = s.shininess;
    const F4 refl = normalized(reflect(-s.view, s.normal));  // hit.rs:93-101 (ray.dir == -view exactly)
    const Color specular = (((s.ks * (sh + 2.0f)) * powf(dot(refl, omega_i), sh)) * kFrac1Pi) / 2.0f;
    return lambertian + specular;
  }
  Color bsdf = black();  // ggx::get_bsdf
  const F4 omega_o = s.view;
  const F4 n = s.normal;
  const float oin = clampf(dot(omega_i, n), 0.0f, 1.0f);
  const float oon = clampf(dot(omega_o, n), 0.0f, 1.0f);
  if (!(oin == 0.0f || oon == 0.0f)) {
    const float a = s.roughness;
    const F4 h = normalized(omega_i + omega_o);
    const Color f = ggx_f(s.ks, omega_i, h);
    const float g = ggx_g1(a, omega_i, n) * ggx_g1(a, omega_o, n);
    const float d = ggx_d(a, h, n);
    const float denominator = 4.0f * oin * oon;
    bsdf = ((f * g) * d) / denominator;
  }
  return s.kd * kFrac1Pi + bsdf;
}

// ---- work distribution ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t xcc_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 7u;
}
// Next 64-wide batch for this wave, or RAYCA_NONE.  The batch list is cut into 8 contiguous
// partitions, one per XCD: waves drain their own XCD's partition first (neighbouring image tiles ->
// the same L2), then steal from the others.  Placement only affects speed, never results.
// Tickets: each of the 8 counters lives on its own 256-B line (kHeadStride dwords apart) -- atomics on
// one line serialise in one L2 channel at ~12 ns each, which for 32k batches would be as long as the
// whole kernel -- and one ticket covers `ticket` consecutive batches: two when the frame has batches to spare, one
// when there are fewer batches than resident waves (a rank's share of a frame on eight GPUs): pairs would then
// leave half the waves without work and double the time of the others.
constexpr uint32_t kHeadStride = 64;
constexpr uint32_t kCounterSetWords = 8u * kHeadStride;   // one set of work counters: what a fused k_generation launch zeroes of the other set
struct WorkCursor {   // (an aggregate: `WorkCursor wc{};`)
  uint32_t exhausted;  // partitions found empty so far
  uint32_t next, end;  // batches of the current ticket still to do
};
__device__ __forceinline__ uint32_t next_batch(uint32_t* heads, uint32_t total, uint32_t home, WorkCursor& wc, uint32_t ticket) {
  if (wc.next < wc.end) return wc.next++;
  ticket = max(ticket, 1u);  // a zero ticket would never drain the counters
  while (wc.exhausted < 8u) {
    const uint32_t part = (home + wc.exhausted) & 7u;
    const uint32_t lo = (uint32_t)(((uint64_t)part * total) >> 3), hi = (uint32_t)(((uint64_t)(part + 1u) * total) >> 3);
    uint32_t idx = 0;
    if (__lane_id() == 0) idx = atomicAdd(&heads[part * kHeadStride], ticket);
    idx = __builtin_amdgcn_readfirstlane(idx);
    if (idx < hi - lo) {
      wc.next = lo + idx + 1u;
      wc.end = min(lo + idx + ticket, hi);
      return lo + idx;
    }
    wc.exhausted++;
  }
  return RAYCA_NONE;
}

struct PathBuffers {
  float4* direct;   // [depth][npix] Color: direct lighting, or the terminal colour
  float4* brdf;     // [depth][npix] Color: factor get_radiance applies to the child's radiance
  uint32_t* state;  // [depth][npix] kVertex*
  uint32_t npix;
};

__device__ __forceinline__ float4 as_f4(Color c) { return make_float4(c.r, c.g, c.b, c.a); }
__device__ __forceinline__ Color as_color(float4 c) { return Color{c.x, c.y, c.z, c.w}; }

// scene.rs:146-148: color /= spp; correct_gamma; RGBA8::from
__device__ __forceinline__ void finalize_pixel(const FrameParams& fp, Color acc, uint32_t p, uint8_t* rgba8, float4* rgba32f) {
  Color c = acc / (float)fp.spp;
  if (fp.inv_gamma != 1.0f) {
    c.r = powf(c.r, fp.inv_gamma);
    c.g = powf(c.g, fp.inv_gamma);
    c.b = powf(c.b, fp.inv_gamma);
  }
  if (rgba32f) rgba32f[p] = as_f4(c);
  if (rgba8) {
    const uint32_t packed = (uint32_t)quantize(c.r) | ((uint32_t)quantize(c.g) << 8) | ((uint32_t)quantize(c.b) << 16) | ((uint32_t)quantize(c.a) << 24);
    reinterpret_cast<uint32_t*>(rgba8)[p] = packed;
  }
}

// Camera ray of output pixel (x, packed row r): scene.rs:125-141 + trs.rs:275-284 + ray.rs:74-91
__device__ __forceinline__ DRay camera_ray(const FrameParams& fp, uint32_t x, uint32_t y) {
  const float xx = (2.0f * ((((float)x + fp.sub_step_x) + fp.sub_offset) * fp.inv_width) - 1.0f) * fp.angle * fp.aspect;
  const float yy = (1.0f - 2.0f * ((((float)y + fp.sub_step_y) + fp.sub_offset) * fp.inv_height)) * fp.angle;
  F4 dir = normalized(vec3(xx, yy, -1.0f));
  F4 origin = point3(0.0f, 0.0f, 0.0f);
  // Ray::scale
  dir = dir * fp.camera.scale;
  origin = point_scale(origin, fp.camera.scale);
  // Ray::rotate
  dir = rotate(dir, fp.camera.rotation);
  origin = point_rotate(origin, fp.camera.rotation);
  origin.w = 1.0f;
  // Ray::translate
  origin = origin + fp.camera.translation;
  DRay r;
  r.o = origin;
  r.d = dir;
  r.rd = reciprocal(dir);
  return r;
}

// wave-aggregated append of the next generation's rays
__device__ __forceinline__ void push_ray(bool has, const QueuedRay& qr, QueuedRay* out, uint32_t* out_count) {
  const unsigned long long mask = __ballot(has);
  if (mask == 0ull) return;
  const uint32_t lane = __lane_id();
  const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(out_count, (uint32_t)__popcll(mask));
  base = __shfl(base, (int)leader);
  if (has) out[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = qr;
}

constexpr int kModeFlat = 0, kModePath = 1, kModeGeneral = 2;

// One NEE sample (sampler/nee.rs:72-166), split around its shadow ray: everything that does not depend
// on the shadow ray's outcome is evaluated first (pure functions, same values), so that only the
// candidate contribution `x` has to survive the traversal.
struct NeeSample {
  Color x;       // contribution if the light turns out to be visible
  float t_stop;  // point light: its distance (any-hit bound); quad light: FLT_MAX (closest hit wanted)
  uint32_t quad; // 1: "lit iff the closest hit is emissive" (nee.rs:103-104)
};
__device__ __forceinline__ NeeSample nee_prepare(const DevScene& sc, const FrameParams& fp, const ShadeCtx& s, uint32_t li, uint32_t k,
                                                 uint32_t key, uint32_t& dim, DRay& shadow_ray) {
  const DevLight L = sc.lights[li];
  NeeSample ns;
  const F4 x_point = s.point;
  if (L.kind == RAYCA_LIGHT_POINT) {  // get_point_light_sample  nee.rs:127-166
    const F4 x1 = f4(L.position[0], L.position[1], L.position[2], L.position[3]);
    const F4 x_to_x1 = as_vec(x1 - x_point);
    const float dist = length(x_to_x1);
    const F4 omega = normalized(x_to_x1);
    shadow_ray = make_ray(s.next_origin, omega);
    // PointLight::get_intensity / get_fallof  light/point.rs:37-49
    const F4 dvec = to_vec(x_point) - to_vec(x1);
    const float r2 = norm2(dvec);
    const float rr = sqrtf(r2);
    const float fallof = hsum(f4(L.attenuation[0], L.attenuation[1], L.attenuation[2], 0.0f) * f4(1.0f, rr, r2, 0.0f));
    const Color le = (L.intensity * load_color(L.color)) / fallof;
    const Color brdf = surf_brdf(s, omega);
    const float r_squared = norm2(x_to_x1);
    const float d_omega = 1.0f / r_squared;
    const float n_dot_omega = clampf(dot(s.normal, omega), 0.0f, 1.0f);
    ns.x = ((le * brdf) * n_dot_omega) * d_omega;
    ns.t_stop = dist;
    ns.quad = 0u;
  } else {  // get_quad_light_sample  nee.rs:72-125 ; QuadLight::get_random_point  light/quad.rs:112-135
    const F4 ab = f4(L.ab[0], L.ab[1], L.ab[2], 0.0f), ac = f4(L.ac[0], L.ac[1], L.ac[2], 0.0f);
    const float sc_f = (float)fp.strate_count;
    const float u1 = rng_f32(key, dim++) / sc_f;
    const float u2 = rng_f32(key, dim++) / sc_f;
    const F4 a = f4(L.position[0], L.position[1], L.position[2], L.position[3]);
    F4 x1 = (a + u1 * ab) + u2 * ac;
    if (fp.light_stratify) {
      const float i1 = (float)(k % fp.strate_count), i2 = (float)(k / fp.strate_count);
      x1 = x1 + ((ab / sc_f) * i1 + (ac / sc_f) * i2);
    }
    const F4 x_to_x1 = as_vec(x1 - x_point);
    const F4 omega = normalized(x_to_x1);
    shadow_ray = make_ray(s.next_origin, omega);
    const Color le = L.intensity * load_color(L.color);
    const Color brdf = surf_brdf(s, omega);
    const float r_squared = norm2(x_to_x1);
    const float d_omega = dot(f4(L.normal[0], L.normal[1], L.normal[2], 0.0f), omega) / r_squared;
    const float n_dot_omega = clampf(dot(s.normal, omega), 0.0f, 1.0f);
    ns.x = (((le * L.area) * brdf) * n_dot_omega) * d_omega;
    ns.t_stop = FLT_MAX;
    ns.quad = 1u;
  }
  return ns;
}

// An NEE sample whose shadow ray need not be traced: its candidate contribution is zero in r, g and b (the surface faces away
// from the light: n_dot_omega clamps to 0; a zero BRDF; a light of intensity 0) and its alpha is
// finite.  The outcome of the traversal then cannot change a bit of the pixel:
//   - every consumer adds the sample with operator+(Color a, Color b) = (a.rgb + b.rgb * b.a, a.a), and "not lit" adds black() =
//     (0, 0, 0, 1): the terms are +-0 * finite = +-0 against +0 * 1 = +0, and alpha stays a.a either way;
//   - the sum the sample joins starts at +0 per channel, and a float sum that starts at +0 never becomes -0 under round to nearest
//     (x + y is -0 only if both are), so it is either +0, where +0 + (+-0) = +0, or non-zero or NaN, where adding +-0 returns it;
//   - hence sum + x and sum + black() are the same bits, whatever `lit` would have been -- for a quad light too, whose `lit`
//     depends on the closest hit's material and equally does not matter.
// (A quad light seen from its back is NOT such a case: d_omega = dot(L.normal, omega) / r^2 is not clamped, the contribution is
// negative, not zero, and the sample is traced.)
// A NaN or an infinity anywhere in x fails one of the four comparisons (0 * inf would be NaN): that sample is traced as before.
// Booking the sample as "not lit" therefore equals tracing it; rays_shadow still counts it (the reference's count of samples).
__device__ __forceinline__ bool nee_irrelevant(const NeeSample& ns) {
  return ns.x.r == 0.0f && ns.x.g == 0.0f && ns.x.b == 0.0f && fabsf(ns.x.a) < INFINITY;
}
// the shadow-ray record of the wavefront engine (WfBuffers::sh_ray) carries the sample's kind and this mark in one word
constexpr uint32_t kShadowQuad = 1u, kShadowSkip = 2u;

// ---- shared by the wavefront engine's kernels (wavefront.inc) and their lane-refill forms (refill.hip) ------------------
struct WfBuffers {
  float4* hits;     // [item]: t, prim, u, v of the generation's rays (item = packed pixel for generation 0, queue slot after)
  float4* sh_ray;   // [2 * (j * npix + p)]: (origin.xyz, t_stop), (dir.xyz, quad flag) of the j-th shadow ray of pixel p
  float4* sh_x;     // [j * npix + p]: the contribution of that sample if the light is visible
  uint32_t nls;     // shadow rays per shaded pixel = lights x light_samples
};

// item -> packed pixel of generation 0: items walk the image in 8x8 tiles (one wave = one tile)
__device__ __forceinline__ bool tile_item_pixel(const FrameParams& fp, uint32_t item, uint32_t& x, uint32_t& r) {
  const uint32_t batch = item >> 6, j = item & 63u;
  if (batch >= fp.tile_count) return false;
  const uint32_t ty = batch / fp.tiles_x, tx = batch - ty * fp.tiles_x;
  x = tx * kTileW + (j & (kTileW - 1u));
  r = ty * kTileH + (j >> RAYCA_TILE_W_LOG2);
  return x < fp.width && r < fp.rows;
}

