// general.inc -- k_general: every IntegratorStrategy / SamplerStrategy combination that k_generation's
// generation scheme does not cover, as one per-pixel stack machine.  Included by kernels.hip.
//
// The reference's integrators are recursive (rayca-soft/src/integrator/*.rs); some branch (Scratcher:
// transmission + reflection; Pathtracer with light_samples > 1: one child per indirect sample) and one is
// unbounded (Russian roulette).  Here a lane owns one pixel and runs the recursion with an explicit stack of
// path-vertex frames kept in global memory (level-major, lane-minor: coalesced).  A frame holds only what
// cannot be recomputed -- the ray that produced the vertex, its hit record, the RNG key and counters, the
// running sums; everything HitInfo derives from the hit (normal, colours, BRDF inputs) is a pure function of
// (ray, hit) and is re-evaluated when a child returns, which yields the same bits.  There is still exactly
// ONE traversal call site: a handler either finishes the pixel, or leaves a pending ray and a phase.
// Evaluation order inside every vertex follows the reference statement by statement, because Color `+` is
// not commutative (rhs is alpha-weighted, color/mod.rs:239-286) and f32 sums are order dependent.

struct GFrameStore {
  float4* frames;    // [level][8][threads]
  float4* samples;   // MIS: [2 * kMisMaxSamples][threads]
  uint32_t threads;  // total threads of the launch
  uint32_t levels;   // frames allocated per lane
};
constexpr uint32_t kMisMaxSamples = 64;
constexpr unsigned long long kFlagUnsupported = 1ull;  // a todo!()/panic arm of the reference was reached
constexpr unsigned long long kFlagTooDeep = 2ull;      // recursion deeper than the frames allocated (roulette)

enum GPhase : uint32_t {
  GP_ENTER = 0,   // depth check, then trace the frame's ray
  GP_ENTER_HIT,   // result of that trace
  GP_BEGIN,       // hit shaded: start of the integrator's vertex program
  GP_PT_NEXT_DIRECT, GP_PT_SHADOW, GP_PT_BRDF_SHADOW, GP_PT_DIRECT_DONE, GP_PT_NEXT_INDIRECT, GP_PT_CHILD_RET,
  GP_W_NEXT_LIGHT, GP_W_SHADOW, GP_W_DONE,
  GP_RT_REFL_RET, GP_SC_TRANS_RET, GP_SC_REFL_RET,
  GP_DI_NEXT, GP_DI_SHADOW,
};

struct GFrame {
  F4 o, d;        // the ray that led to this vertex (Ray::new recomputes rdir)
  DHit hit;
  uint32_t key, dim, depth, li, k, phase, collect;
  Color a, b, thr;  // running sums (meaning per integrator), ray throughput (roulette)
  F4 omega;       // pending child's direction
  float weight;   // pending child's roulette boost
};

__device__ __forceinline__ void gframe_store(const GFrameStore& st, uint32_t level, uint32_t tid, const GFrame& f) {
  float4* p = st.frames + ((size_t)level * 8u) * st.threads + tid;
  const size_t s = st.threads;
  p[0 * s] = make_float4(f.o.x, f.o.y, f.o.z, f.hit.t);
  p[1 * s] = make_float4(f.d.x, f.d.y, f.d.z, __uint_as_float(f.hit.prim));
  p[2 * s] = make_float4(f.hit.u, f.hit.v, __uint_as_float(f.key), __uint_as_float(f.dim));
  p[3 * s] = make_float4(__uint_as_float(f.depth), __uint_as_float(f.li), __uint_as_float(f.k), __uint_as_float(f.phase | (f.collect << 8)));
  p[4 * s] = as_f4(f.a);
  p[5 * s] = as_f4(f.b);
  p[6 * s] = as_f4(f.thr);
  p[7 * s] = make_float4(f.omega.x, f.omega.y, f.omega.z, f.weight);
}
__device__ __forceinline__ void gframe_load(const GFrameStore& st, uint32_t level, uint32_t tid, GFrame& f) {
  const float4* p = st.frames + ((size_t)level * 8u) * st.threads + tid;
  const size_t s = st.threads;
  const float4 q0 = p[0 * s], q1 = p[1 * s], q2 = p[2 * s], q3 = p[3 * s], q7 = p[7 * s];
  f.o = point3(q0.x, q0.y, q0.z);
  f.d = vec3(q1.x, q1.y, q1.z);
  f.hit.t = q0.w;
  f.hit.prim = __float_as_uint(q1.w);
  f.hit.u = q2.x;
  f.hit.v = q2.y;
  f.key = __float_as_uint(q2.z);
  f.dim = __float_as_uint(q2.w);
  f.depth = __float_as_uint(q3.x);
  f.li = __float_as_uint(q3.y);
  f.k = __float_as_uint(q3.z);
  const uint32_t pc = __float_as_uint(q3.w);
  f.phase = pc & 0xFFu;
  f.collect = pc >> 8;
  f.a = as_color(p[4 * s]);
  f.b = as_color(p[5 * s]);
  f.thr = as_color(p[6 * s]);
  f.omega = vec3(q7.x, q7.y, q7.z);
  f.weight = q7.w;
}

// ---- what HitInfo offers beyond ShadeCtx (hit.rs:93-101,139-142,211-245) --------------------------------
struct GSurface {
  ShadeCtx s;
  Color color;     // get_color()
  F4 reflection;   // get_reflection(): normalized(reflect(ray.dir, normal))
  float metallic;  // pbr only
  float mat_t;     // Material::get_t  material/mod.rs:165-171 (phong.rs:67-74, ggx.rs:53-60)
  bool emissive;
  bool t_todo;     // get_t on a Pbr material is todo!()
};

template <bool SPH>
__device__ __forceinline__ void surface_of(const DevScene& sc, const DRay& ray, const DHit& hit, GSurface& g) {
  shade_hit<SPH>(sc, ray, hit, true, g.color, g.emissive, g.s);
  g.reflection = normalized(reflect(-g.s.view, g.s.normal));  // of hit.ray.dir, which for a sphere is the model-space direction
  const PrimExt& e = sc.ext[hit.prim];
  const DevMaterial m = (e.material != RAYCA_NONE && e.material < sc.material_count) ? sc.materials[e.material] : default_material();
  g.metallic = 0.0f;
  g.t_todo = m.kind == RAYCA_MATERIAL_PBR;
  g.mat_t = 0.0f;
  if (m.kind == RAYCA_MATERIAL_PBR) {
    // metallic = ks / base for the one place that needs it (ggx::get_radiance): re-derive as the reference does
    const bool is_sphere = SPH && e.kind == RAYCA_GEOMETRY_SPHERE;
    const float bu = hit.u, bv = hit.v, w2 = 1.0f - bu - bv;
    const F2 uv = is_sphere ? F2{0.0f, 0.0f}
                            : F2{(e.uv[2][0] * w2 + e.uv[0][0] * bu) + e.uv[1][0] * bv, (e.uv[2][1] * w2 + e.uv[0][1] * bu) + e.uv[1][1] * bv};
    float ro;
    pbr_metallic_roughness(sc, m, uv, g.metallic, ro);
  } else {
    const float kd_avg = hsum(vec3(m.diffuse[0], m.diffuse[1], m.diffuse[2])) / 3.0f;
    const float ks_avg = hsum(vec3(m.specular[0], m.specular[1], m.specular[2])) / 3.0f;
    if (ks_avg == 0.0f && kd_avg == 0.0f) g.mat_t = 1.0f;
    else {
      const float t = ks_avg / (ks_avg + kd_avg);
      g.mat_t = m.kind == RAYCA_MATERIAL_GGX ? fmaxf(t, 0.25f) : t;
    }
  }
}

// colour / emissive flag / emission of a hit whose full shading is not needed (shadow-ray hits)
template <bool SPH>
__device__ __forceinline__ void hit_color(const DevScene& sc, const DRay& ray, const DHit& hit, Color& color, bool& emissive, Color& emission) {
  ShadeCtx unused;
  shade_hit<SPH>(sc, ray, hit, false, color, emissive, unused);
  const PrimExt& e = sc.ext[hit.prim];
  emission = black();  // Material::get_emission: Phong only
  if (e.material != RAYCA_NONE && e.material < sc.material_count) {
    const DevMaterial& m = sc.materials[e.material];
    if (m.kind == RAYCA_MATERIAL_PHONG) emission = load_color(m.emission);
  }
}

// shared tail of cosine.rs:77-87, hemisphere.rs:29-39, ggx.rs:168-178, lambertian.rs:62-71
__device__ __forceinline__ F4 orient_sample(F4 sdir, F4 w, bool normalize_v) {
  const F4 a = close(w, vec3(0, 1, 0)) ? vec3(1, 0, 0) : vec3(0, 1, 0);
  const F4 u = normalized(cross(a, w));
  F4 v = cross(w, u);
  if (normalize_v) v = normalized(v);
  return (u * sdir.x + v * sdir.y) + w * sdir.z;
}
// (acosf / sinf / cosf of a sampled direction: the host C library's results, bit for bit -- libm_exact.hpp)
__device__ __forceinline__ F4 spherical(float theta, float omega) { return vec3(rc_cosf(omega) * rc_sinf(theta), rc_sinf(omega) * rc_sinf(theta), rc_cosf(theta)); }

// ggx.rs:131-146 / lambertian.rs:18-27
__device__ __forceinline__ float surf_pdf(const GSurface& g, F4 omega_i) {
  const ShadeCtx& s = g.s;
  if (s.kind == RAYCA_MATERIAL_PHONG) {
    const float r_dot_omega = clampf(dot(g.reflection, omega_i), 0.0f, 1.0f);
    const float sh = s.shininess;
    const float spec = (sh + 1.0f) * kFrac2Pi * powf(r_dot_omega, sh);
    const float diff = clampf(dot(s.normal, omega_i), 0.0f, 1.0f) * kFrac1Pi;
    return (1.0f - g.mat_t) * diff + g.mat_t * spec;
  }
  const F4 omega_o = s.view;
  const F4 h = normalized(omega_o + omega_i);
  const float h_dot_omega_i = clampf(dot(h, omega_i), 0.0f, 1.0f);
  if (h_dot_omega_i == 0.0f) return 0.0f;
  const float n_dot_h = clampf(dot(s.normal, h), 0.0f, 1.0f);
  const float spec = ggx_d(s.roughness, h, s.normal) * n_dot_h / (4.0f * h_dot_omega_i);
  const float dif = clampf(dot(s.normal, omega_i), 0.0f, 1.0f) * kFrac1Pi;
  return (1.0f - g.mat_t) * dif + g.mat_t * spec;
}
// ggx.rs:148-187 / lambertian.rs:32-72 (three draws)
__device__ __forceinline__ F4 surf_random_dir(const GSurface& g, uint32_t key, uint32_t& dim) {
  const ShadeCtx& s = g.s;
  const float e0 = rng_f32(key, dim++), e1 = rng_f32(key, dim++), e2 = rng_f32(key, dim++);
  const float t = g.mat_t;
  const float omega = 2.0f * kPi * e2;
  if (s.kind == RAYCA_MATERIAL_PHONG) {
    const float sh = s.shininess;
    const float theta = (e0 <= t) ? rc_acosf(clampf(powf(e1, 1.0f / (sh + 1.0f)), -1.0f, 1.0f)) : rc_acosf(clampf(sqrtf(e1), -1.0f, 1.0f));
    const F4 w = (e0 <= t) ? g.reflection : s.normal;
    return orient_sample(spherical(theta, omega), w, false);
  }
  const float a = s.roughness;
  const float theta = (e0 <= t) ? atanf((a * sqrtf(e1)) / sqrtf(1.0f - e1)) : rc_acosf(clampf(sqrtf(e1), -1.0f, 1.0f));
  const F4 sd = orient_sample(spherical(theta, omega), s.normal, false);
  if (e0 <= t) return reflect(-s.view, sd);
  return sd;
}
// ggx.rs:189-203 / lambertian.rs:74-80
__device__ __forceinline__ Color surf_specular_component(const GSurface& g, F4 omega_i) {
  const ShadeCtx& s = g.s;
  if (s.kind == RAYCA_MATERIAL_PHONG) {
    const float sh = s.shininess;
    const float n_dot_omega = clampf(dot(s.normal, omega_i), 0.0f, 1.0f);
    return ((s.ks * n_dot_omega) * (sh + 2.0f)) / (sh + 1.0f);
  }
  const F4 omega_o = s.view, n = s.normal;
  const float omega_o_dot_n = clampf(dot(omega_o, n), 0.0f, 1.0f);
  const F4 h = normalized(omega_i + omega_o);
  const float n_dot_h = clampf(dot(n, h), 0.0f, 1.0f);
  if (omega_o_dot_n == 0.0f || n_dot_h == 0.0f) return black();
  const float a = s.roughness;
  const float h_dot_omega_i = clampf(dot(h, omega_i), 0.0f, 1.0f);
  const float gg = ggx_g1(a, omega_i, n) * ggx_g1(a, omega_o, n);
  return ((ggx_f(s.ks, omega_i, h) * gg) * h_dot_omega_i) / (omega_o_dot_n * n_dot_h);
}

// Irradiance::new (hit.rs:263-287) + the Whitted get_radiance of both BRDF modules (ggx.rs:33-52, lambertian.rs:76-81)
__device__ __forceinline__ Color surf_radiance(const GSurface& g, Color intensity, F4 light_dir, bool& todo) {
  const ShadeCtx& s = g.s;
  const F4 l = light_dir, n = s.normal, v = s.view;
  const float n_dot_v = clampf(dot(n, v), 0.0f, 1.0f) + 1e-5f;
  const float n_dot_l = clampf(dot(n, l), 0.0f, 1.0f);
  const F4 h = normalized(v + l);
  const float n_dot_h = clampf(dot(n, h), 0.0f, 1.0f);
  const float l_dot_h = clampf(dot(l, h), 0.0f, 1.0f);
  if (s.kind == RAYCA_MATERIAL_PHONG) {
    const Color diffuse = s.kd * n_dot_l;
    const Color specular = s.ks * powf(n_dot_h, s.shininess);
    return (diffuse + specular) * intensity;
  }
  float metallic = 0.0f, roughness = 1.0f;
  if (s.kind == RAYCA_MATERIAL_PBR) {
    metallic = g.metallic;
    roughness = s.roughness;
  } else {
    todo = true;  // get_metallic_roughness on a Ggx material panics (material/mod.rs:54-62)
  }
  const float a = n_dot_h * roughness;
  const float kk = roughness / (1.0f - n_dot_h * n_dot_h + a * a);
  const float d = kk * kk * kFrac1Pi;
  const Color albedo = g.color;
  F4 f0 = f4(0.04f, 0.04f, 0.04f, 0.04f) * (1.0f - metallic) + premultiplied(albedo) * metallic;
  f0.w = 0.0f;
  const float fpow = powf(1.0f - l_dot_h, 5.0f);
  const F4 f = f0 + (vec3(1, 1, 1) - f0) * fpow;
  const F4 kd = (vec3(1, 1, 1) - f) * (1.0f - metallic);
  const float ggxv = n_dot_l * (n_dot_v * (1.0f - roughness) + roughness);
  const float ggxl = n_dot_v * (n_dot_l * (1.0f - roughness) + roughness);
  const float gsm = 0.5f / (ggxv + ggxl);
  const Color fr = (d * gsm) * Color{f.x, f.y, f.z, 1.0f};
  const Color fd = (Color{kd.x, kd.y, kd.z, 1.0f} * albedo) * kFrac1Pi;
  return ((fd + fr) * intensity) * n_dot_l;
}

// ---- lights (rayca-model/src/light/{mod,point,quad,directional}.rs) -------------------------------------
__device__ __forceinline__ F4 light_position(const DevLight& L) { return f4(L.position[0], L.position[1], L.position[2], L.position[3]); }
__device__ __forceinline__ float point_fallof(const DevLight& L, F4 frag_pos) {  // point.rs:41-49
  const F4 dist = to_vec(frag_pos) - to_vec(light_position(L));
  const float r2 = norm2(dist);
  const float r = sqrtf(r2);
  return hsum(f4(L.attenuation[0], L.attenuation[1], L.attenuation[2], 0.0f) * f4(1.0f, r, r2, 0.0f));
}
__device__ __forceinline__ F4 quad_corner(const DevLight& L, uint32_t which) {  // get_a: which = edge, get_b: edge + 1
  const F4 ab = vec3(L.ab[0], L.ab[1], L.ab[2]), ac = vec3(L.ac[0], L.ac[1], L.ac[2]);
  const F4 a = light_position(L);
  switch (which & 3u) {
    case 0: return a;
    case 1: return a + ab;
    case 2: return (a + ab) + ac;
    default: return a + ac;
  }
}
__device__ __forceinline__ Color light_intensity(const DevLight& L, F4 frag_pos, F4 frag_n) {  // light/mod.rs:53-59
  const Color lc = L.intensity * load_color(L.color);
  if (L.kind == RAYCA_LIGHT_DIRECTIONAL) return lc;
  if (L.kind == RAYCA_LIGHT_POINT) return lc / point_fallof(L, frag_pos);
  F4 ret = vec3(0, 0, 0);  // QuadLight::get_radiance  quad.rs:70-101
  for (uint32_t e = 0; e < 4; ++e) {
    const F4 ra = as_vec(quad_corner(L, e) - frag_pos), rb = as_vec(quad_corner(L, e + 1u) - frag_pos);
    const float theta = rc_acosf(dot(normalized(ra), normalized(rb)));
    const F4 gamma = normalized(cross(ra, rb));
    ret = ret + gamma * theta;
  }
  ret = ret / 2.0f;
  return lc * dot(ret, frag_n);
}
// Light::get_direction  light/mod.rs:83-89
__device__ __forceinline__ F4 light_direction(const DevLight& L, F4 frag_pos, bool& todo) {
  if (L.kind == RAYCA_LIGHT_DIRECTIONAL) return vec3(L.direction[0], L.direction[1], L.direction[2]);
  if (L.kind == RAYCA_LIGHT_POINT) return -normalized(to_vec(frag_pos) - to_vec(light_position(L)));
  todo = true;  // Quad: todo!()
  return vec3(0, 0, 0);
}
__device__ __forceinline__ float light_distance(const DevLight& L, F4 frag_pos, bool& todo) {  // light/mod.rs:45-51
  if (L.kind == RAYCA_LIGHT_QUAD) {
    todo = true;
    return 0.0f;
  }
  return length(to_vec(frag_pos - to_vec(light_position(L))));
}
// NextEventEstimationSample::get_pdf  nee.rs:44-66 with QuadLight::intersects  quad.rs:138-159
__device__ __forceinline__ float nee_pdf(const DevScene& sc, uint32_t light, const GSurface& g, F4 omega) {
  const DevLight L = sc.lights[light];
  if (L.kind != RAYCA_LIGHT_QUAD) return 0.0f;
  const DRay ray = make_ray(g.s.next_origin, omega);
  const F4 ab = vec3(L.ab[0], L.ab[1], L.ab[2]), ac = vec3(L.ac[0], L.ac[1], L.ac[2]);
  const float bias = 1e-2f;
  const Trs lt{f4(L.trs_translation[0], L.trs_translation[1], L.trs_translation[2], 0.0f),
               f4(L.trs_rotation[0], L.trs_rotation[1], L.trs_rotation[2], L.trs_rotation[3]),
               f4(L.trs_scale[0], L.trs_scale[1], L.trs_scale[2], 0.0f)};
  const F4 a = trs_apply_point(lt, to_point(-normalized(ab + ac) * bias));
  const F4 b = trs_apply_point(lt, to_point(ab + normalized(ab - ac) * bias));
  const F4 c = trs_apply_point(lt, to_point((ab + ac) + normalized(ab + ab) * bias));
  const F4 d = trs_apply_point(lt, to_point(ac + normalized(ac - ab) * bias));
  float t, u, v;
  bool got = tri_test(a, c, b, ray, t, u, v);
  if (!got) got = tri_test(a, d, c, ray, t, u, v);
  if (!got) return 0.0f;
  if (L.area == 0.0f) return 0.0f;
  const float nl_dot_omega = clampf(dot(vec3(L.normal[0], L.normal[1], L.normal[2]), omega), 0.0f, 1.0f);
  if (nl_dot_omega == 0.0f) return 0.0f;
  const F4 lp = ray.o + ray.d * t;
  const float r_squared = norm2(as_vec(lp - g.s.point));
  return r_squared / (L.area * nl_dot_omega);
}

// SoftSampler::get_radiance of the indirect sampler  cosine.rs:90-99, hemisphere.rs:42-52, brdf.rs:77-90
__device__ __forceinline__ Color indirect_radiance(const FrameParams& fp, const GSurface& g, F4 omega_i, Color sample, float weight) {
  if (fp.indirect_sampler == RAYCA_SAMPLER_COSINE) return ((kPi * surf_brdf(g.s, omega_i)) * sample) * weight;
  if (fp.indirect_sampler == RAYCA_SAMPLER_HEMISPHERE) {
    const Color brdf = surf_brdf(g.s, omega_i);
    const float cosine_law = clampf(dot(g.s.normal, omega_i), 0.0f, 1.0f);
    return ((((2.0f * kPi) * brdf) * cosine_law) * sample) * weight;
  }
  return (sample * (g.s.kd + surf_specular_component(g, omega_i))) * weight;  // Brdf
}

// One pixel per lane, persistent waves over 8x8 tiles like generation 0 of k_generation.
template <bool ORDERED, bool FAST, bool SPH, bool SPILL, bool STATS>
// Occupancy beats registers here: left to itself the compiler takes 264 VGPRs (one wave per SIMD).  Measured on the atrium at
// 1080p (tests/gpu_ab_general.py, one process): waves per SIMD 1 / 2 / 3 / 4 -> Pathtracer depth 3 on this engine 11.36 / 6.62 /
// 7.30 / 6.19 ms, Raytracer depth 2 8.23 / 5.12 / 5.62 / 5.18 ms, Pathtracer depth 3 with 4 light samples 223.8 / 126.4 / 139.7 /
// 104.8 ms -- the spills of the 128-register build cost less than the latency three more waves hide.
#ifndef RAYCA_GENERAL_MIN_WAVES
#define RAYCA_GENERAL_MIN_WAVES 4
#endif
__global__ __launch_bounds__(kBlock, RAYCA_GENERAL_MIN_WAVES) void k_general(DevScene sc, FrameParams fp, uint32_t* heads, PathBuffers pb, GFrameStore store,
                                                    TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  const uint32_t tid = rc_bid() * kBlock + rc_tid();
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, tid);
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  WorkCursor wc{};
  LaneCounters cnt{};
  uint32_t n_shaded = 0, n_shadow = 0, n_bounce = 0;
  unsigned long long flags = 0ull;
  const uint32_t integ = fp.integrator;
  const bool whitted = integ == RAYCA_INTEGRATOR_RAYTRACER || integ == RAYCA_INTEGRATOR_SCRATCHER;

  for (;;) {
    const uint32_t batch = next_batch(heads, fp.tile_count, home, wc, tl.ticket);
    if (batch == RAYCA_NONE) break;
    const uint32_t ty = batch / fp.tiles_x, tx = batch - ty * fp.tiles_x;
    const uint32_t x = tx * kTileW + (lane & (kTileW - 1u)), r = ty * kTileH + (lane >> RAYCA_TILE_W_LOG2);
    bool live = x < fp.width && r < fp.rows;
    const uint32_t y = ((r / fp.band) * fp.parts + fp.part) * fp.band + (r % fp.band);
    const uint32_t p = r * fp.width + x;

    GFrame f;
    uint32_t level = 0;
    f.hit.t = 0.0f; f.hit.prim = RAYCA_NONE; f.hit.u = f.hit.v = 0.0f;
    f.key = 0; f.dim = 0; f.depth = 0; f.li = 0; f.k = 0; f.phase = GP_ENTER; f.collect = 1;
    f.a = f.b = black();
    f.thr = white();
    f.omega = vec3(0, 0, 0);
    f.weight = 1.0f;
    f.o = point3(0, 0, 0);
    f.d = vec3(0, 0, 1);
    if (live) {
      const DRay cam = camera_ray(fp, x, y);
      f.o = cam.o;
      f.d = cam.d;
      f.key = rng_root(fp.seed, y * fp.width + x, fp.sample);
    }
    GSurface g;
    bool pending = false;       // a ray waits to be traced
    DRay tray = make_ray(f.o, f.d);
    float t_stop = FLT_MAX;
    NeeSample ns;               // the NEE / light sample the pending shadow ray decides
    ns.x = black(); ns.t_stop = FLT_MAX; ns.quad = 0u;
    bool ns_skipped = false;    // that sample cannot contribute: no shadow ray was traced for it
    F4 s_omega = vec3(0, 0, 0); // direction of the pending shadow ray where the handler needs it again
    float s_aux = 0.0f;
    Color ret = black();        // result of the child that just returned
    bool ret_some = false;
    uint32_t mis_n = 0;

    while (live) {
      DHit h;
      h.t = INFINITY; h.prim = RAYCA_NONE; h.u = h.v = 0.0f;
      bool found = false;
      if (pending) {
        found = trace<ORDERED, FAST, SPH, false, SPILL, STATS, false, ORDERED ? RAYCA_LEAVE_K_BOUNCE : 0>(sc, tray, t_stop, stack, h, cnt);
        pending = false;
      }
      bool again = true;
      bool need_surface = false;
      while (again && live) {
        again = false;
        if (need_surface) {
          surface_of<SPH>(sc, make_ray(f.o, f.d), f.hit, g);
          need_surface = false;
        }
        // do_return: hand `rv` to the parent (or to the pixel)
        bool returning = false, rv_some = false;
        Color rv = black();
        bool todo = false;
        switch (f.phase) {
          case GP_ENTER: {
            bool cut;  // pathtracer.rs:69-71, raytracer.rs:17-19, scratcher.rs:17-19, direct.rs:17-19, analyticdirect.rs:17-19
            if (integ == RAYCA_INTEGRATOR_PATHTRACER) cut = !fp.russian_roulette && f.depth >= fp.max_depth;
            else if (whitted) cut = f.depth > fp.max_depth;
            else cut = f.depth >= fp.max_depth;
            if (cut) { returning = true; break; }
            if (level > 0) n_bounce++;  // statistics: secondary rays that are actually traced
            tray = make_ray(f.o, f.d);
            t_stop = FLT_MAX;
            pending = true;
            f.phase = GP_ENTER_HIT;
          } break;
          case GP_ENTER_HIT: {
            if (!found) { returning = true; break; }
            f.hit = h;
            n_shaded++;
            need_surface = true;
            f.phase = GP_BEGIN;
            again = true;
          } break;
          case GP_BEGIN: {
            f.dim = 0; f.li = 0; f.k = 0;
            f.a = black(); f.b = black();
            if (integ == RAYCA_INTEGRATOR_PATHTRACER) {
              if (f.collect && g.emissive) { returning = true; rv_some = true; rv = g.color; break; }  // pathtracer.rs:83-87
              mis_n = 0;
              f.phase = GP_PT_NEXT_DIRECT;
              again = true;
            } else if (integ == RAYCA_INTEGRATOR_RAYTRACER) {
              f.phase = GP_W_NEXT_LIGHT;
              again = true;
            } else if (integ == RAYCA_INTEGRATOR_SCRATCHER) {
              if (is_transparent(g.color)) {  // scratcher.rs:31-43, get_transmit_ray_origin hit.rs:178-187
                GFrame c = f;
                f.phase = GP_SC_TRANS_RET;
                gframe_store(store, level, tid, f);
                if (level + 1u >= store.levels) { flags |= kFlagTooDeep; live = false; break; }
                ++level;
                f = c;
                f.o = g.s.point + (-g.s.normal) * kRayBias;
                f.o.w = 1.0f;
                f.d = -g.s.view;  // hit.ray.dir
                f.depth = c.depth + 1u;
                f.phase = GP_ENTER;
                again = true;
              } else {
                f.phase = GP_W_NEXT_LIGHT;
                again = true;
              }
            } else if (integ == RAYCA_INTEGRATOR_DIRECT) {
              if (g.emissive) { returning = true; rv_some = true; rv = g.color; break; }  // direct.rs:30-32
              f.phase = GP_DI_NEXT;
              again = true;
            } else {  // AnalyticDirect  analyticdirect.rs:16-48
              if (g.emissive) { returning = true; rv_some = true; rv = g.color; break; }
              Color lc = black();
              for (uint32_t li = 0; li < sc.light_count; ++li) lc = lc + light_intensity(sc.lights[li], g.s.point, g.s.normal);
              returning = true; rv_some = true;
              rv = (g.s.kd * kFrac1Pi) * lc;
            }
          } break;

          // ---- Pathtracer: direct lighting (sampler/{nee,mis,brdf}.rs), then the indirect loop -------------
          case GP_PT_NEXT_DIRECT: {
            const bool sample_lights = fp.direct_sampler == RAYCA_SAMPLER_NEE || fp.direct_sampler == RAYCA_SAMPLER_MIS;
            if (sample_lights && f.li < sc.light_count) {
              if (sc.lights[f.li].kind == RAYCA_LIGHT_DIRECTIONAL) {  // nee.rs:178 todo!()
                todo = true;
                if (++f.k == fp.light_samples) { f.k = 0; ++f.li; }
                again = true;
                break;
              }
              ns = nee_prepare(sc, fp, g.s, f.li, f.k, f.key, f.dim, tray);
              s_omega = tray.d;
              n_shadow++;
              f.phase = GP_PT_SHADOW;
              // A sample that cannot contribute (nee_irrelevant, trace_core.inc) goes straight to its handler as "not lit", without a
              // traversal.  MIS still records it, as black() = (0, 0, 0, 1) where the traced sample would be (+-0, +-0, +-0, a): both
              // enter the weighted sum as (w * +-0) * alpha, the same bits because a is finite (the rule) -- +-0 for a finite w, NaN
              // for a NaN one, whatever the alpha.
              ns_skipped = ORDERED && fp.nee_skip && nee_irrelevant(ns);
              if (ns_skipped) {
                again = true;
              } else {
                t_stop = ns.t_stop;
                pending = true;
              }
            } else if (fp.direct_sampler == RAYCA_SAMPLER_MIS) {  // BrdfSampler::sample_direct  brdf.rs:47-66
              s_omega = surf_random_dir(g, f.key, f.dim);
              if (g.t_todo) todo = true;
              tray = make_ray(g.s.next_origin, s_omega);
              t_stop = FLT_MAX;
              pending = true;
              n_shadow++;
              f.phase = GP_PT_BRDF_SHADOW;
            } else {
              f.phase = GP_PT_DIRECT_DONE;
              again = true;
            }
          } break;
          case GP_PT_SHADOW: {
            bool lit = false;
            if (ns_skipped) {
              // (no shadow ray was traced: `found` and `h` are not this sample's)
            } else if (ns.quad) {
              if (found) {
                const uint32_t hm = sc.ext[h.prim].material;
                lit = hm != RAYCA_NONE && hm < sc.material_count && sc.materials[hm].emissive != 0u;
              }
            } else {
              lit = !(found && h.t < ns.t_stop);
            }
            const Color x = lit ? ns.x : black();
            if (fp.direct_sampler == RAYCA_SAMPLER_MIS) {
              if (mis_n < kMisMaxSamples) {
                store.samples[(size_t)(2u * mis_n) * store.threads + tid] = make_float4(s_omega.x, s_omega.y, s_omega.z, __uint_as_float(f.li));
                store.samples[(size_t)(2u * mis_n + 1u) * store.threads + tid] = as_f4(x);
              } else {
                todo = true;  // more light samples per vertex than the sample store holds
              }
              ++mis_n;
            } else {
              f.a = f.a + x;  // nee.rs:209-216
            }
            if (++f.k == fp.light_samples) { f.k = 0; ++f.li; }
            f.phase = GP_PT_NEXT_DIRECT;
            again = true;
          } break;
          case GP_PT_BRDF_SHADOW: {  // mis.rs:40-72
            Color bx = black();
            if (found) {
              Color hc, em;
              bool emis;
              hit_color<SPH>(sc, tray, h, hc, emis, em);
              if (emis) bx = em * (g.s.kd + surf_specular_component(g, s_omega));
            }
            const float b_pdf = surf_pdf(g, s_omega);
            const uint32_t n = mis_n < kMisMaxSamples ? mis_n : kMisMaxSamples;
            Color acc = black();
            for (uint32_t i = 0; i < n; ++i) {
              const float4 so = store.samples[(size_t)(2u * i) * store.threads + tid];
              const Color sx = as_color(store.samples[(size_t)(2u * i + 1u) * store.threads + tid]);
              const F4 om = vec3(so.x, so.y, so.z);
              float pdf_nee = 0.0f;
              for (uint32_t j = 0; j < n; ++j) {
                const uint32_t lj = __float_as_uint(store.samples[(size_t)(2u * j) * store.threads + tid].w);
                pdf_nee += nee_pdf(sc, lj, g, om);
              }
              pdf_nee = pdf_nee / (float)n;
              const float pdf_brdf = surf_pdf(g, om);
              const float den = powf(pdf_nee, 2.0f) + powf(pdf_brdf, 2.0f);
              const float w = den == 0.0f ? 0.0f : powf(pdf_nee, 2.0f) / den;
              acc = acc + w * sx;
            }
            float pdf_nee = 0.0f;
            for (uint32_t j = 0; j < n; ++j) {
              const uint32_t lj = __float_as_uint(store.samples[(size_t)(2u * j) * store.threads + tid].w);
              pdf_nee += nee_pdf(sc, lj, g, s_omega);
            }
            pdf_nee = pdf_nee / (float)n;
            const float den = powf(pdf_nee, 2.0f) + powf(b_pdf, 2.0f);
            const float w = den == 0.0f ? 0.0f : powf(b_pdf, 2.0f) / den;
            acc = acc + w * bx;
            f.a = acc;
            f.phase = GP_PT_DIRECT_DONE;
            again = true;
          } break;
          case GP_PT_DIRECT_DONE: {
            f.k = 0;
            f.b = black();  // li
            f.phase = GP_PT_NEXT_INDIRECT;
            again = true;
          } break;
          case GP_PT_NEXT_INDIRECT: {  // get_indirect_lighting  pathtracer.rs:23-66
            const uint32_t limit = fp.direct_sampler != RAYCA_SAMPLER_NONE ? fp.max_depth - 1u : fp.max_depth;
            const bool enter = fp.russian_roulette || f.depth < limit;
            if (!enter) { returning = true; rv_some = true; rv = f.a + black(); break; }
            if (f.k >= fp.light_samples) {
              const Color indirect = black() + f.b / (float)fp.light_samples;
              returning = true; rv_some = true; rv = f.a + indirect;
              break;
            }
            F4 omega_i;
            if (fp.indirect_sampler == RAYCA_SAMPLER_HEMISPHERE) {
              const float e1 = rng_f32(f.key, f.dim++), e2 = rng_f32(f.key, f.dim++);
              omega_i = orient_sample(spherical(rc_acosf(e1), 2.0f * kPi * e2), g.s.normal, true);
            } else if (fp.indirect_sampler == RAYCA_SAMPLER_COSINE) {
              const float e1 = rng_f32(f.key, f.dim++), e2 = rng_f32(f.key, f.dim++);
              omega_i = orient_sample(spherical(rc_acosf(sqrtf(e1)), 2.0f * kPi * e2), g.s.normal, false);
            } else if (fp.indirect_sampler == RAYCA_SAMPLER_BRDF) {
              omega_i = surf_random_dir(g, f.key, f.dim);
              if (g.t_todo) todo = true;
            } else {
              todo = true;
              omega_i = vec3(0, 0, 1);
            }
            float weight = 1.0f;
            Color child_thr = white();
            if (fp.russian_roulette) {  // pathtracer.rs:40-52, Ray::next_russian_roulette ray.rs:95-105
              const Color brdf = surf_brdf(g.s, omega_i);
              const Color next_thr = (((2.0f * kPi) * f.thr) * brdf) * clampf(dot(g.s.normal, omega_i), 0.0f, 1.0f);
              const float q = 1.0f - fminf(fmaxf(fmaxf(next_thr.r, next_thr.g), next_thr.b), 1.0f);
              const float e = clampf(rng_f32(f.key, f.dim++), 0.0f, 1.0f - FLT_EPSILON);
              if (q < e) {
                weight = 1.0f / (1.0f - q);
                child_thr = next_thr * weight;
              } else {
                ++f.k;
                again = true;
                break;
              }
            }
            GFrame c = f;
            f.omega = omega_i;
            f.weight = weight;
            f.phase = GP_PT_CHILD_RET;
            gframe_store(store, level, tid, f);
            if (level + 1u >= store.levels) { flags |= kFlagTooDeep; live = false; break; }
            ++level;
            f = c;
            f.o = g.s.next_origin;
            f.d = omega_i;
            f.depth = c.depth + 1u;
            f.collect = fp.direct_sampler == RAYCA_SAMPLER_NONE ? 1u : 0u;
            f.key = rng_child(c.key, c.k);
            f.thr = child_thr;
            f.phase = GP_ENTER;
            again = true;
          } break;
          case GP_PT_CHILD_RET: {
            if (ret_some) f.b = f.b + indirect_radiance(fp, g, f.omega, ret, f.weight);
            ++f.k;
            f.phase = GP_PT_NEXT_INDIRECT;
            again = true;
          } break;

          // ---- Raytracer / Scratcher: the light loop (raytracer.rs:34-62, scratcher.rs:45-75) ---------------
          case GP_W_NEXT_LIGHT: {
            if (f.li < sc.light_count) {
              const F4 ldir = light_direction(sc.lights[f.li], g.s.point, todo);
              tray = make_ray(g.s.next_origin, ldir);
              t_stop = FLT_MAX;
              pending = true;
              n_shadow++;
              f.phase = GP_W_SHADOW;
            } else {
              f.phase = GP_W_DONE;
              again = true;
            }
          } break;
          case GP_W_SHADOW: {
            const DevLight L = sc.lights[f.li];
            bool is_light;
            if (!found) is_light = true;
            else {
              const float ldist = light_distance(L, g.s.point, todo);
              if (h.t > ldist) is_light = true;
              else {
                Color hc, em;
                bool emis;
                hit_color<SPH>(sc, tray, h, hc, emis, em);
                is_light = is_transparent(hc);
              }
            }
            if (is_light) {
              const Color intensity = light_intensity(L, g.s.point, g.s.normal);
              const F4 ldir = light_direction(L, g.s.point, todo);
              f.a = f.a + surf_radiance(g, intensity, ldir, todo);
            }
            ++f.li;
            f.phase = GP_W_NEXT_LIGHT;
            again = true;
          } break;
          case GP_W_DONE: {  // reflection child  raytracer.rs:64-73, scratcher.rs:77-86
            GFrame c = f;
            f.phase = integ == RAYCA_INTEGRATOR_RAYTRACER ? GP_RT_REFL_RET : GP_SC_REFL_RET;
            gframe_store(store, level, tid, f);
            if (level + 1u >= store.levels) { flags |= kFlagTooDeep; live = false; break; }
            ++level;
            f = c;
            f.o = g.s.next_origin;
            f.d = g.reflection;
            f.depth = c.depth + 1u;
            f.phase = GP_ENTER;
            again = true;
          } break;
          case GP_RT_REFL_RET: {
            if (ret_some) f.a = f.a + (ret * g.s.ks) * 1.0f;
            returning = true; rv_some = true;
            rv = g.color + f.a;
          } break;
          case GP_SC_TRANS_RET: {
            if (ret_some) {  // Color::over  color/mod.rs:149-154
              const Color top = g.color;
              const Color tr = Color{top.r * top.a + ret.r * (1.0f - top.a), top.g * top.a + ret.g * (1.0f - top.a),
                                     top.b * top.a + ret.b * (1.0f - top.a), 1.0f};
              f.a = f.a + tr;
            }
            f.li = 0;
            f.phase = GP_W_NEXT_LIGHT;
            again = true;
          } break;
          case GP_SC_REFL_RET: {
            if (ret_some) f.a = f.a + surf_radiance(g, ret, g.reflection, todo);
            returning = true; rv_some = true;
            rv = f.a;
          } break;

          // ---- Direct: quad lights sampled by area (direct.rs:34-82) ---------------------------------------
          case GP_DI_NEXT: {
            while (f.li < sc.light_count && sc.lights[f.li].kind != RAYCA_LIGHT_QUAD) ++f.li;
            if (f.li >= sc.light_count) { returning = true; rv_some = true; rv = f.a; break; }
            const DevLight L = sc.lights[f.li];
            const F4 ab = vec3(L.ab[0], L.ab[1], L.ab[2]), ac = vec3(L.ac[0], L.ac[1], L.ac[2]);
            const float sc_f = (float)fp.strate_count;
            const float u1 = rng_f32(f.key, f.dim++) / sc_f;
            const float u2 = rng_f32(f.key, f.dim++) / sc_f;
            F4 x1 = (light_position(L) + u1 * ab) + u2 * ac;
            if (fp.light_stratify) {
              const float i1 = (float)(f.k % fp.strate_count), i2 = (float)(f.k / fp.strate_count);
              x1 = x1 + ((ab / sc_f) * i1 + (ac / sc_f) * i2);
            }
            const F4 x1_to_hit = as_vec(x1 - g.s.point);
            s_omega = normalized(x1_to_hit);
            s_aux = length(x1_to_hit);
            tray = make_ray(g.s.next_origin, s_omega);
            t_stop = FLT_MAX;
            pending = true;
            n_shadow++;
            f.phase = GP_DI_SHADOW;
          } break;
          case GP_DI_SHADOW: {
            const DevLight L = sc.lights[f.li];
            bool skip = false;
            if (found) {
              const uint32_t hm = sc.ext[h.prim].material;
              const bool emis = hm != RAYCA_NONE && hm < sc.material_count && sc.materials[hm].emissive != 0u;
              skip = !emis;
            }
            if (!skip) {
              const Color brdf = surf_brdf(g.s, s_omega);
              const float r_squared = powf(s_aux, 2.0f);
              const float d_omega_i = dot(vec3(L.normal[0], L.normal[1], L.normal[2]), s_omega) / r_squared;
              f.b = f.b + (brdf * dot(g.s.normal, s_omega)) * d_omega_i;
            }
            if (++f.k == fp.light_samples) {
              const Color lcol = L.intensity * load_color(L.color);
              const Color ld = ((lcol * L.area) * f.b) / (float)fp.light_samples;
              f.a = f.a + ld;
              f.b = black();
              f.k = 0;
              ++f.li;
            }
            f.phase = GP_DI_NEXT;
            again = true;
          } break;
          default: live = false; break;
        }
        if (todo) flags |= kFlagUnsupported;
        if (returning) {
          if (level == 0) {
            pb.direct[p] = as_f4(rv);
            pb.state[p] = rv_some ? kVertexEmissive : kVertexNone;
            live = false;
          } else {
            ret = rv;
            ret_some = rv_some;
            --level;
            gframe_load(store, level, tid, f);
            need_surface = true;
            again = true;
          }
        }
      }
    }
  }
  if (STATS) {
    unsigned long long b = cnt.boxes, t = cnt.tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
    }
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
    }
  }
  unsigned long long sh = n_shaded, s2 = n_shadow, b2 = n_bounce;
  for (int off = 32; off > 0; off >>= 1) {
    sh += __shfl_down(sh, off);
    s2 += __shfl_down(s2, off);
    b2 += __shfl_down(b2, off);
  }
  if (lane == 0) {
    atomicAdd(&counters->shaded, sh);
    atomicAdd(&counters->shadow, s2);
    atomicAdd(&counters->bounce, b2);
  }
  if (flags) atomicOr(&counters->flags, flags);
}
