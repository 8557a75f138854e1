// direct.inc -- direct light at points (rayca_hip_direct_device): the NEE sum of a path vertex (sampler/nee.rs:72-166; nee_prepare
// in trace_core.inc) with the BRDF taken out, for points that are no path vertices.  N = light_count x light_samples shadow rays
// per point, made in registers from the point, its optional normal and the scene's light records, folded into one record per
// point.  Included by both traversal units behind ambient.inc: kernels.hip instantiates k_direct_rays and k_direct_fold,
// refill.hip calls direct_point / direct_sample / direct_lit from k_direct_refill.  Everything here is a template or an inline
// function, so a unit emits only what it names.
//
// The text of the header's comment on RaycaDirect, once: every operation in f32 and rounded on its own (the units are built with
// -ffp-contract=off), in nee_prepare's order and association, the Color operators included.  Both trace kernels and the fold
// call direct_sample, so the samples that are summed are the samples that were traced.
//
// Order-free results: a trace kernel only ORs bit j of the point's mask word (a 64-bit vector atomic, from lanes whose sample
// was traced and found lit); everything else is made from the finished word by k_direct_fold, in j order.

struct DirectPoint {
  F4 p, n;
  bool active;
};
// SPHERE: no normals -- the point is its own origin and the cosine term is absent.
template <bool SPHERE>
__device__ __forceinline__ DirectPoint direct_point(const DirectIo& a, uint32_t i) {
  DirectPoint pt;
  const float* p = a.points + 3ull * i;
  pt.p = point3(p[0], p[1], p[2]);
  pt.n = vec3(0.0f, 0.0f, 0.0f);
  pt.active = ambient_finite(pt.p.x) && ambient_finite(pt.p.y) && ambient_finite(pt.p.z);
  if (!SPHERE) {
    const float* n = a.normals + 3ull * i;
    pt.n = vec3(n[0], n[1], n[2]);
    const bool zero = pt.n.x == 0.0f && pt.n.y == 0.0f && pt.n.z == 0.0f;   // RaycaAmbient's inactive rule
    pt.active = pt.active && !zero && ambient_finite(pt.n.x) && ambient_finite(pt.n.y) && ambient_finite(pt.n.z);
  }
  return pt;
}

// Sample j of an active point: its shadow ray, what Color operator+ would add for it, and its class.
//   t_stop   point light: the light's distance, the any-hit bound; quad light: FLT_MAX, the closest hit is wanted (as NeeSample)
//   dropped  a component of y is not finite: neither traced nor added
//   empty    not dropped and y is all zeros (the header's "void"): not traced, its bit stays clear -- nee_irrelevant's argument
// A point-light sample that is traced has 0 < t_stop < FLT_MAX: a distance of 0 or NaN makes d_omega infinite or NaN and every
// product of it with le infinite or NaN, an infinite distance makes d_omega 0 -- dropped or empty either way.  Hence
// t_stop == FLT_MAX names the quad samples among the traced ones, as in k_generation.
struct DirectSample {
  F4 o, omega;
  float yr, yg, yb;
  float t_stop;
  bool dropped, empty;
};
template <bool SPHERE>
__device__ __forceinline__ DirectSample direct_sample(const DevLight* lights, const DirectIo& a, const DirectPoint& pt, uint32_t i, uint32_t j) {
  const uint32_t b = j / a.light_samples, k = j - b * a.light_samples;
  const DevLight& L = lights[a.light_first + b];
  const F4 x_point = pt.p;
  DirectSample s;
  Color x;
  if (L.kind == RAYCA_LIGHT_POINT) {  // get_point_light_sample  nee.rs:127-166
    const F4 x1 = f4(L.position[0], L.position[1], L.position[2], L.position[3]);
    const F4 x_to_x1 = as_vec(x1 - x_point);
    const float dist = length(x_to_x1);
    s.omega = normalized(x_to_x1);
    // PointLight::get_intensity / get_fallof  light/point.rs:37-49
    const F4 dvec = to_vec(x_point) - to_vec(x1);
    const float r2 = norm2(dvec);
    const float rr = sqrtf(r2);
    const float fallof = hsum(f4(L.attenuation[0], L.attenuation[1], L.attenuation[2], 0.0f) * f4(1.0f, rr, r2, 0.0f));
    const Color le = (L.intensity * load_color(L.color)) / fallof;
    const float r_squared = norm2(x_to_x1);
    const float d_omega = 1.0f / r_squared;
    if (SPHERE) {
      x = le * d_omega;
    } else {
      const float n_dot_omega = clampf(dot(pt.n, s.omega), 0.0f, 1.0f);
      x = (le * n_dot_omega) * d_omega;
    }
    s.t_stop = dist;
  } else {  // get_quad_light_sample  nee.rs:72-125 ; QuadLight::get_random_point  light/quad.rs:112-135
    // where a path vertex's `dim` stands when it reaches this sample: two dimensions for every quad-light sample in front of it
    const uint32_t q = a.quad_base + (uint32_t)__popcll(a.quad_bits & ((1ull << b) - 1ull));
    uint32_t dim = 2u * (q * a.light_samples + k);
    const uint32_t key = rng_root(a.seed, a.first_index + i, a.sample);
    const F4 ab = f4(L.ab[0], L.ab[1], L.ab[2], 0.0f), ac = f4(L.ac[0], L.ac[1], L.ac[2], 0.0f);
    const float sc_f = (float)a.strate_count;
    const float u1 = rng_f32(key, dim++) / sc_f;
    const float u2 = rng_f32(key, dim++) / sc_f;
    const F4 c = f4(L.position[0], L.position[1], L.position[2], L.position[3]);
    F4 x1 = (c + u1 * ab) + u2 * ac;
    if (a.light_stratify) {
      const float i1 = (float)(k % a.strate_count), i2 = (float)(k / a.strate_count);
      x1 = x1 + ((ab / sc_f) * i1 + (ac / sc_f) * i2);
    }
    const F4 x_to_x1 = as_vec(x1 - x_point);
    s.omega = normalized(x_to_x1);
    const Color le = L.intensity * load_color(L.color);
    const float r_squared = norm2(x_to_x1);
    const float d_omega = dot(f4(L.normal[0], L.normal[1], L.normal[2], 0.0f), s.omega) / r_squared;
    if (SPHERE) {
      x = (le * L.area) * d_omega;
    } else {
      const float n_dot_omega = clampf(dot(pt.n, s.omega), 0.0f, 1.0f);
      x = ((le * L.area) * n_dot_omega) * d_omega;
    }
    s.t_stop = FLT_MAX;
  }
  s.yr = x.r * x.a;
  s.yg = x.g * x.a;
  s.yb = x.b * x.a;
  s.dropped = !(ambient_finite(s.yr) && ambient_finite(s.yg) && ambient_finite(s.yb));
  s.empty = !s.dropped && s.yr == 0.0f && s.yg == 0.0f && s.yb == 0.0f;
  s.o = SPHERE ? pt.p : point3(pt.p.x + pt.n.x * a.bias, pt.p.y + pt.n.y * a.bias, pt.p.z + pt.n.z * a.bias);
  return s;
}

// The outcome of a traced sample's search.  Point light: lit iff nothing counts in front of the light -- query_found's strict
// t < tmax, what RAYCA_QUERY_OCCLUDED answers.  Quad light: lit iff the closest hit's material is emissive (nee.rs:103-104,
// k_shadow_refill's statement; bit 2 of a surface record's flags).
__device__ __forceinline__ bool direct_lit(const DevScene& sc, const DHit& hit, float t_stop) {
  if (t_stop == FLT_MAX) {
    if (hit.prim == RAYCA_NONE) return false;
    const uint32_t hm = sc.ext[hit.prim].material;
    return hm != RAYCA_NONE && hm < sc.material_count && sc.materials[hm].emissive != 0u;
  }
  return !query_found(hit, t_stop);
}

// k_ambient_rays' sibling: one sample per lane, item = i * N + j, on the binary f32 nodes with the spill path -- what serves a
// RAYCA_BUILDER_REFERENCE scene and a SAH scene whose formats thread has not finished.  A point-light sample is an any-hit search
// with t_stop = its distance, a quad-light sample an unbounded closest-hit search (k_query_rays' two forms).
template <bool SPHERE, bool FAST, bool SPH, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_TRACE_MIN_WAVES) void k_direct_rays(DevScene sc, DirectIo a, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<true> stack = make_stack<true>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t item = rc_bid() * rc_bdim() + rc_tid();
  LaneCounters cnt{};
  uint32_t traced = 0;
  if (item < a.count * a.samples) {   // (the host refuses count x samples >= 2^32)
    const uint32_t i = item / a.samples, j = item - i * a.samples;
    const DirectPoint pt = direct_point<SPHERE>(a, i);
    if (pt.active) {
      const DirectSample s = direct_sample<SPHERE>(sc.lights, a, pt, i, j);
      if (!s.dropped && !s.empty) {
        const DRay ray = make_ray(s.o, s.omega);
        DHit hit;
        hit.t = INFINITY;
        hit.prim = RAYCA_NONE;
        hit.u = hit.v = 0.0f;
        trace<true, FAST, SPH, false, true, STATS, false, 0, kSlackAlways>(sc, ray, s.t_stop, stack, hit, cnt);
        traced = 1u;
        if (direct_lit(sc, hit, s.t_stop)) atomicOr(&a.mask[i], 1ull << j);   // (i < count: nothing else is ever written)
      }
    }
  }
  if (a.count_traced) {   // (uniform)
    const unsigned long long m = __ballot(traced != 0u);
    if (m != 0ull && __lane_id() == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(&counters->shadow, (unsigned long long)__popcll(m));
  }
  if (STATS) {
    unsigned long long b = cnt.boxes, t = cnt.tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
    }
    if (__lane_id() == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
    }
  }
}

// The fold: one point per lane, behind the trace kernel on the same stream.  Reads the finished mask word, makes the point's
// samples again and sums the lit ones in j order; the SH9 projection only for sh_out.  An inactive point gives zeros.
constexpr uint32_t kDirectFoldBlock = 64;
template <bool SPHERE, bool SH>
__global__ __launch_bounds__(kDirectFoldBlock) void k_direct_fold(const DevLight* lights, DirectIo a) {
  const uint32_t i = rc_bid() * kDirectFoldBlock + rc_tid();
  if (i >= a.count) return;
  const DirectPoint pt = direct_point<SPHERE>(a, i);
  const unsigned long long m = pt.active ? a.mask[i] : 0ull;   // (an inactive point's word was cleared and never ORed into)
  float er = 0.0f, eg = 0.0f, eb = 0.0f;
  float hr[9], hg[9], hb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) hr[k] = hg[k] = hb[k] = 0.0f;
  uint32_t dropped = 0;
  if (pt.active) {
    for (uint32_t j = 0; j < a.samples; ++j) {
      const DirectSample s = direct_sample<SPHERE>(lights, a, pt, i, j);
      if (s.dropped) {
        ++dropped;
        continue;
      }
      if (!(m >> j & 1ull)) continue;
      er = er + s.yr;
      eg = eg + s.yg;
      eb = eb + s.yb;
      if (SH) {
        float y[9];
        sh9_basis(s.omega, y);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          hr[k] = hr[k] + s.yr * y[k];
          hg[k] = hg[k] + s.yg * y[k];
          hb[k] = hb[k] + s.yb * y[k];
        }
      }
    }
  }
  const uint32_t lit = (uint32_t)__popcll(m);
  if (a.irradiance_out) a.irradiance_out[i] = make_float4(er, eg, eb, (float)lit / (float)a.samples);
  if (SH) {
    float4* sh = a.sh_out + 9ull * i;
#pragma unroll
    for (int k = 0; k < 9; ++k) sh[k] = make_float4(hr[k], hg[k], hb[k], 0.0f);
  }
  if (a.mask_out && a.mask_out != a.mask) a.mask_out[i] = m;
  if (a.counts_out) a.counts_out[i] = lit | dropped << 16;
}
