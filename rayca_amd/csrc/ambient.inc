// ambient.inc -- hemisphere visibility at points (rayca_hip_ambient_device): S occlusion rays per point, made in registers from
// the point, its normal, an optional rotation and a table of local directions, folded into one record per point.  Included by
// both traversal units: kernels.hip instantiates k_ambient_rays and k_ambient_finish, refill.hip calls ambient_point / ambient_ray
// from k_ambient_refill.  Everything here is a template or an inline function, so a unit emits only what it names.
//
// The text of the header's comment on RaycaAmbient, once: +, -, x, /, comparisons and selects in f32, every operation rounded on
// its own (the units are built with -ffp-contract=off).  Both trace kernels and the fold call ambient_ray, so the d_j summed into
// `bent` are the d_j that were traced.
//
// Order-free results: a trace kernel only ORs bit j of the point's mask word (a 64-bit vector atomic, from lanes whose ray was
// occluded); hits, open and bent are made from the finished word by k_ambient_finish, bent by summing in j order.

// One point's inputs as the kernels carry them.  bound: the radius as the traversal carries a tmax (query_bound: FLT_MAX =
// unbounded); dead: nothing is traced for this point -- it is inactive, or its radius is NaN or <= 0.
struct AmbientPoint {
  F4 p, n;
  float c, s;
  float bound;
  bool active, dead;
};
__device__ __forceinline__ bool ambient_finite(float v) { return fabsf(v) <= FLT_MAX; }   // (a NaN fails the comparison)
template <bool ROT>
__device__ __forceinline__ AmbientPoint ambient_point(const AmbientIo& a, uint32_t i) {
  AmbientPoint pt;
  const float* p = a.points + 3ull * i;
  const float* n = a.normals + 3ull * i;
  pt.p = point3(p[0], p[1], p[2]);
  pt.n = vec3(n[0], n[1], n[2]);
  pt.c = 1.0f;
  pt.s = 0.0f;
  if (ROT) {
    pt.c = a.rotations[2ull * i];
    pt.s = a.rotations[2ull * i + 1ull];
  }
  const bool zero = pt.n.x == 0.0f && pt.n.y == 0.0f && pt.n.z == 0.0f;   // what rayca_hip_surface_device writes for a miss
  pt.active = !zero && ambient_finite(pt.p.x) && ambient_finite(pt.p.y) && ambient_finite(pt.p.z) && ambient_finite(pt.n.x) && ambient_finite(pt.n.y) &&
              ambient_finite(pt.n.z);
  const float tm = a.radius ? a.radius[i] : a.radius_all;
  pt.dead = !pt.active || !(tm > 0.0f);
  pt.bound = tm < FLT_MAX ? tm : FLT_MAX;
  return pt;
}

// Sample j of a point: origin and direction.  The branch-free basis of Duff et al. 2017, its sign taken by a comparison.
struct AmbientRay {
  F4 o, d;
};
template <bool ROT>
__device__ __forceinline__ AmbientRay ambient_ray(F4 p, F4 n, float c, float s, const float* dirs, uint32_t j, float bias) {
  const float sg = n.z >= 0.0f ? 1.0f : -1.0f;
  const float a = -1.0f / (sg + n.z);
  const float b = (n.x * n.y) * a;
  const float tx = 1.0f + ((sg * n.x) * n.x) * a, ty = sg * b, tz = (-sg) * n.x;
  const float bx = b, by = sg + (n.y * n.y) * a, bz = -n.y;
  const float lx = dirs[3u * j], ly = dirs[3u * j + 1u], lz = dirs[3u * j + 2u];
  float rx = lx, ry = ly;
  if (ROT) {
    rx = c * lx - s * ly;
    ry = s * lx + c * ly;
  }
  AmbientRay r;
  r.d = vec3(((tx * rx) + (bx * ry)) + n.x * lz, ((ty * rx) + (by * ry)) + n.y * lz, ((tz * rx) + (bz * ry)) + n.z * lz);
  r.o = point3(p.x + n.x * bias, p.y + n.y * bias, p.z + n.z * bias);
  return r;
}

// The nine real spherical harmonics of bands 0 .. 2 at a direction, exactly the expressions of the header's comment on RaycaGather:
// what the gather fold and the direct-light fold weigh a sample with.
__device__ __forceinline__ void sh9_basis(F4 d, float (&y)[9]) {
  y[0] = 0.2820948f;
  y[1] = 0.4886025f * d.y;
  y[2] = 0.4886025f * d.z;
  y[3] = 0.4886025f * d.x;
  y[4] = 1.0925484f * (d.x * d.y);
  y[5] = 1.0925484f * (d.y * d.z);
  y[6] = 0.3153916f * ((3.0f * (d.z * d.z)) - 1.0f);
  y[7] = 1.0925484f * (d.x * d.z);
  y[8] = 0.5462742f * ((d.x * d.x) - (d.y * d.y));
}

// k_query_rays<..., OCCLUDED>'s sibling: one ray per lane, item = i * S + j, on the binary f32 nodes with the spill path -- what
// serves a RAYCA_BUILDER_REFERENCE scene and a SAH scene whose formats thread has not finished.  Same t_stop convention (an
// unbounded ray gets the largest float below FLT_MAX, so that the early out is on for it too), same query_found.
template <bool FAST, bool SPH, bool STATS, bool ROT>
__global__ __launch_bounds__(kBlock, RAYCA_TRACE_MIN_WAVES) void k_ambient_rays(DevScene sc, AmbientIo a, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<true> stack = make_stack<true>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t item = rc_bid() * rc_bdim() + rc_tid();
  LaneCounters cnt{};
  if (item < a.count * a.samples) {   // (the host refuses count x samples >= 2^32)
    const uint32_t i = item / a.samples, j = item - i * a.samples;
    const AmbientPoint pt = ambient_point<ROT>(a, i);
    if (!pt.dead) {
      const AmbientRay ar = ambient_ray<ROT>(pt.p, pt.n, pt.c, pt.s, a.dirs, j, a.bias);
      const DRay ray = make_ray(ar.o, ar.d);
      DHit hit;
      hit.t = INFINITY;
      hit.prim = RAYCA_NONE;
      hit.u = hit.v = 0.0f;
      const float t_stop = pt.bound < FLT_MAX ? pt.bound : __uint_as_float(0x7F7FFFFEu);
      trace<true, FAST, SPH, false, true, STATS, false, 0, kSlackAlways>(sc, ray, t_stop, stack, hit, cnt);
      if (query_found(hit, pt.bound)) atomicOr(&a.mask[i], 1ull << j);   // (i < count: nothing else is ever written)
    }
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

// The fold: one point per lane, behind the trace kernel on the same stream.  Reads the finished mask word and writes the outputs
// that are asked for; the direction loop runs only for bent_out.  An inactive point traced nothing: mask 0, hits 0, open 1, bent 0.
template <bool BENT, bool ROT>
__global__ __launch_bounds__(kBlock) void k_ambient_finish(AmbientIo a) {
  const uint32_t i = rc_bid() * rc_bdim() + rc_tid();
  if (i >= a.count) return;
  const unsigned long long m = a.mask[i];
  const uint32_t hits = (uint32_t)__popcll(m);
  if (a.mask_out && a.mask_out != a.mask) a.mask_out[i] = m;
  if (a.hits_out) a.hits_out[i] = hits;
  if (a.open_out) a.open_out[i] = (float)(a.samples - hits) / (float)a.samples;
  if (BENT) {
    const AmbientPoint pt = ambient_point<ROT>(a, i);
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (pt.active) {
      for (uint32_t j = 0; j < a.samples; ++j) {
        const AmbientRay ar = ambient_ray<ROT>(pt.p, pt.n, pt.c, pt.s, a.dirs, j, a.bias);
        if (!(m >> j & 1ull)) {
          x = x + ar.d.x;
          y = y + ar.d.y;
          z = z + ar.d.z;
        }
      }
    }
    a.bent_out[3ull * i] = x;
    a.bent_out[3ull * i + 1ull] = y;
    a.bent_out[3ull * i + 2ull] = z;
  }
}
