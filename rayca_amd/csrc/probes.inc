// probes.inc -- irradiance volumes (rayca_hip_probe_lookup_device): the diffuse light at points from a regular grid of SH9 probes,
// the eight probes of a point's cell blended by trilinear weight, a wrapped normal term and, when asked for, one short occlusion
// ray per corner.  Included by both traversal units behind ambient.inc: kernels.hip instantiates k_probe_rays and k_probe_fold,
// refill.hip calls probe_point / probe_cell / probe_corner / probe_ray from k_probe_refill.  Everything here is a template or an
// inline function, so a unit emits only what it names.
//
// The text of the header's comment on RaycaProbeLookup, once: +, -, x, /, floor, min, max, |x|, comparisons, selects and integers,
// in f32, every operation rounded on its own (the units are built with -ffp-contract=off).  Both trace kernels and the fold call
// the same four functions, so the rays that are traced are the rays the fold assumes.
//
// Order-free results: a trace kernel only ORs bit 8 + k of the point's mask word (a 32-bit vector atomic, from lanes whose ray was
// occluded); k_probe_fold makes everything else from the finished word, in k order.

struct ProbePoint {
  F4 p, n;
  bool active;
};
__device__ __forceinline__ ProbePoint probe_point(const ProbeIo& a, uint32_t i) {
  ProbePoint pt;
  const float* p = a.points + 3ull * i;
  const float* n = a.normals + 3ull * i;
  pt.p = point3(p[0], p[1], p[2]);
  pt.n = vec3(n[0], n[1], n[2]);
  const bool zero = pt.n.x == 0.0f && pt.n.y == 0.0f && pt.n.z == 0.0f;   // RaycaAmbient's inactive rule
  pt.active = !zero && ambient_finite(pt.p.x) && ambient_finite(pt.p.y) && ambient_finite(pt.p.z) && ambient_finite(pt.n.x) && ambient_finite(pt.n.y) &&
              ambient_finite(pt.n.z);
  return pt;
}

// The cell of a point, per axis: the two probe indices and the weight of the upper one.  A point outside the grid takes the
// nearest boundary cell (fmaxf / fminf are maxNum / minNum; an active point's f is never NaN: p, g and h are finite, h > 0).
struct ProbeCell {
  uint32_t i0[3], i1[3];
  float t[3];
};
__device__ __forceinline__ void probe_axis(float p, float g, float h, uint32_t dim, uint32_t& i0, uint32_t& i1, float& t) {
  float f = (p - g) / h;
  f = fminf(fmaxf(f, 0.0f), (float)(dim - 1u));
  i0 = min((uint32_t)floorf(f), dim >= 2u ? dim - 2u : 0u);
  t = f - (float)i0;
  i1 = min(i0 + 1u, dim - 1u);
}
__device__ __forceinline__ ProbeCell probe_cell(const ProbeIo& a, F4 p) {
  ProbeCell c;
  probe_axis(p.x, a.origin[0], a.cell[0], a.dims[0], c.i0[0], c.i1[0], c.t[0]);
  probe_axis(p.y, a.origin[1], a.cell[1], a.dims[1], c.i0[1], c.i1[1], c.t[1]);
  probe_axis(p.z, a.origin[2], a.cell[2], a.dims[2], c.i0[2], c.i1[2], c.t[2]);
  return c;
}

// Corner k of a cell: the probe's index, its centre, its trilinear weight, and whether it is a candidate (wt > 0 and valid).
struct ProbeCorner {
  uint32_t m;
  F4 c;
  float wt;
  bool candidate;
};
__device__ __forceinline__ ProbeCorner probe_corner(const ProbeIo& a, const ProbeCell& cell, uint32_t k, bool kept) {
  const bool bx = (k & 1u) != 0u, by = (k >> 1 & 1u) != 0u, bz = (k >> 2 & 1u) != 0u;
  const uint32_t ix = bx ? cell.i1[0] : cell.i0[0], iy = by ? cell.i1[1] : cell.i0[1], iz = bz ? cell.i1[2] : cell.i0[2];
  const float wx = bx ? cell.t[0] : 1.0f - cell.t[0], wy = by ? cell.t[1] : 1.0f - cell.t[1], wz = bz ? cell.t[2] : 1.0f - cell.t[2];
  ProbeCorner pc;
  pc.m = (iz * a.dims[1] + iy) * a.dims[0] + ix;   // (below the dims' product, which the host keeps at 2^24)
  pc.c = point3(a.origin[0] + (float)ix * a.cell[0], a.origin[1] + (float)iy * a.cell[1], a.origin[2] + (float)iz * a.cell[2]);
  pc.wt = (wx * wy) * wz;
  pc.candidate = pc.wt > 0.0f;
  if (kept) pc.candidate = pc.candidate && a.kept[pc.m] != 0u;   // (kept: the call has a kept array; read for corners with a weight alone)
  return pc;
}

// The occlusion ray of a corner: from the lifted point to the probe's centre, tmax = 1.
__device__ __forceinline__ AmbientRay probe_ray(const ProbePoint& pt, F4 c, float bias) {
  AmbientRay r;
  r.o = point3(pt.p.x + pt.n.x * bias, pt.p.y + pt.n.y * bias, pt.p.z + pt.n.z * bias);
  r.d = vec3(c.x - r.o.x, c.y - r.o.y, c.z - r.o.z);
  return r;
}

// The normal term: a signed squared cosine of the angle between the normal and the way to the probe, wrapped so that a probe
// behind the surface keeps a sixteenth.  No square root: s |s| / l2 is cos |cos| for a unit normal.
__device__ __forceinline__ float probe_normal_weight(const ProbePoint& pt, F4 c) {
  const float vx = c.x - pt.p.x, vy = c.y - pt.p.y, vz = c.z - pt.p.z;
  const float s = (vx * pt.n.x + vy * pt.n.y) + vz * pt.n.z;
  const float l2 = (vx * vx + vy * vy) + vz * vz;
  const float q = l2 > 0.0f ? (s * fabsf(s)) / l2 : 1.0f;
  float wb = (q + 1.0f) * 0.5f;
  wb = wb * wb + 0.0625f;
  return wb;
}

// k_ambient_rays' sibling: one ray per lane, item = i * 8 + k, on the binary f32 nodes with the spill path -- what serves a
// RAYCA_BUILDER_REFERENCE scene and a SAH scene whose formats thread has not finished.  A candidate corner's ray is traced with
// t_stop = 1; a lane whose ray was occluded ORs bit 8 + k into the point's word.
template <bool FAST, bool SPH, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_TRACE_MIN_WAVES) void k_probe_rays(DevScene sc, ProbeIo a, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<true> stack = make_stack<true>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t item = rc_bid() * rc_bdim() + rc_tid();
  LaneCounters cnt{};
  if (item < a.count * 8u) {   // (the host refuses count x 8 >= 2^32)
    const uint32_t i = item >> 3, k = item & 7u;
    const ProbePoint pt = probe_point(a, i);
    if (pt.active) {
      const ProbeCorner pc = probe_corner(a, probe_cell(a, pt.p), k, a.kept != nullptr);
      if (pc.candidate) {
        const AmbientRay pr = probe_ray(pt, pc.c, a.bias);
        const DRay ray = make_ray(pr.o, pr.d);
        DHit hit;
        hit.t = INFINITY;
        hit.prim = RAYCA_NONE;
        hit.u = hit.v = 0.0f;
        trace<true, FAST, SPH, false, true, STATS, false, 0, kSlackAlways>(sc, ray, 1.0f, stack, hit, cnt);
        if (query_found(hit, 1.0f)) atomicOr(&a.mask[i], 1u << (8u + k));   // (i < count: nothing else is ever written)
      }
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

// One pass of the blend over the corners in `take`, k ascending: wsum and H from zero.
struct ProbeBlend {
  float wsum;
  float r[9], g[9], b[9];
};
template <bool NORMAL>
__device__ __forceinline__ void probe_blend(const ProbeIo& a, const ProbePoint& pt, const ProbeCell& cell, uint32_t take, ProbeBlend& h) {
  h.wsum = 0.0f;
#pragma unroll
  for (int j = 0; j < 9; ++j) h.r[j] = h.g[j] = h.b[j] = 0.0f;
  for (uint32_t k = 0; k < 8u; ++k) {
    if (!(take >> k & 1u)) continue;
    const ProbeCorner pc = probe_corner(a, cell, k, false);   // (`take` holds candidates only: kept has been read)
    float w = pc.wt;
    if (NORMAL) w = w * probe_normal_weight(pt, pc.c);
    if (!(w > 0.0f)) continue;   // (a NaN weight fails the comparison)
    const float4* rec = a.sh + 9ull * pc.m;
    h.wsum = h.wsum + w;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const float4 s = rec[j];
      h.r[j] = h.r[j] + w * s.x;
      h.g[j] = h.g[j] + w * s.y;
      h.b[j] = h.b[j] + w * s.z;
    }
  }
}

// The fold: one point per lane, behind the trace kernel on the same stream (or alone, without RAYCA_PROBE_VISIBILITY).  Reads the
// finished mask word, blends the counting corners' records (aligned 16-byte loads), evaluates the irradiance at the normal and
// writes the outputs that are asked for.  An inactive point gives zeros; its radiance_out is base's pixel, or (0, 0, 0, 1).
constexpr uint32_t kProbeFoldBlock = 64;
template <bool VIS, bool NORMAL, bool KEPT>
__global__ __launch_bounds__(kProbeFoldBlock) void k_probe_fold(ProbeIo a) {
  const uint32_t i = rc_bid() * kProbeFoldBlock + rc_tid();
  if (i >= a.count) return;
  const ProbePoint pt = probe_point(a, i);
  ProbeBlend h;
  h.wsum = 0.0f;
#pragma unroll
  for (int j = 0; j < 9; ++j) h.r[j] = h.g[j] = h.b[j] = 0.0f;
  float er = 0.0f, eg = 0.0f, eb = 0.0f;
  uint32_t word = 0u;
  if (pt.active) {
    const ProbeCell cell = probe_cell(a, pt.p);
    uint32_t cand = 0u;
    for (uint32_t k = 0; k < 8u; ++k)
      if (probe_corner(a, cell, k, KEPT).candidate) cand |= 1u << k;
    const uint32_t occ = VIS ? (a.mask[i] >> 8 & 0xFFu) : 0u;   // (a subset of cand: only candidates were traced)
    word = cand | occ << 8;
    probe_blend<NORMAL>(a, pt, cell, cand & ~occ, h);
    if ((VIS || NORMAL) && !(h.wsum > 0.0f)) {   // the fallback: the trilinear weights alone, over every candidate
      probe_blend<false>(a, pt, cell, cand, h);
      word |= 1u << 16;
    }
    if (h.wsum > 0.0f) {
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        h.r[j] = h.r[j] / h.wsum;
        h.g[j] = h.g[j] / h.wsum;
        h.b[j] = h.b[j] / h.wsum;
      }
    } else {
      h.wsum = 0.0f;
#pragma unroll
      for (int j = 0; j < 9; ++j) h.r[j] = h.g[j] = h.b[j] = 0.0f;
    }
    const F4 n = pt.n;
    float bj[9];
    bj[0] = 3.1415927f * 0.2820948f;
    bj[1] = 2.0943952f * (0.4886025f * n.y);
    bj[2] = 2.0943952f * (0.4886025f * n.z);
    bj[3] = 2.0943952f * (0.4886025f * n.x);
    bj[4] = 0.7853982f * (1.0925484f * (n.x * n.y));
    bj[5] = 0.7853982f * (1.0925484f * (n.y * n.z));
    bj[6] = 0.7853982f * (0.3153916f * ((3.0f * (n.z * n.z)) - 1.0f));
    bj[7] = 0.7853982f * (1.0925484f * (n.x * n.z));
    bj[8] = 0.7853982f * (0.5462742f * ((n.x * n.x) - (n.y * n.y)));
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      er = er + bj[j] * h.r[j];
      eg = eg + bj[j] * h.g[j];
      eb = eb + bj[j] * h.b[j];
    }
    er = fmaxf(er, 0.0f);
    eg = fmaxf(eg, 0.0f);
    eb = fmaxf(eb, 0.0f);
  }
  if (a.irradiance_out) a.irradiance_out[i] = make_float4(er, eg, eb, h.wsum);
  if (a.sh_out) {
    float4* sh = a.sh_out + 9ull * i;
#pragma unroll
    for (int j = 0; j < 9; ++j) sh[j] = make_float4(h.r[j], h.g[j], h.b[j], 0.0f);
  }
  if (a.mask_out) a.mask_out[i] = word;
  if (a.radiance_out) {
    float4 l = a.base ? a.base[i] : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if (pt.active) {
      const float4 al = a.albedo[i];
      const float lr = al.x * (er * 0.31830987f), lg = al.y * (eg * 0.31830987f), lb = al.z * (eb * 0.31830987f);
      if (a.base) {
        l.x = lr + l.x;
        l.y = lg + l.y;
        l.z = lb + l.z;
      } else {
        l.x = lr;
        l.y = lg;
        l.z = lb;
      }
    }
    a.radiance_out[i] = l;
  }
}
