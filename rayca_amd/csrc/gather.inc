// gather.inc -- irradiance at points (rayca_hip_gather_device): ambient.inc's rays, made in registers and written straight into the
// frame driver's generation-0 queue, and the fold of the radiance that comes back into irradiance and nine spherical-harmonic
// coefficients per point.  Included by kernels.hip behind ambient.inc, whose ambient_point / ambient_ray both kernels call: the
// d_j the fold weighs a sample with is the d_j that was traced.
//
// The text of the header's comment on RaycaGather, once: every operation in f32 and rounded on its own (the unit is built with
// -ffp-contract=off), the samples of a point folded in j order by one lane.  One launch of each kernel per internal frame of
// whole points; GatherIo is that frame's view of the call's arrays.

// k_enqueue_rays (wavefront.inc) without the 24-B ray array: one thread per (i, j) of the frame, entry = "pixel" = i * S + j, the
// key of pixel index first_index + entry.  The queue is dense: the slots of an inactive point hold the ray o = d = (0, 0, 0), which
// hits nothing (a zero direction component has reciprocal 0, so every plane distance is 0 and slab's tmax > 0 fails for every
// box); the fold discards what the miss is shaded to.  The queue's count is written by the launch's first thread, behind whatever
// cleared the counters in stream order.
template <bool ROT>
__global__ __launch_bounds__(kBlock) void k_enqueue_gather(GatherIo g, uint32_t seed, uint32_t sample, QueuedRay* __restrict__ out_rays, uint32_t* out_count) {
  const uint32_t item = rc_bid() * kBlock + rc_tid();
  const uint32_t total = g.a.count * g.a.samples;   // (the host keeps a frame at kGatherFrameRays or one point: no wrap)
  if (item == 0u) *out_count = total;
  if (item >= total) return;
  const uint32_t i = item / g.a.samples, j = item - i * g.a.samples;
  const AmbientPoint pt = ambient_point<ROT>(g.a, i);
  QueuedRay q;
  q.ox = q.oy = q.oz = 0.0f;
  q.dx = q.dy = q.dz = 0.0f;
  if (pt.active) {
    const AmbientRay ar = ambient_ray<ROT>(pt.p, pt.n, pt.c, pt.s, g.a.dirs, j, g.a.bias);
    q.ox = ar.o.x; q.oy = ar.o.y; q.oz = ar.o.z;
    q.dx = ar.d.x; q.dy = ar.d.y; q.dz = ar.d.z;
  }
  q.pixel = item;
  q.key = rng_root(seed, g.first_index + item, sample);
  out_rays[item] = q;
}

// The fold: one point per lane, behind the frame's last kernel on the same stream.  A lane walks its own S records, 16 bytes a
// load, 16 S bytes from its neighbour's (1 KiB at S = 64): not a coalesced access.  The eight records of a 128-B line are read by
// one lane in eight consecutive iterations, so the expectation is that a line comes from memory once and from the cache after
// that -- an expectation: the fold has not been timed on its own (DESIGN 4.19).  Directions are made again only for sh_out.
constexpr uint32_t kGatherFoldBlock = 64;
__device__ __forceinline__ bool gather_counts(float4 c) { return (c.x - c.x == 0.0f) && (c.y - c.y == 0.0f) && (c.z - c.z == 0.0f); }   // image_pass.inc finite4 on r, g, b
template <bool SH, bool WEIGHTS, bool ROT>
__global__ __launch_bounds__(kGatherFoldBlock) void k_gather_fold(GatherIo g) {
  const uint32_t i = rc_bid() * kGatherFoldBlock + rc_tid();
  if (i >= g.a.count) return;
  const uint32_t samples = g.a.samples;
  const AmbientPoint pt = ambient_point<ROT>(g.a, i);
  const float4* records = g.samples + (size_t)i * samples;
  float er = 0.0f, eg = 0.0f, eb = 0.0f;
  float hr[9], hg[9], hb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) hr[k] = hg[k] = hb[k] = 0.0f;
  uint32_t kept = 0;
  if (pt.active) {
    for (uint32_t j = 0; j < samples; ++j) {
      const float4 l = records[j];
      if (!gather_counts(l)) continue;
      float cr = l.x, cg = l.y, cb = l.z;
      if (WEIGHTS) {
        const float w = g.weights[j];
        cr = w * cr;
        cg = w * cg;
        cb = w * cb;
      }
      er = er + cr;
      eg = eg + cg;
      eb = eb + cb;
      if (SH) {
        const F4 d = ambient_ray<ROT>(pt.p, pt.n, pt.c, pt.s, g.a.dirs, j, g.a.bias).d;
        float y[9];
        sh9_basis(d, y);   // (ambient.inc: the header's nine expressions)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          hr[k] = hr[k] + cr * y[k];
          hg[k] = hg[k] + cg * y[k];
          hb[k] = hb[k] + cb * y[k];
        }
      }
      ++kept;
    }
  } else if (g.samples_out) {
    float4* rows = g.samples_out + (size_t)i * samples;
    for (uint32_t j = 0; j < samples; ++j) rows[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  if (kept > 0) {
    const float n = (float)kept;
    er = er / n;
    eg = eg / n;
    eb = eb / n;
    if (SH) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        hr[k] = hr[k] / n;
        hg[k] = hg[k] / n;
        hb[k] = hb[k] / n;
      }
    }
  }
  if (g.irradiance_out) g.irradiance_out[i] = make_float4(er, eg, eb, (float)kept / (float)samples);
  if (SH) {
    float4* sh = g.sh_out + 9ull * i;
#pragma unroll
    for (int k = 0; k < 9; ++k) sh[k] = make_float4(hr[k], hg[k], hb[k], 0.0f);
  }
  if (g.kept_out) g.kept_out[i] = kept;
}
