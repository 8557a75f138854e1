// wavefront.inc -- the same frames as k_generation, split so that traversal runs in LEAN kernels.
// Included by kernels.hip.
//
// Why: PMC on k_generation shows a latency-bound kernel (57 % of wave-cycles in s_waitcnt, VALU 51 % busy,
// ~400 cycles per wave load) that can keep only 4-5 waves per SIMD resident because the shading state of
// the fused state machine lives in registers across the traversal.  Here a generation is three launches:
//   k_wf_trace   closest hit of every ray of the generation           (one thread per ray)
//   k_wf_shade   HitInfo, NEE sample set-up, bounce sampling           (streaming, one thread per ray)
//   k_wf_shadow  the pixel's shadow rays in order, direct lighting sum  (one thread per pixel)
// and the traversal kernels carry nothing but the ray, the best hit and the stack pointer (6 waves per SIMD).
//
// A persistent variant with lane-level refill (finished lanes take new rays while the others keep their
// traversal state) was built and measured twice.  First with the ray set-up inline: 114 VGPRs, 0.42 ms for the
// atrium's camera rays against 0.27 ms for the plain one-thread-per-ray kernel at 76 VGPRs.  Then around
// node_step() with a lean per-lane state (101 VGPRs camera rays, 82 queued rays): atrium camera rays 0.36 -> 0.60 ms,
// Cornell 0.09 -> 0.17 ms, and on the 1 M-triangle soup, whose node loop runs at 17 % lane utilisation
// (tests/gpu_util_probe.py), 5.8 -> 4.1 ms -- only 7 % under the fused kernel's 4.5 ms.  The idle lanes were not the
// cost: these kernels wait on dependent fetches, and occupancy buys more fetches in flight than full waves do.
// The plain form ships.
// Workgroups are dealt to XCDs round-robin by the hardware; the block index is remapped so that each XCD
// walks one contiguous eighth of the tile list (neighbouring tiles -> the same L2).
//
// Arithmetic is shared with k_generation (camera_ray, trace(), shade_hit, nee_prepare, the bounce block);
// results are bit-identical (tests/test_gpu_engines.py).

// (node formats of these kernels: RAYCA_WF_* in trace_core.inc, shared with refill.hip)
#ifndef RAYCA_LEAVE_K_WF_CAMERA
#define RAYCA_LEAVE_K_WF_CAMERA RAYCA_LEAVE_K_CAMERA   // early leave of the node phase (trace(), trace_core.inc)
#endif
#ifndef RAYCA_LEAVE_K_WF_SHADOW
#define RAYCA_LEAVE_K_WF_SHADOW RAYCA_LEAVE_K_BOUNCE
#endif
#ifndef RAYCA_WF_MIN_WAVES
#define RAYCA_WF_MIN_WAVES 1
#endif

// blockIdx -> logical block such that XCD k (which receives blocks k, k+8, k+16, ...) works on one contiguous
// eighth of the list
__device__ __forceinline__ uint32_t xcd_contiguous_block(uint32_t b, uint32_t nblocks) {
  const uint32_t per = nblocks >> 3;  // blocks per XCD in the evenly divisible part
  if (per == 0u || b >= per * 8u) return b;
  return (b & 7u) * per + (b >> 3);
}

// Closest hits of one generation.  GEN0: items are pixels in 8x8-tile order, rays come from the camera;
// otherwise items are the entries of the input queue.
template <bool GEN0, bool FAST, bool SPH, bool SPILL, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_WF_MIN_WAVES) void k_wf_trace(DevScene sc, FrameParams fp, const QueuedRay* in_rays, const uint32_t* in_count, WfBuffers wb,
                                                      TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t item = xcd_contiguous_block(rc_bid(), rc_gdim()) * kBlock + rc_tid();
  LaneCounters cnt{};
  bool live;
  uint32_t out_index = 0;
  DRay ray = make_ray(point3(0, 0, 0), vec3(0, 0, 1));
  if (GEN0) {
    uint32_t x = 0, r = 0;
    live = tile_item_pixel(fp, item, x, r);
    if (live) {
      const uint32_t y = ((r / fp.band) * fp.parts + fp.part) * fp.band + (r % fp.band);
      ray = camera_ray(fp, x, y);
      out_index = r * fp.width + x;
    }
  } else {
    live = item < *in_count;
    if (live) {
      const QueuedRay q = in_rays[item];
      ray = make_ray(point3(q.ox, q.oy, q.oz), vec3(q.dx, q.dy, q.dz));
      out_index = item;
    }
  }
  if (live) {
    DHit hit;
    trace<true, FAST, SPH, FAST && (GEN0 ? RAYCA_WF_PRIMARY_WIDE : RAYCA_WF_BOUNCE_WIDE), SPILL, STATS, FAST && (GEN0 ? RAYCA_WF_PRIMARY_HALF : RAYCA_WF_BOUNCE_HALF), GEN0 ? RAYCA_LEAVE_K_WF_CAMERA : RAYCA_LEAVE_K_BOUNCE, GEN0 ? kSlackAlways : kSlackNever>(sc, ray, FLT_MAX, stack, hit, cnt);
    wb.hits[out_index] = make_float4(hit.t, __uint_as_float(hit.prim), hit.u, hit.v);
  }
  if (STATS) {
    unsigned long long b = cnt.boxes, t = cnt.tris, sb = cnt.slot_boxes, stt = cnt.slot_tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
      sb += __shfl_down(sb, off);
      stt += __shfl_down(stt, off);
    }
    if (__lane_id() == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}

// Shadow rays of one generation: a thread owns a pixel, traces its shadow rays in sample order and sums the
// direct lighting exactly like the NEE loop of k_generation (direct = direct + (lit ? x : BLACK)).
template <bool GEN0, bool FAST, bool SPH, bool SPILL, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_WF_MIN_WAVES) void k_wf_shadow(DevScene sc, FrameParams fp, const QueuedRay* in_rays, const uint32_t* in_count, WfBuffers wb,
                                                       PathBuffers pb, uint32_t depth, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t item = xcd_contiguous_block(rc_bid(), rc_gdim()) * kBlock + rc_tid();
  LaneCounters cnt{};
  uint32_t p = RAYCA_NONE;
  if (GEN0) {
    uint32_t x = 0, r = 0;
    if (tile_item_pixel(fp, item, x, r)) p = r * fp.width + x;
  } else if (item < *in_count) {
    p = in_rays[item].pixel;
  }
  bool live = false;
  if (p != RAYCA_NONE) {
    const uint32_t st = pb.state[(size_t)depth * pb.npix + p];
    live = st == kVertexLit || st == kVertexLitNoIndirect;
  }
  Color direct = black();
  uint32_t j = 0;
  while (live) {
    // the pixel's next sample that has to be traced: one that k_wf_shade marked as unable to contribute is "not lit" without
    // a traversal, which leaves the sum as it is (nee_irrelevant, trace_core.inc)
    while (j < wb.nls && (__float_as_uint(wb.sh_ray[2 * ((size_t)j * pb.npix + p) + 1].w) & kShadowSkip)) ++j;
    if (j == wb.nls) {
      pb.direct[(size_t)depth * pb.npix + p] = as_f4(direct);
      break;
    }
    const size_t e = (size_t)j * pb.npix + p;
    const float4 a = wb.sh_ray[2 * e], b = wb.sh_ray[2 * e + 1];
    const uint32_t quad = __float_as_uint(b.w) & kShadowQuad;
    const float t_stop = a.w;
    DHit hit;
    const bool found = trace<true, FAST, SPH, FAST && RAYCA_WF_SHADOW_WIDE, SPILL, STATS, FAST && RAYCA_WF_SHADOW_HALF, RAYCA_LEAVE_K_WF_SHADOW, kSlackNever>(sc, make_ray(point3(a.x, a.y, a.z), vec3(b.x, b.y, b.z)), t_stop, stack, hit, cnt);
    bool lit;
    if (quad) {
      lit = false;
      if (found) {
        const uint32_t hm = sc.ext[hit.prim].material;
        lit = hm != RAYCA_NONE && hm < sc.material_count && sc.materials[hm].emissive != 0u;
      }
    } else {
      lit = !(found && hit.t < t_stop);
    }
    direct = direct + (lit ? as_color(wb.sh_x[e]) : black());
    if (++j == wb.nls) {
      pb.direct[(size_t)depth * pb.npix + p] = as_f4(direct);
      live = false;
    }
  }
  if (STATS) {
    unsigned long long b = cnt.boxes, t = cnt.tris, sb = cnt.slot_boxes, stt = cnt.slot_tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
      sb += __shfl_down(sb, off);
      stt += __shfl_down(stt, off);
    }
    if (__lane_id() == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}

// HitInfo + sampling of one generation, one thread per ray.  Same statements as the shading part of
// k_generation's state machine; the shadow rays are written out instead of traced.
// RAYS (rayca_hip_radiance_device; !GEN0 only): the queue holds the caller's rays, not bounce rays -- the vertex is a path's first,
// which collects an emissive hit whatever the direct sampler is (pathtracer.rs:83-87), as GEN0 does for a camera ray.
constexpr uint32_t kShadeBlock = 256;  // 4 waves share one queue-append atomic (see the end of the kernel); 512 and 1024 were slower
template <int MODE, bool GEN0, bool FUSED, bool SPH, bool RAYS = false>
__global__ __launch_bounds__(kShadeBlock) void k_wf_shade(DevScene sc, FrameParams fp, const QueuedRay* in_rays, const uint32_t* in_count, QueuedRay* out_rays,
                                                      uint32_t* out_count, WfBuffers wb, PathBuffers pb, uint32_t depth, uint8_t* rgba8, float4* rgba32f,
                                                      unsigned long long* shade_stats) {
  const uint32_t i = rc_bid() * kShadeBlock + rc_tid();
  const uint32_t n_items = GEN0 ? fp.tile_count * 64u : *in_count;
  bool live = i < n_items;
  uint32_t p = 0, key = 0;
  DRay ray = make_ray(point3(0, 0, 0), vec3(0, 0, 1));
  uint32_t gx = 0, gr = 0;
  // generation 0 walks the image in 8x8 tiles like the trace kernel, so that a wave's bounce rays -- appended to the
  // queue together -- start from one patch of surface instead of a 64-pixel strip
  if (GEN0 && live) live = tile_item_pixel(fp, i, gx, gr);
  if (live) {
    if (GEN0) {
      const uint32_t r = gr, x = gx;
      p = r * fp.width + x;
      const uint32_t y = ((r / fp.band) * fp.parts + fp.part) * fp.band + (r % fp.band);
      ray = camera_ray(fp, x, y);
      key = rng_root(fp.seed, y * fp.width + x, fp.sample);
    } else {
      const QueuedRay q = in_rays[i];
      ray = make_ray(point3(q.ox, q.oy, q.oz), vec3(q.dx, q.dy, q.dz));
      p = q.pixel;
      key = q.key;
    }
  }
  const size_t slot = (size_t)depth * pb.npix + p;
  static_assert(!(GEN0 && RAYS), "the caller's rays come through the queue");
  const bool collect_emissive = (GEN0 || RAYS) ? true : (fp.direct_sampler == RAYCA_SAMPLER_NONE);
  const uint32_t nee_lights = (MODE == kModePath && fp.direct_sampler == RAYCA_SAMPLER_NEE) ? sc.light_count : 0u;
  bool want_bounce = false;
  QueuedRay next{};
  uint32_t n_shaded = 0, n_shadow = 0, n_bounce = 0;
  if (live) {
    const float4 hq = wb.hits[GEN0 ? p : i];
    DHit hit;
    hit.t = hq.x;
    hit.prim = __float_as_uint(hq.y);
    hit.u = hq.z;
    hit.v = hq.w;
    if (hit.prim == RAYCA_NONE) {
      if (FUSED) finalize_pixel(fp, black() + black(), p, rgba8, rgba32f);
      else pb.state[slot] = kVertexNone;
    } else {
      n_shaded = 1;
      Color color;
      bool emissive;
      ShadeCtx cx;
      shade_hit<SPH>(sc, ray, hit, MODE == kModePath, color, emissive, cx);
      if (MODE == kModeFlat) {
        if (FUSED) finalize_pixel(fp, black() + color, p, rgba8, rgba32f);
        else {
          pb.direct[slot] = as_f4(color);
          pb.state[slot] = kVertexEmissive;
        }
      } else if (collect_emissive && emissive) {
        pb.direct[slot] = as_f4(color);
        pb.state[slot] = kVertexEmissive;
      } else {
        uint32_t dim = 0, jj = 0;
        for (uint32_t li = 0; li < nee_lights; ++li)
          for (uint32_t k = 0; k < fp.light_samples; ++k, ++jj) {
            DRay sray;
            const NeeSample ns = nee_prepare(sc, fp, cx, li, k, key, dim, sray);
            const size_t e = (size_t)jj * pb.npix + p;
            wb.sh_ray[2 * e] = make_float4(sray.o.x, sray.o.y, sray.o.z, ns.t_stop);
            const uint32_t mark = (fp.nee_skip && nee_irrelevant(ns)) ? kShadowSkip : 0u;  // the shadow kernels do not traverse it
            wb.sh_ray[2 * e + 1] = make_float4(sray.d.x, sray.d.y, sray.d.z, __uint_as_float(ns.quad | mark));
            wb.sh_x[e] = as_f4(ns.x);
            n_shadow++;
          }
        if (nee_lights == 0u) pb.direct[slot] = as_f4(black());
        const uint32_t limit = fp.direct_sampler != RAYCA_SAMPLER_NONE ? fp.max_depth - 1u : fp.max_depth;
        if (depth < limit) {
          const float e1 = rng_f32(key, dim++), e2 = rng_f32(key, dim++);
          const bool hemi = fp.indirect_sampler == RAYCA_SAMPLER_HEMISPHERE;
          const float theta = hemi ? rc_acosf(e1) : rc_acosf(sqrtf(e1));   // (the host libm's bits: libm_exact.hpp)
          const float omega_a = 2.0f * kPi * e2;
          const F4 sdir = vec3(rc_cosf(omega_a) * rc_sinf(theta), rc_sinf(omega_a) * rc_sinf(theta), rc_cosf(theta));
          const F4 w = cx.normal;
          const F4 a = close(w, vec3(0, 1, 0)) ? vec3(1, 0, 0) : vec3(0, 1, 0);
          const F4 u = normalized(cross(a, w));
          F4 v = cross(w, u);
          if (hemi) v = normalized(v);
          const F4 omega_i = (sdir.x * u + sdir.y * v) + sdir.z * w;
          const Color brdf = surf_brdf(cx, omega_i);
          Color factor;
          if (hemi) factor = ((2.0f * kPi) * brdf) * clampf(dot(cx.normal, omega_i), 0.0f, 1.0f);
          else factor = kPi * brdf;
          pb.brdf[slot] = as_f4(factor);
          pb.state[slot] = kVertexLit;
          if (depth + 1u < fp.max_depth) {
            want_bounce = true;
            next.ox = cx.next_origin.x; next.oy = cx.next_origin.y; next.oz = cx.next_origin.z;
            next.dx = omega_i.x; next.dy = omega_i.y; next.dz = omega_i.z;
            next.pixel = p;
            next.key = rng_child(key, 0u);
            n_bounce = 1;
          }
        } else {
          pb.state[slot] = kVertexLitNoIndirect;
        }
      }
    }
  }
  if (MODE == kModePath && !FUSED) {
    // append to the next generation's queue: ballot/popcount compaction inside the wave as in push_ray, but ONE atomic
    // per block of 4 waves -- every wave of the launch adds to the same counter, and atomics on one address retire at
    // ~12 ns each: 32 k waves of a 1080p generation would spend 0.39 ms in that queue alone (measured: this kernel took
    // 0.39 ms with the bounce block and 0.09 ms without; 5-deep frame 6.58 -> 5.85 ms; blocks of 8 / 16 waves: 5.97 / 6.17 ms)
    __shared__ uint32_t wave_count[kShadeBlock / 64];
    __shared__ uint32_t block_base;
    const unsigned long long mask = __ballot(want_bounce);
    const uint32_t wave = rc_tid() >> 6, lane = __lane_id();
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (rc_tid() == 0) {
      uint32_t total = 0;
      for (uint32_t w = 0; w < kShadeBlock / 64; ++w) total += wave_count[w];
      block_base = total ? atomicAdd(out_count, total) : 0u;
    }
    __syncthreads();
    if (want_bounce) {
      uint32_t at = block_base;
      for (uint32_t w = 0; w < wave; ++w) at += wave_count[w];
      out_rays[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = next;
    }
  }
  // statistics: one atomic per wave and counter, spread over 64 lines (atomics on one line serialise at ~12 ns
  // each; with 32 k waves per frame that alone would be 0.4 ms)
  unsigned long long sh = n_shaded, s2 = n_shadow, b2 = n_bounce;
  for (int off = 32; off > 0; off >>= 1) {
    sh += __shfl_down(sh, off);
    s2 += __shfl_down(s2, off);
    b2 += __shfl_down(b2, off);
  }
  if (__lane_id() == 0 && (sh | s2 | b2)) {
    unsigned long long* line = shade_stats + (size_t)(rc_bid() & 63u) * 16u;
    atomicAdd(&line[0], sh);
    if (s2) atomicAdd(&line[1], s2);
    if (b2) atomicAdd(&line[2], b2);
  }
}

// rayca_hip_radiance_device: the caller's rays (6 f32 each: origin, direction) as the input queue of generation 0, one thread
// per ray.  Ray i is "pixel" i of the call's outputs and draws from the stream of pixel index first_index + i; the queue's
// count is written by the launch's first thread (the launch is in stream order behind whatever cleared the counters).
__global__ __launch_bounds__(kBlock) void k_enqueue_rays(const float* __restrict__ rays, uint32_t count, uint32_t first_index, uint32_t seed, uint32_t sample,
                                                         QueuedRay* __restrict__ out_rays, uint32_t* out_count) {
  const uint32_t i = rc_bid() * kBlock + rc_tid();   // (the host keeps count <= 2^31: no wrap)
  if (i == 0u) *out_count = count;
  if (i >= count) return;
  const float* r = rays + 6ull * i;
  QueuedRay q;
  q.ox = r[0]; q.oy = r[1]; q.oz = r[2];
  q.dx = r[3]; q.dy = r[4]; q.dz = r[5];
  q.pixel = i;
  q.key = rng_root(seed, first_index + i, sample);
  out_rays[i] = q;
}
