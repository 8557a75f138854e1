// kernels.hip -- hand-written gfx950 kernels of the rayca hot path.
//
//   k_generation<..>  one persistent-wavefront kernel per ray generation:
//                     generation 0 = camera rays (rayca-soft/src/scene.rs:117-150),
//                     generation g = the g-th bounce of Pathtracer::trace_impl
//                     (integrator/pathtracer.rs:68-106).  Each wave pulls batches of 64 rays from a
//                     per-XCD work counter, traverses the BVH with a per-lane node stack in LDS
//                     (TlasNode/BvhNode::intersects, bvh/tlas.rs:136-180, bvh/blas.rs:129-177),
//                     intersects triangles (rayca-geometry/src/triangle.rs:84-159), shades the hit
//                     (hit.rs, brdf/ggx.rs, sampler/nee.rs, sampler/cosine.rs) and compacts the
//                     surviving rays of the next generation with __ballot/__popcll/__shfl.
//   k_resolve         folds the per-depth records back in the reference's evaluation order,
//                     accumulates samples, applies gamma and quantises (scene.rs:146-148).
//   k_trace_rays      Tlas::intersects for caller-supplied rays (parity/debug entry).
//   k_query_rays      the same for rays in device memory, with a distance bound and an occlusion form
//                     (rayca_hip_query_device where the lane-refill kernel of refill.hip cannot run).
//   k_surface,        surface records (shade_hit) for hit records, and a frame's camera rays, in device memory
//   k_camera_rays     (surface.inc: rayca_hip_surface_device, rayca_hip_camera_rays_device).
//   k_nearest         nearest-point queries: the closest surface point to points in device memory, within a radius
//                     (nearest.inc: rayca_hip_nearest_device).
//   k_cdf_*,          surface sampling: the slots' areas into integer weights and their exact prefix sums, and area-weighted points
//   k_sample_surface  on the triangles drawn from that table (sample.inc: rayca_hip_surface_cdf_device,
//                     rayca_hip_surface_sample_device).
//   k_hits            multi-hit ray queries: the first k hits along rays in device memory, in order, or their number
//                     (hits.inc: rayca_hip_hits_device).
//   k_signed          signed distance and occupancy: the nearest surface point of points or grid points in device memory and a
//                     vote of crossing-count rays on the side they lie on (signed.inc: rayca_hip_signed_device).
//   k_ambient_rays,   hemisphere visibility at points: occlusion rays made in registers, one per lane, and the fold of a point's
//   k_ambient_finish  mask word into hits, openness and the bent normal (ambient.inc: rayca_hip_ambient_device; the lane-refill
//                     form is refill.hip k_ambient_refill).
//   k_probe_rays,     irradiance volumes: the occlusion rays from a point to the eight probes of its grid cell, one per lane, and the
//   k_probe_fold      blend of those probes' SH9 records into the light at the point (probes.inc: rayca_hip_probe_lookup_device; the
//                     lane-refill form is refill.hip k_probe_refill).
//   k_direct_rays,    direct light at points: the shadow rays of a range of the scene's lights, made in registers, one per lane, and
//   k_direct_fold     the sum of the lit samples in a fixed order (direct.inc: rayca_hip_direct_device; the lane-refill form is
//                     refill.hip k_direct_refill).
//   k_enqueue_gather, irradiance at points: the same rays written straight into the frame driver's generation-0 queue, and the
//   k_gather_fold     fold of their radiance into irradiance and nine spherical-harmonic coefficients per point
//                     (gather.inc: rayca_hip_gather_device).
//   tile_pixel, ...   what the image-space passes below share: the 64 x 4 tile prologue, the guide terms of a tap, luminance,
//                     albedo (de)modulation and the output stage (image_pass.inc; their entry points are in post.inc).
//   k_atrous,         the edge-avoiding a-trous denoiser on a frame and its G-buffer in device memory
//   k_denoise_*       (denoise.inc: rayca_hip_denoise_device).
//   k_accumulate      temporal accumulation of a frame into a history, with reprojection through the previous camera
//                     (temporal.inc: rayca_hip_accumulate_device).
//   k_plan_*,         adaptive sampling: a film's variance into per-pixel weights, ray offsets (an exact prefix sum) and camera
//   k_film_fold       rays, and the fold of the samples traced along them back into the film
//                     (adaptive.inc: rayca_hip_sample_plan_device, rayca_hip_film_fold_device).
//   k_variance_init,  the variance-guided a-trous filter: the film's luminance variance steers the luminance weight and is
//   k_atrous_var      filtered along with the colour (denoise_variance.inc: rayca_hip_denoise_variance_device).
//   k_upsample        a low-resolution frame onto a full-size G-buffer: a joint bilateral upsample
//                     (upsample.inc: rayca_hip_upsample_device).
//   k_meter_hist,     exposure metering and tone mapping: a luminance histogram of a linear frame (LDS bins, integer atomics),
//   k_exposure,       the exposure record made from it by one wave, and the display operator in front of the output stage
//   k_tonemap         (tonemap.inc: rayca_hip_meter_device, rayca_hip_tonemap_device).
//
// No MFMA anywhere: there is no dense contraction in this path.  Built with -ffp-contract=off.
#include "no_pk.hpp"   // RAYCA_NO_PK_F32: no packed f32 arithmetic in the traversal, leaf, shading and BRDF code
RAYCA_NO_PK_BEGIN
#include <hip/hip_runtime.h>
#include "device_types.hpp"
RAYCA_NO_PK_END

namespace rayca {
namespace {

RAYCA_NO_PK_BEGIN
#include "trace_core.inc"

// One generation of rays.  Per lane a small state machine around ONE traversal call site:
//   primary ray -> shade -> [NEE shadow ray]* -> bounce sample -> done
// so the traversal loop is instantiated once per kernel and the registers that must survive it are
// the ray, the hit, the compact ShadeCtx and a few colours.
// k_generation's arguments as ONE aggregate, so that every field has a known offset in the kernel-argument segment.  Hot fields
// -- what trace() and NodeStack read of `sc`, `heads`, `depth`, `tl` -- are read from the argument itself and live in SGPRs over
// the persistent loop.  Cold fields -- the camera and sampling fields of `fp`, the shading tables of `sc`, `pb`, the queues, the
// counters and the outputs -- are read through GEN_COLD(member) in the block that uses them (cold_arg, trace_core.inc): once per
// batch, vertex or sample, a scalar load from the (cached) argument segment instead of an SGPR kept, or spilled, over the loop.
// -DRAYCA_COLD_ARGS=0: every field from the by-value argument, for A/B runs.
#ifndef RAYCA_COLD_ARGS
#define RAYCA_COLD_ARGS 1
#endif
struct GenArgs {
  DevScene sc;
  FrameParams fp;
  uint32_t* heads;
  const QueuedRay* in_rays;
  const uint32_t* in_count;
  QueuedRay* out_rays;
  uint32_t* out_count;
  PathBuffers pb;
  uint32_t depth;
  uint8_t* rgba8;
  float4* rgba32f;
  TraceCounters* counters;
  TraceLaunch tl;
  uint32_t* clear;   // FUSED: the work-counter set this launch does not draw from (kCounterSetWords dwords), zeroed by block 0; or null
};
#if RAYCA_COLD_ARGS
#define GEN_COLD(member) cold_arg<decltype(GenArgs::member)>((uint32_t)offsetof(GenArgs, member))
#else
#define GEN_COLD(member) (a.member)
#endif
// LAST (Path only; Flat does not read it): the generation behind which no vertex samples a bounce -- `depth >= limit` of the tail
// below holds for every vertex, which the host knows from the Config (last_form, select.inc).  The tail then takes the direct sum
// back from LDS and writes the vertex's record; the bounce sampler with its double-precision libm_exact functions, surf_brdf, the
// factor record, push_ray, the bounce counter and the fetch of the parked context are not compiled in.  The records are those the
// general form writes for such a vertex: the same direct sum, kVertexLitNoIndirect, pb.brdf untouched.
// FUSED: the kernel writes the pixel and no record -- `pb` is not read.  Flat (generation 0), and Path with GEN0 && LAST: the one-sample
// depth-1 path frame, whose every lane ends in this launch.  A lane that finishes leaves the sum k_resolve would have folded for one
// depth and sample 0 -- miss: black() + black(); emissive hit: black() + color; a vertex with all its samples in:
// black() + (direct + black()), the `+ black()` terms being the reference's evaluation order (k_resolve) -- and the gamma + quantise +
// store tail runs once per batch behind the loop, with the wave reconverged: whole 8 x 8 tile stores.  Path keeps that sum in the
// parked direct sum's slot (park_sum_set), which a lane that ends without samples does not need: as a loop-carried value it would be
// three more registers over trace().  The same launch zeroes the work-counter set it does not draw from (GenArgs.clear), for the
// context's next frame: what k_resolve's clear did for a frame that has a k_resolve.
template <int MODE, bool GEN0, bool ORDERED, bool FUSED, bool FAST, bool SPH, bool WIDE, bool SPILL, bool STATS, bool HALF, bool LAST>
__global__ __launch_bounds__(kGenBlock, MODE == kModeFlat ? RAYCA_MIN_WAVES_FLAT : path_waves(STATS, SPH)) void k_generation(GenArgs a) {
  static_assert(!FUSED || MODE == kModeFlat || (MODE == kModePath && GEN0 && LAST && !STATS), "FUSED: Flat, or the path frame's only generation on the last-vertex form");
  const TraceLaunch& tl = a.tl;
  uint32_t* const heads = a.heads;
  const uint32_t depth = a.depth;
  extern __shared__ uint32_t lds_stack[];
  // (workgroups of kGenBlock threads: the stride of the stack rows and of the parked context; no barrier, nothing shared between waves)
  NodeStack<SPILL, kGenBlock> stack = make_stack<SPILL, kGenBlock>(lds_stack, tl, rc_bid() * kGenBlock + rc_tid());
  // behind the stack rows: the workgroup's parked ShadeCtx, one slot a lane (path frames only; the host sizes the allocation)
  const CtxSlot ctx_slot{lds_stack + tl.lds_entries * kGenBlock};
  constexpr bool PARK = RAYCA_PARK_CTX && MODE == kModePath;
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  WorkCursor wc{};
  const uint32_t total = GEN0 ? GEN_COLD(fp).tile_count : (*GEN_COLD(in_count) + 63u) / 64u;
  LaneCounters cnt{};
  uint32_t n_shaded = 0, n_shadow = 0, n_bounce = 0;
  const bool collect_emissive = GEN0 ? true : (GEN_COLD(fp).direct_sampler == RAYCA_SAMPLER_NONE);
  const uint32_t nee_lights = (MODE == kModePath && GEN_COLD(fp).direct_sampler == RAYCA_SAMPLER_NEE) ? GEN_COLD(sc).light_count : 0u;
  if (FUSED && rc_bid() == 0) {
    // the other counter set of the context: no wave of this launch reads it, and the passes of one context are ordered (the
    // context-pass protocol), so whoever drew from it has retired and the next frame finds it zero without a fill launch
    if (uint32_t* const clear = GEN_COLD(clear))
      for (uint32_t i = rc_tid(); i < kCounterSetWords; i += kGenBlock) clear[i] = 0u;
  }

  for (;;) {
    const uint32_t batch = next_batch(heads, total, home, wc, tl.ticket);
    if (batch == RAYCA_NONE) break;
    bool live;
    uint32_t p = 0, key = 0;
    DRay ray;
    if (GEN0) {
      const FrameParams& fp = GEN_COLD(fp);
      const uint32_t ty = batch / fp.tiles_x, tx = batch - ty * fp.tiles_x;
      const uint32_t x = tx * kTileW + (lane & (kTileW - 1u)), r = ty * kTileH + (lane >> RAYCA_TILE_W_LOG2);
      live = x < fp.width && r < fp.rows;
      const uint32_t y = ((r / fp.band) * fp.parts + fp.part) * fp.band + (r % fp.band);
      p = r * fp.width + x;
      if (live) {
        ray = camera_ray(fp, x, y);
        key = rng_root(fp.seed, y * fp.width + x, fp.sample);
      }
    } else {
      const uint32_t i = batch * 64u + lane;
      live = i < *GEN_COLD(in_count);
      if (live) {
        const QueuedRay q = GEN_COLD(in_rays)[i];
        ray = make_ray(point3(q.ox, q.oy, q.oz), vec3(q.dx, q.dy, q.dz));
        p = q.pixel;
        key = q.key;
      }
    }
    const size_t slot = FUSED ? 0 : (size_t)depth * GEN_COLD(pb).npix + p;
    bool in_shadow = false;
    // shadow rays: the any-hit bound.  A point light's is its distance (a finite square root, never FLT_MAX); FLT_MAX
    // means "closest hit wanted": camera and bounce rays, and the shadow ray of a quad light (NeeSample.quad)
    float t_stop = FLT_MAX;
    ShadeCtx cx;
    Color ns_x = black();  // the pending NEE sample's contribution if its light turns out to be visible   (PARK: park_sample)
    Color direct = black();  // sum of the direct samples so far                                           (PARK: park_sum_add)
    uint32_t li = 0, k = 0, dim = 0;
    // FUSED: a lane that finishes leaves its pixel sum in `direct` (Flat) or in the parked sum's slot (Path); the gamma + quantise +
    // store tail runs once per batch with the wave reconverged, not inside the divergent state machine
    const bool has_pixel = live;
    // Path: a vertex whose direct samples are all in leaves the loop with `tail` set; its record, the bounce sample and the
    // next generation's ray are made behind the loop, with the wave reconverged -- so the bounce ray is not a loop-carried
    // value (eight registers the traversal loop had to carry for nothing) and the sampling code runs with full lanes
    bool tail = false;

    while (live) {
      DHit hit;
      constexpr int kLeaveK = !ORDERED ? 0 : (MODE == kModeFlat ? RAYCA_LEAVE_K_CAMERA : (GEN0 ? RAYCA_LEAVE_K_PATH0 : RAYCA_LEAVE_K_BOUNCE));
      constexpr int kSlackForm = MODE == kModeFlat ? kSlackAlways : (GEN0 ? kSlackPerWave : kSlackNever);
      const bool found = trace<ORDERED, FAST, SPH, WIDE, SPILL, STATS, HALF, kLeaveK, kSlackForm>(a.sc, ray, t_stop, stack, hit, cnt);
      if (!in_shadow) {
        if (!found) {
          if (FUSED && PARK) park_sum_reset<kGenBlock>(ctx_slot);  // black() + black(): +0.0f thrice and alpha 1, black()'s own bits
          else if (FUSED) direct = black() + black();  // unwrap_or(BLACK), color += it
          else GEN_COLD(pb).state[slot] = kVertexNone;
          live = false;
        } else {
          n_shaded++;
          Color color;
          bool emissive;
          const PathBuffers& pb = GEN_COLD(pb);
          shade_hit<SPH>(GEN_COLD(sc), ray, hit, MODE == kModePath, color, emissive, cx);
          if (MODE == kModeFlat) {  // Flat::trace  integrator/flat.rs:16-28
            if (FUSED) direct = black() + color;
            else {
              pb.direct[slot] = as_f4(color);
              pb.state[slot] = kVertexEmissive;
            }
            live = false;
          } else if (collect_emissive && emissive) {  // pathtracer.rs:83-87
            if (FUSED && PARK) park_sum_set<kGenBlock>(ctx_slot, black() + color);
            else if (FUSED) direct = black() + color;
            else {
              pb.direct[slot] = as_f4(color);
              pb.state[slot] = kVertexEmissive;
            }
            live = false;
          } else {
            in_shadow = true;  // enter the NEE loop (possibly empty)
            if (PARK) {
              park_ctx<kGenBlock>(ctx_slot, cx);
              park_sum_reset<kGenBlock>(ctx_slot);
            }
          }
        }
      } else {
        // outcome of the pending NEE sample
        bool lit;
        if (t_stop == FLT_MAX) {  // quad light: "lit iff the closest hit is emissive" (nee.rs:103-104)
          lit = false;
          if (found) {
            const DevScene& sc = GEN_COLD(sc);
            const uint32_t hm = sc.ext[hit.prim].material;
            lit = hm != RAYCA_NONE && hm < sc.material_count && sc.materials[hm].emissive != 0u;
          }
        } else {
          lit = !(found && hit.t < t_stop);  // nee.rs:152-156
        }
        if (PARK) {
          park_sum_add<kGenBlock>(ctx_slot, lit);
        } else {
          direct = direct + (lit ? ns_x : black());
        }
        if (++k == GEN_COLD(fp).light_samples) {
          k = 0;
          ++li;
        }
      }
      if (live && in_shadow) {
        // the next sample that has to be traced.  A sample that cannot contribute (nee_irrelevant, trace_core.inc) is booked as
        // "not lit" -- the sum stays as it is, the same bits as adding black() -- and the lane prepares the one after it
        // instead of entering trace() for it; ORDERED only: the exhaustive form reproduces the reference's test counts
        bool pending = false;
        while (li < nee_lights) {
          // (its own LDS slot: no barrier; the compiler orders a lane's LDS accesses.  Fetched per trip: a context that stayed in
          // registers over the loop's back edge doubled the kernel's spills)
          if (PARK) cx = unpark_ctx<kGenBlock>(ctx_slot);
          const FrameParams& fp = GEN_COLD(fp);
          const NeeSample ns = nee_prepare(GEN_COLD(sc), fp, cx, li, k, key, dim, ray);
          const bool irrelevant = ORDERED && nee_irrelevant(ns);
          if (STATS) {  // booked at once by one lane: a counter of its own would be one more register the trace loop carries
            const unsigned long long m = __ballot(irrelevant);
            if (m != 0ull && lane == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(&GEN_COLD(counters)->nee_irrelevant, (unsigned long long)__popcll(m));
          }
          if (irrelevant && fp.nee_skip) {
            if (++k == fp.light_samples) {
              k = 0;
              ++li;
            }
            continue;
          }
          if (PARK) park_sample<kGenBlock>(ctx_slot, ns.x);
          else ns_x = ns.x;
          t_stop = ns.t_stop;
          pending = true;
          break;
        }
        if (!pending) {
          tail = true;
          live = false;
        }
      }
    }
    if (FUSED) {
      if (has_pixel) {
        if (PARK) direct = unpark_sum<kGenBlock>(ctx_slot);
        // the last vertex of a path (pathtracer.rs:89-93 with depth >= limit), folded as k_resolve folds one depth
        if (MODE == kModePath && tail) direct = black() + (direct + black());
        finalize_pixel(GEN_COLD(fp), direct, p, GEN_COLD(rgba8), GEN_COLD(rgba32f));
      }
      if (MODE == kModePath) n_shadow += (uint32_t)__popcll(__ballot(tail)) * nee_lights * GEN_COLD(fp).light_samples;
    } else if (MODE == kModePath && LAST) {
      // the last vertex of a path: its direct sum is its record (pathtracer.rs:89-93 with depth >= limit); the context stays parked
      if (tail) {
        const PathBuffers& pb = GEN_COLD(pb);
        if (PARK) direct = unpark_sum<kGenBlock>(ctx_slot);
        pb.direct[slot] = as_f4(direct);
        pb.state[slot] = kVertexLitNoIndirect;
      }
      n_shadow += (uint32_t)__popcll(__ballot(tail)) * nee_lights * GEN_COLD(fp).light_samples;
    } else if (MODE == kModePath) {
      const FrameParams& fp = GEN_COLD(fp);
      const PathBuffers& pb = GEN_COLD(pb);
      bool want_bounce = false;
      QueuedRay next{};
      if (tail) {
        // all direct samples done: Pathtracer::trace_impl tail  pathtracer.rs:89-105
        const uint32_t limit = fp.direct_sampler != RAYCA_SAMPLER_NONE ? fp.max_depth - 1u : fp.max_depth;
        const bool hemi = fp.indirect_sampler == RAYCA_SAMPLER_HEMISPHERE;
        F4 sdir = vec3(0.0f, 0.0f, 0.0f);
        if (depth < limit) {
          // CosineSampler::get_random_dir  sampler/cosine.rs:65-88 ; HemisphereSampler  hemisphere.rs:17-40.  The direction in the
          // sampler's own frame only needs the two random numbers: made before the parked context comes back from LDS, so that
          // the double-precision temporaries of libm_exact.hpp (the host libm's bits) and the context are not live together
          const float e1 = rng_f32(key, dim++), e2 = rng_f32(key, dim++);
          const float theta = hemi ? rc_acosf(e1) : rc_acosf(sqrtf(e1));
          const float omega_a = 2.0f * kPi * e2;
          const float st = rc_sinf(theta);
          sdir = vec3(rc_cosf(omega_a) * st, rc_sinf(omega_a) * st, rc_cosf(theta));
        }
        if (PARK) {
          cx = unpark_ctx<kGenBlock>(ctx_slot);
          direct = unpark_sum<kGenBlock>(ctx_slot);
        }
        pb.direct[slot] = as_f4(direct);
        if (depth < limit) {
          const F4 w = cx.normal;
          const F4 a = close(w, vec3(0, 1, 0)) ? vec3(1, 0, 0) : vec3(0, 1, 0);
          const F4 u = normalized(cross(a, w));
          F4 v = cross(w, u);
          if (hemi) v = normalized(v);
          const F4 omega_i = (sdir.x * u + sdir.y * v) + sdir.z * w;
          const Color brdf = surf_brdf(cx, omega_i);
          // the factor SoftSampler::get_radiance applies to the incoming radiance, evaluated in its
          // order up to the point where the child's result enters: cosine.rs:90-99 `PI * brdf`,
          // hemisphere.rs:42-52 `2.0 * PI * brdf * cosine_law`
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
          }
        } else {
          pb.state[slot] = kVertexLitNoIndirect;
        }
      }
      // ray counts, wave-uniform (per-lane counters would be loop-carried registers of the traversal loop): every vertex
      // that reaches `tail` has traced all of its nee_lights x light_samples shadow rays
      n_shadow += (uint32_t)__popcll(__ballot(tail)) * nee_lights * fp.light_samples;
      n_bounce += (uint32_t)__popcll(__ballot(want_bounce));
      push_ray(want_bounce, next, GEN_COLD(out_rays), GEN_COLD(out_count));
    }
  }
  if (STATS) {
    // wave reduction, then one atomic per wave and counter
    unsigned long long b = cnt.boxes, t = cnt.tris, sh = n_shaded, sb = cnt.slot_boxes, stt = cnt.slot_tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
      sh += __shfl_down(sh, off);
      sb += __shfl_down(sb, off);
      stt += __shfl_down(stt, off);
    }
    if (lane == 0) {
      TraceCounters* const counters = GEN_COLD(counters);
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->shaded, sh);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
  if (MODE == kModePath) {
    const unsigned long long s2 = n_shadow, b2 = n_bounce;  // already whole-wave sums
    if ((FUSED ? lane_now() : lane) == 0 && (s2 | b2)) {
      TraceCounters* const counters = GEN_COLD(counters);
      atomicAdd(&counters->shadow, s2);
      if (!LAST) atomicAdd(&counters->bounce, b2);
    }
  }
}

// Fold the per-depth records in the reference's order (pathtracer.rs:23-66,94-105):
//   L_g = direct_g + (BLACK + (BLACK + (factor_g * L_{g+1}) * weight) / light_samples)
// `clear` (optional): `clear_words` dwords zeroed by the first block -- the work counters of this frame context, which the
// generation kernel in front of this one has finished with (same stream), so that the next frame of the context needs no
// memset launch of its own (a frame is three launches then instead of four: what a rank's share of a frame costs on the
// host is what limits an 8-GPU run).
__global__ __launch_bounds__(kBlock) void k_resolve(FrameParams fp, PathBuffers pb, uint32_t depths, float4* accum, uint8_t* rgba8, float4* rgba32f,
                                                    uint32_t* clear, uint32_t clear_words) {
  if (clear && rc_bid() == 0)
    for (uint32_t i = rc_tid(); i < clear_words; i += rc_bdim()) clear[i] = 0u;
  const uint32_t p = rc_bid() * rc_bdim() + rc_tid();
  if (p >= pb.npix) return;
  bool some = false;
  Color L = black();
  for (int g = (int)depths - 1; g >= 0; --g) {
    const size_t slot = (size_t)g * pb.npix + p;
    const uint32_t st = pb.state[slot];
    if (st == kVertexNone) {
      some = false;
    } else if (st == kVertexEmissive) {
      some = true;
      L = as_color(pb.direct[slot]);
    } else {
      const Color direct = as_color(pb.direct[slot]);
      Color indirect = black();
      if (st == kVertexLit) {
        Color li = black();
        if (some) {
          const Color factor = as_color(pb.brdf[slot]);
          const Color x = (factor * L) * 1.0f;  // ... * indirect_sample * weight (weight = 1 without roulette)
          li = li + x;
        }
        indirect = indirect + li / (float)fp.light_samples;
      }
      L = direct + indirect;
      some = true;
    }
  }
  const Color c = some ? L : black();
  const Color prev = fp.sample == 0 ? black() : as_color(accum[p]);
  const Color acc = prev + c;
  if (fp.sample + 1u == fp.spp) finalize_pixel(fp, acc, p, rgba8, rgba32f);
  else accum[p] = as_f4(acc);
}

template <bool ORDERED, bool FAST, bool SPH, bool WIDE, bool SPILL, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_TRACE_MIN_WAVES) void k_trace_rays(DevScene sc, const float* rays, uint32_t count, float* t_out, uint32_t* prim_out, float* uv_out,
                                                       TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t i = rc_bid() * rc_bdim() + rc_tid();
  LaneCounters cnt{};
  if (i < count) {
    const float* r = rays + 6ull * i;
    const DRay ray = make_ray(point3(r[0], r[1], r[2]), vec3(r[3], r[4], r[5]));
    DHit hit;
    const bool found = trace<ORDERED, FAST, SPH, WIDE, SPILL, STATS, false, 0, kSlackAlways>(sc, ray, FLT_MAX, stack, hit, cnt);
    t_out[i] = found ? hit.t : FLT_MAX;
    prim_out[i] = found ? hit.prim : RAYCA_NONE;
    uv_out[2 * i] = found ? hit.u : 0.0f;
    uv_out[2 * i + 1] = found ? hit.v : 0.0f;
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

// k_trace_rays' sibling for rayca_hip_query_device where the lane-refill kernel (refill.hip k_query_refill) cannot run: scenes
// without the reference-leaf filter, exhaustive traversal, and the first calls on a scene whose 4-wide / fp16 nodes are still
// being made.  One ray per lane, rays, bounds and results in device memory.  CLOSEST traces unbounded and applies the bound
// to the record (trace()'s t_stop would end the search at the first hit in front of it); OCCLUDED hands trace() the bound as
// t_stop -- for an unbounded ray the largest float below FLT_MAX, so that the early out is on for it too: a hit at or beyond
// that value merely lets the search run to its end, and query_found() decides either way.
template <bool ORDERED, bool FAST, bool SPH, bool WIDE, bool SPILL, bool STATS, bool OCCLUDED>
__global__ __launch_bounds__(kBlock, RAYCA_TRACE_MIN_WAVES) void k_query_rays(DevScene sc, QueryIo q, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t i = rc_bid() * rc_bdim() + rc_tid();
  LaneCounters cnt{};
  if (i < q.count) {
    bool dead;
    const float bound = query_bound(q, i, dead);
    DHit hit;
    hit.t = INFINITY;
    hit.prim = RAYCA_NONE;
    hit.u = hit.v = 0.0f;
    if (!dead) {
      const float* r = q.rays + 6ull * i;
      const DRay ray = make_ray(point3(r[0], r[1], r[2]), vec3(r[3], r[4], r[5]));
      const float t_stop = !OCCLUDED ? FLT_MAX : (bound < FLT_MAX ? bound : __uint_as_float(0x7F7FFFFEu));
      trace<ORDERED, FAST, SPH, WIDE, SPILL, STATS, false, 0, kSlackAlways>(sc, ray, t_stop, stack, hit, cnt);
    }
    query_store<OCCLUDED>(q, i, hit, query_found(hit, bound));
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

#include "general.inc"
#include "wavefront.inc"
#include "surface.inc"
#include "nearest.inc"
#include "sample.inc"
#include "hits.inc"
#include "signed.inc"
#include "ambient.inc"
#include "probes.inc"
#include "gather.inc"
#include "direct.inc"
RAYCA_NO_PK_END   // (the image-space passes below keep the packed forms: whole float4 pixels)
#include "image_pass.inc"
#include "denoise.inc"
#include "denoise_variance.inc"
#include "temporal.inc"
#include "adaptive.inc"
#include "upsample.inc"
#include "tonemap.inc"

}  // namespace
}  // namespace rayca

#include "api.inc"
