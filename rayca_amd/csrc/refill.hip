// refill.hip -- camera rays of a Flat frame with LANE REFILL (gfx950).
//
// k_generation gives a wave 64 rays and keeps it until the slowest of them has finished.  Where the length of a ray's
// walk through the tree varies a lot inside a tile -- the 1 M-triangle soup: free paths through a random cloud are
// exponentially distributed, so the longest of 64 is about 4.7 times the mean -- most lanes of a wave idle most of the
// time (measured: 17 % lane utilisation in the node loop, 21.5 % of VALU thread-cycles active).  Here a wave is a
// persistent pool of 64 lanes: when no more than RAYCA_REFILL_THRESHOLD of them are still traversing, the finished
// ones shade and store their pixel (Flat::trace, integrator/flat.rs:16-28; scene.rs:146-148) and take new pixels from
// the wave's current 8x8 tile (work tickets as in k_generation: one counter per XCD), while the long rays keep their
// place.  Same arithmetic, same node_step / test_leaf / shade_hit as every other kernel (trace_core.inc): the frame is
// bit-identical to k_generation's (tests/test_gpu_engines.py); which of the two renders a scene's Flat frames is decided
// by timing both on that scene (RaycaScene::Tune in api.inc).
//
// Coherent scenes lose with it (the atrium's camera rays: new rays at the root next to old rays deep in the tree
// diverge in their node addresses), which is why it is a per-scene choice and not the default.
#include "no_pk.hpp"   // RAYCA_NO_PK_F32
RAYCA_NO_PK_BEGIN
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "refill.hpp"
RAYCA_NO_PK_END

namespace rayca {
namespace {

RAYCA_NO_PK_BEGIN
#include "trace_core.inc"
#include "ambient.inc"   // ambient_point, ambient_ray: what k_ambient_refill makes its rays with
#include "probes.inc"    // probe_point, probe_cell, probe_corner, probe_ray: what k_probe_refill makes its rays with
#include "direct.inc"    // direct_point, direct_sample, direct_lit: what k_direct_refill makes and judges its samples with

#ifndef RAYCA_REFILL_THRESHOLD
#define RAYCA_REFILL_THRESHOLD 44
#endif
#ifndef RAYCA_REFILL_SCHED
#define RAYCA_REFILL_SCHED 0
#endif
#ifndef RAYCA_REFILL_LEAVE_K
#define RAYCA_REFILL_LEAVE_K 32
#endif
#ifndef RAYCA_REFILL_WAVES
#define RAYCA_REFILL_WAVES RAYCA_MIN_WAVES_FLAT
#endif
#ifndef RAYCA_REFILL_NODE_W
#define RAYCA_REFILL_NODE_W 1
#endif
#ifndef RAYCA_REFILL_LEAF_W
#define RAYCA_REFILL_LEAF_W 1
#endif

template <bool SPH, bool WIDE, bool SPILL, bool STATS, bool HALF>
__global__ __launch_bounds__(kBlock, RAYCA_REFILL_WAVES) void k_flat_refill(DevScene sc, FrameParams fp, uint32_t* heads, uint8_t* rgba8, float4* rgba32f,
                                                                             TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  WorkCursor wc{};
  LaneCounters cnt{};
  uint32_t n_shaded = 0;
  // lane state: a ray that is still traversing (cur != kTerminated), a finished ray waiting to be retired (has), or nothing
  bool has = false;
  uint32_t cur = kTerminated, p = 0;
  DRay ray{};
  FastRay fr{};
  DHit hit{};
  float limit = INFINITY;
  // wave state: pixels [pool_next, pool_end) of the tile list (64 per tile, in tile order) not handed out yet
  uint32_t pool_next = 0, pool_end = 0;
  bool dry = false;  // the work counters are exhausted

  for (;;) {
    const uint32_t n_active = (uint32_t)__popcll(__ballot(cur != kTerminated));
    if (n_active <= (dry ? 0u : (uint32_t)RAYCA_REFILL_THRESHOLD)) {
      if (has && cur == kTerminated) {  // retire: Flat::trace + the pixel store
        Color sum = black() + black();  // unwrap_or(BLACK), color += it
        if (hit.prim != RAYCA_NONE) {
          n_shaded++;
          Color color;
          bool emissive;
          ShadeCtx unused;
          shade_hit<SPH>(sc, ray, hit, false, color, emissive, unused);
          sum = black() + color;
        }
        finalize_pixel(fp, sum, p, rgba8, rgba32f);
        has = false;
      }
      if (dry && n_active == 0u) break;  // every lane reaches this: n_active and dry are wave-uniform
      while (!dry) {
        const unsigned long long idle = __ballot(!has);
        if (idle == 0ull) break;
        if (pool_next == pool_end) {
          const uint32_t batch = next_batch(heads, fp.tile_count, home, wc, tl.ticket);
          if (batch == RAYCA_NONE) {
            dry = true;
            break;
          }
          pool_next = batch * 64u;
          pool_end = pool_next + 64u;
        }
        const uint32_t avail = pool_end - pool_next;
        const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
        if (!has && rank < avail) {
          const uint32_t idx = pool_next + rank, batch = idx >> 6, l = idx & 63u;
          const uint32_t ty = batch / fp.tiles_x, tx = batch - ty * fp.tiles_x;
          const uint32_t x = tx * kTileW + (l & (kTileW - 1u)), r = ty * kTileH + (l >> RAYCA_TILE_W_LOG2);
          if (x < fp.width && r < fp.rows) {  // (pixels of a ragged edge tile outside the frame are skipped: the lane asks again)
            const uint32_t y = ((r / fp.band) * fp.parts + fp.part) * fp.band + (r % fp.band);
            p = r * fp.width + x;
            ray = camera_ray(fp, x, y);
            // prologue of trace(): Tlas::intersects tests the root box first (blas.rs:136-139)
            fr = make_fast(sc, ray, HALF);
            hit.t = INFINITY;
            hit.prim = RAYCA_NONE;
            hit.u = hit.v = 0.0f;
            limit = INFINITY;
            stack.clear();
            float tmin;
            if (STATS) cnt.boxes++;
            cur = slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin)
                      ? (WIDE ? sc.root_ref4 : (!HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref))
                      : kTerminated;
            has = true;
          }
        }
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        pool_next += n_idle < avail ? n_idle : avail;
      }
    }
    // One trip of the traversal for the lanes that hold a ray: EITHER a node step for the lanes that are searching (cur is an
    // inner node) OR the leaf test for the lanes that hold a leaf -- whichever side has more lanes (weighted:
    // RAYCA_REFILL_NODE_W searching lanes count like RAYCA_REFILL_LEAF_W leaf lanes).  trace()'s while-while form keeps
    // stepping until the slowest search of the wave has found its leaf; with refilled lanes descending from the root next
    // to lanes deep in the tree that idles most of the wave (measured on the soup: 0.29 lane utilisation in the node loop,
    // 9.5 ms per frame; with the majority rule 0.6-0.7 in both loops).  Every lane still performs its own steps in its own
    // order: only the interleaving of lanes changes, not a single result.
#if RAYCA_REFILL_SCHED == 1
    const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
    const bool at_leaf = (cur & kLeafFlag) != 0u;
    const uint32_t n_search = (uint32_t)__popcll(__ballot(searching)), n_leaf = (uint32_t)__popcll(__ballot(at_leaf));
    if (n_search * (uint32_t)RAYCA_REFILL_NODE_W >= n_leaf * (uint32_t)RAYCA_REFILL_LEAF_W && n_search != 0u) {
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF>(sc, ray, fr, limit, cur, stack, cnt);
    } else if (at_leaf) {
      test_leaf<true, SPH, STATS>(sc, ray, fr, cur, FLT_MAX, hit, limit, cnt);
      cur = stack.pop();
    }
#else
    // RAYCA_REFILL_SCHED 0: node phase until fewer than RAYCA_REFILL_LEAVE_K lanes are still searching (and some lane holds
    // a leaf), then the leaf phase for every lane that holds one
    for (;;) {
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)RAYCA_REFILL_LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF>(sc, ray, fr, limit, cur, stack, cnt);
    }
    if (cur & kLeafFlag) {
      test_leaf<true, SPH, STATS>(sc, ray, fr, cur, FLT_MAX, hit, limit, cnt);
      cur = stack.pop();
    }
#endif
  }
  if (STATS) {
    unsigned long long b = cnt.boxes, t = cnt.tris, sh = n_shaded, sb = cnt.slot_boxes, stt = cnt.slot_tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
      sh += __shfl_down(sh, off);
      sb += __shfl_down(sb, off);
      stt += __shfl_down(stt, off);
    }
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->shaded, sh);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}


// ---- queued rays (the wavefront engine's bounce generations) with lane refill ------------------------------------------
// The same persistent-lane scheme for the rays of an input queue: bounce rays start from scattered points in scattered
// directions, their searches differ in length far more than camera rays' do, and with one ray per lane for the lifetime of
// a wave (k_wf_trace) most lanes of a wave sit out most of its trips (measured on the atrium, 4 bounces: 0.47 of the lanes
// in the node loop, 0.23 in the leaf loop).  Here a lane that has finished its ray writes the hit record and takes the next
// queue entry.  Items are dealt in batches of 64 consecutive entries through the same per-XCD work counters; closest hits
// only (4-wide fp16 nodes, RAYCA_WF_BOUNCE_WIDE / _HALF, as k_wf_trace traverses them), every ray still takes its own
// steps in its own order: the hit records are the ones k_wf_trace writes.
// Measured (atrium 1080p, default 5-deep Config, four frames in flight, tests/gpu_ab_inflight.py; profiles/r02_ab_qrefill.log):
// k_wf_trace 4.995 ms per frame, this kernel with (threshold, K) = (44, 32) 4.792, (32, 16) 4.744, (48, 8) 4.736,
// (24, 8) 4.755, (56, 24) 4.786, (48, 48) 5.29; the 3840x2160 4-bounce frame 19.18 -> 18.18 ms; lanes active in the
// node loop over the whole frame 0.47 -> 0.56.
#ifndef RAYCA_QREFILL_THRESHOLD
#define RAYCA_QREFILL_THRESHOLD 48   // refill when at most this many lanes still hold a live ray
#endif
#ifndef RAYCA_QREFILL_LEAVE_K
#define RAYCA_QREFILL_LEAVE_K 8      // leave the node phase when fewer lanes than this are searching (and a lane holds a leaf)
#endif
#ifndef RAYCA_QREFILL_WAVES
#define RAYCA_QREFILL_WAVES RAYCA_REFILL_WAVES
#endif
// (This kernel and k_shadow_refill trace bounce and shadow rays only: their origins lie on the scene's surfaces, where the padding
// of the steering boxes covers the rounding of c -- trace_core.inc ray_needs_slack -- so their node steps carry no slack.
// SLACK: the queue holds rays a caller has supplied (generation 0 of rayca_hip_radiance_device), whose origins may lie anywhere:
// node steps and leaf tests with the slack, as k_query_refill takes them.)
template <bool SPH, bool STATS, bool SLACK = false>
__global__ __launch_bounds__(kBlock, RAYCA_QREFILL_WAVES) void k_queue_refill(DevScene sc, const QueuedRay* in_rays, const uint32_t* in_count, float4* hits,
                                                                              uint32_t* heads, TraceCounters* counters, TraceLaunch tl) {
  constexpr bool WIDE = RAYCA_WF_BOUNCE_WIDE != 0, SPILL = true, HALF = RAYCA_WF_BOUNCE_HALF != 0;   // (as k_wf_trace traverses bounce rays)
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  const uint32_t count = *in_count, n_batches = (count + 63u) >> 6;
  WorkCursor wc{};
  LaneCounters cnt{};
  bool has = false;
  uint32_t cur = kTerminated, item = 0;
  DRay ray{};
  FastRay fr{};
  DHit hit{};
  float limit = INFINITY;
  uint32_t pool_next = 0, pool_end = 0;
  bool dry = false;
  for (;;) {
    const uint32_t n_active = (uint32_t)__popcll(__ballot(cur != kTerminated));
    if (n_active <= (dry ? 0u : (uint32_t)RAYCA_QREFILL_THRESHOLD)) {
      if (has && cur == kTerminated) {  // retire: the hit record of this queue entry
        hits[item] = make_float4(hit.t, __uint_as_float(hit.prim), hit.u, hit.v);
        has = false;
      }
      if (dry && n_active == 0u) break;  // every lane reaches this: n_active and dry are wave-uniform
      while (!dry) {
        const unsigned long long idle = __ballot(!has);
        if (idle == 0ull) break;
        if (pool_next == pool_end) {
          const uint32_t batch = next_batch(heads, n_batches, home, wc, tl.ticket);
          if (batch == RAYCA_NONE) {
            dry = true;
            break;
          }
          pool_next = batch * 64u;
          pool_end = min(pool_next + 64u, count);
        }
        const uint32_t avail = pool_end - pool_next;
        const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
        if (!has && rank < avail) {
          item = pool_next + rank;
          const QueuedRay q = in_rays[item];
          ray = make_ray(point3(q.ox, q.oy, q.oz), vec3(q.dx, q.dy, q.dz));
          fr = make_fast(sc, ray, HALF);   // prologue of trace(): the root box first (blas.rs:136-139)
          hit.t = INFINITY;
          hit.prim = RAYCA_NONE;
          hit.u = hit.v = 0.0f;
          limit = INFINITY;
          stack.clear();
          float tmin;
          if (STATS) cnt.boxes++;
          cur = slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin) ? (WIDE ? sc.root_ref4 : (!HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref)) : kTerminated;
          has = true;
        }
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        pool_next += n_idle < avail ? n_idle : avail;
      }
    }
    for (;;) {  // (RAYCA_REFILL_SCHED 0 of k_flat_refill)
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)RAYCA_QREFILL_LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF, SLACK>(sc, ray, fr, limit, cur, stack, cnt);
    }
    if (cur & kLeafFlag) {
      test_leaf<true, SPH, STATS, SLACK>(sc, ray, fr, cur, FLT_MAX, hit, limit, cnt);
      cur = stack.pop();
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
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}


// The shadow-ray pass the same way (k_wf_shadow: a lane owns a pixel, traces its shadow rays in sample order and sums the
// direct light exactly like the NEE loop of k_generation).  A shadow ray ends at the first occluder, so the searches of a
// wave differ in length even more than closest-hit searches do; and the items that have no lit vertex never occupy a lane.
// A lane whose ray is done adds its sample, then takes the pixel's next shadow ray or -- after the last -- writes the sum and
// takes the next item.  Items: the tile list for generation 0, the input queue after; the other set of work counters
// (heads_b), since the closest-hit pass of the same generation has used the first.
template <bool GEN0, bool SPH, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_QREFILL_WAVES) void k_shadow_refill(DevScene sc, FrameParams fp, const QueuedRay* in_rays, const uint32_t* in_count, WfBuffers wb,
                                                                                PathBuffers pb, uint32_t depth, uint32_t* heads, TraceCounters* counters, TraceLaunch tl) {
  constexpr bool WIDE = RAYCA_WF_SHADOW_WIDE != 0, SPILL = true, HALF = RAYCA_WF_SHADOW_HALF != 0;   // (as k_wf_shadow traverses them)
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  const uint32_t count = GEN0 ? fp.tile_count * 64u : *in_count, n_batches = (count + 63u) >> 6;
  WorkCursor wc{};
  LaneCounters cnt{};
  bool has = false;          // the lane holds a pixel whose shadow rays are not all done
  uint32_t cur = kTerminated, p = 0, j = 0, quad = 0;
  float t_stop = FLT_MAX;
  Color direct = black();
  DRay ray{};
  FastRay fr{};
  DHit hit{};
  float limit = INFINITY;
  uint32_t pool_next = 0, pool_end = 0;
  bool dry = false;
  // the next shadow ray of pixel p that has to be traced, from the j-th on: prologue of trace() with the any-hit bound.  A sample
  // that k_wf_shade marked as unable to contribute is "not lit" without a traversal, which leaves the sum as it is
  // (nee_irrelevant, trace_core.inc).  After the pixel's last sample the sum is written and the lane is free for the next item.
  auto start_ray = [&]() {
    while (j < wb.nls && (__float_as_uint(wb.sh_ray[2 * ((size_t)j * pb.npix + p) + 1].w) & kShadowSkip)) ++j;
    if (j == wb.nls) {
      pb.direct[(size_t)depth * pb.npix + p] = as_f4(direct);
      has = false;
      cur = kTerminated;
      return;
    }
    const size_t e = (size_t)j * pb.npix + p;
    const float4 a = wb.sh_ray[2 * e], b = wb.sh_ray[2 * e + 1];
    quad = __float_as_uint(b.w) & kShadowQuad;
    t_stop = a.w;
    ray = make_ray(point3(a.x, a.y, a.z), vec3(b.x, b.y, b.z));
    fr = make_fast(sc, ray, HALF);
    hit.t = INFINITY;
    hit.prim = RAYCA_NONE;
    hit.u = hit.v = 0.0f;
    limit = t_stop < FLT_MAX ? cull_limit<false>(sc, fr, t_stop) : INFINITY;
    stack.clear();
    float tmin;
    if (STATS) cnt.boxes++;
    cur = slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin) ? (WIDE ? sc.root_ref4 : (!HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref)) : kTerminated;
  };
  for (;;) {
    const uint32_t n_active = (uint32_t)__popcll(__ballot(cur != kTerminated));
    if (n_active <= (dry ? 0u : (uint32_t)RAYCA_QREFILL_THRESHOLD)) {
      if (has && cur == kTerminated) {  // retire a shadow ray: k_wf_shadow's statements
        const bool found = hit.prim != RAYCA_NONE;
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
        const size_t e = (size_t)j * pb.npix + p;
        direct = direct + (lit ? as_color(wb.sh_x[e]) : black());
        ++j;
        start_ray();   // (or, after the last sample, the pixel's sum)
      }
      // (every lane reaches this: both operands are wave-uniform.  A lane that still holds a pixel -- its next ray started by
      // the retire above, or ended at the root box at once -- keeps the wave going; it retires on a later trip)
      if (dry && __ballot(has) == 0ull) break;
      while (!dry) {
        const unsigned long long idle = __ballot(!has);
        if (idle == 0ull) break;
        if (pool_next == pool_end) {
          const uint32_t batch = next_batch(heads, n_batches, home, wc, tl.ticket);
          if (batch == RAYCA_NONE) {
            dry = true;
            break;
          }
          pool_next = batch * 64u;
          pool_end = min(pool_next + 64u, count);
        }
        const uint32_t avail = pool_end - pool_next;
        const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
        if (!has && rank < avail) {
          const uint32_t item = pool_next + rank;
          uint32_t px = RAYCA_NONE;
          if (GEN0) {
            uint32_t x = 0, r = 0;
            if (tile_item_pixel(fp, item, x, r)) px = r * fp.width + x;
          } else {
            px = in_rays[item].pixel;
          }
          if (px != RAYCA_NONE) {  // (items without a lit vertex are skipped: the lane asks again)
            const uint32_t st = pb.state[(size_t)depth * pb.npix + px];
            if (st == kVertexLit || st == kVertexLitNoIndirect) {
              p = px;
              j = 0;
              direct = black();
              has = true;
              start_ray();
            }
          }
        }
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        pool_next += n_idle < avail ? n_idle : avail;
      }
    }
    for (;;) {
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)RAYCA_QREFILL_LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF, false>(sc, ray, fr, limit, cur, stack, cnt);
    }
    if (cur & kLeafFlag) {
      test_leaf<true, SPH, STATS, false>(sc, ray, fr, cur, t_stop, hit, limit, cnt);
      cur = (t_stop < FLT_MAX && hit.t < t_stop) ? kTerminated : stack.pop();   // any hit in front of the light ends the search (trace())
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
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}

// ---- caller-supplied rays (rayca_hip_query_device) with lane refill --------------------------------------------------------
// k_queue_refill's scheme for rays the caller keeps in device memory: batches of 64 consecutive rays dealt through the per-XCD
// work counters, a lane that retires its ray writes its outputs and takes the next one.  Differences: the 24-B rays and the
// optional per-ray bound are read where they lie; the cull bound starts at the ray's tmax (with trace()'s slack) instead of
// +inf; OCCLUDED ends a ray's search at its first hit in front of tmax (k_shadow_refill's statement, here also for an
// unbounded ray) and writes one byte.
// Exactness.  CLOSEST never ends a search early: tmax only seeds `limit`, and test_leaf keeps limit >= min(best t, tmax) +
// slack.  If the unbounded winner (t*, reference order) has t* < tmax, no box on its path is culled that the unbounded
// search would not cull with limit = t* + slack, and every candidate that ties with it has the same t*: the same record.
// Otherwise every hit the search can find has t >= t* >= tmax and query_found() reports the miss record.  OCCLUDED stops at
// an accepted hit with t < tmax, which implies t* <= t < tmax; without such a stop the search is CLOSEST's.
// (Threshold, leave-K) = k_queue_refill's measured pair, not retuned.
template <bool OCCLUDED, bool SPH, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_QREFILL_WAVES) void k_query_refill(DevScene sc, QueryIo q, uint32_t* heads, TraceCounters* counters, TraceLaunch tl) {
  constexpr bool WIDE = RAYCA_WF_BOUNCE_WIDE != 0, SPILL = true, HALF = RAYCA_WF_BOUNCE_HALF != 0;   // (as k_queue_refill)
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  const uint32_t count = q.count, n_batches = (count + 63u) >> 6;
  WorkCursor wc{};
  LaneCounters cnt{};
  bool has = false;
  uint32_t cur = kTerminated, item = 0;
  float t_stop = FLT_MAX;
  DRay ray{};
  FastRay fr{};
  DHit hit{};
  float limit = INFINITY;
  uint32_t pool_next = 0, pool_end = 0;
  bool dry = false;
  for (;;) {
    const uint32_t n_active = (uint32_t)__popcll(__ballot(cur != kTerminated));
    if (n_active <= (dry ? 0u : (uint32_t)RAYCA_QREFILL_THRESHOLD)) {
      if (has && cur == kTerminated) {  // retire: this ray's outputs (item < count: nothing else is ever written)
        query_store<OCCLUDED>(q, item, hit, query_found(hit, t_stop));
        has = false;
      }
      if (dry && n_active == 0u) break;  // every lane reaches this: n_active and dry are wave-uniform
      while (!dry) {
        const unsigned long long idle = __ballot(!has);
        if (idle == 0ull) break;
        if (pool_next == pool_end) {
          const uint32_t batch = next_batch(heads, n_batches, home, wc, tl.ticket);
          if (batch == RAYCA_NONE) {
            dry = true;
            break;
          }
          pool_next = batch * 64u;
          pool_end = min(pool_next + 64u, count);
        }
        const uint32_t avail = pool_end - pool_next;
        const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
        if (!has && rank < avail) {
          item = pool_next + rank;
          const float* r = q.rays + 6ull * item;
          ray = make_ray(point3(r[0], r[1], r[2]), vec3(r[3], r[4], r[5]));
          bool dead;
          t_stop = query_bound(q, item, dead);
          fr = make_fast(sc, ray, HALF);   // prologue of trace(): the root box first (blas.rs:136-139)
          hit.t = INFINITY;
          hit.prim = RAYCA_NONE;
          hit.u = hit.v = 0.0f;
          limit = t_stop < FLT_MAX ? cull_limit<true>(sc, fr, t_stop) : INFINITY;
          stack.clear();
          float tmin;
          if (STATS && !dead) cnt.boxes++;
          cur = !dead && slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin)
                    ? (WIDE ? sc.root_ref4 : (!HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref))
                    : kTerminated;
          has = true;
        }
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        pool_next += n_idle < avail ? n_idle : avail;
      }
    }
    for (;;) {  // (RAYCA_REFILL_SCHED 0 of k_flat_refill)
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)RAYCA_QREFILL_LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF>(sc, ray, fr, limit, cur, stack, cnt);
    }
    if (cur & kLeafFlag) {
      test_leaf<true, SPH, STATS>(sc, ray, fr, cur, t_stop, hit, limit, cnt);
      cur = (OCCLUDED && query_found(hit, t_stop)) ? kTerminated : stack.pop();
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
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}

// ---- hemisphere visibility at points (rayca_hip_ambient_device) with lane refill ----------------------------------------------
// k_query_refill<OCCLUDED>'s sibling, written beside it so that its listings stay what they were: the same work counters,
// threshold and leave-K, node_step / test_leaf, stack plan and persistent grid, on the same 4-wide fp16 nodes.  What differs is
// where a ray comes from and where its answer goes.  Item = i * S + j, sample j of point i: a lane that takes an item reads the
// point's 24 B (32 B with a rotation) and 12 B of the direction table and makes origin and direction in registers (ambient.inc
// ambient_ray) instead of reading a 24-B ray; a batch of 64 items is the full sample set of 64 / S neighbouring points, whose
// origins coincide and whose node fetches are shared.  A retiring lane whose ray was occluded ORs bit j into the point's mask
// word with one 64-bit atomic; an unoccluded lane writes nothing.  The items of an inactive point, or of one whose radius
// nothing can be in front of, retire at once -- they never hold a lane through a trip of the traversal.
template <bool ROT, bool SPH, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_QREFILL_WAVES) void k_ambient_refill(DevScene sc, AmbientIo a, uint32_t* heads, TraceCounters* counters, TraceLaunch tl) {
  constexpr bool WIDE = RAYCA_WF_BOUNCE_WIDE != 0, SPILL = true, HALF = RAYCA_WF_BOUNCE_HALF != 0;   // (as k_query_refill)
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  const uint32_t count = a.count * a.samples, n_batches = (count + 63u) >> 6;   // (the host refuses count x samples >= 2^32)
  WorkCursor wc{};
  LaneCounters cnt{};
  bool has = false;
  uint32_t cur = kTerminated, item = 0;
  float t_stop = FLT_MAX;
  DRay ray{};
  FastRay fr{};
  DHit hit{};
  float limit = INFINITY;
  uint32_t pool_next = 0, pool_end = 0;
  bool dry = false;
  for (;;) {
    const uint32_t n_active = (uint32_t)__popcll(__ballot(cur != kTerminated));
    if (n_active <= (dry ? 0u : (uint32_t)RAYCA_QREFILL_THRESHOLD)) {
      if (has && cur == kTerminated) {  // retire: bit j of point i, iff the ray was occluded (i < count: nothing else is ever written)
        if (query_found(hit, t_stop)) {
          const uint32_t i = item / a.samples, j = item - i * a.samples;
          atomicOr(&a.mask[i], 1ull << j);
        }
        has = false;
      }
      if (dry && n_active == 0u) break;  // every lane reaches this: n_active and dry are wave-uniform
      while (!dry) {
        const unsigned long long idle = __ballot(!has);
        if (idle == 0ull) break;
        if (pool_next == pool_end) {
          const uint32_t batch = next_batch(heads, n_batches, home, wc, tl.ticket);
          if (batch == RAYCA_NONE) {
            dry = true;
            break;
          }
          pool_next = batch * 64u;
          pool_end = min(pool_next + 64u, count);
        }
        const uint32_t avail = pool_end - pool_next;
        const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
        if (!has && rank < avail) {
          item = pool_next + rank;
          const uint32_t i = item / a.samples, j = item - i * a.samples;
          const AmbientPoint pt = ambient_point<ROT>(a, i);
          if (!pt.dead) {   // (a dead item is skipped: the lane asks again)
            const AmbientRay ar = ambient_ray<ROT>(pt.p, pt.n, pt.c, pt.s, a.dirs, j, a.bias);
            ray = make_ray(ar.o, ar.d);
            t_stop = pt.bound;
            fr = make_fast(sc, ray, HALF);   // prologue of trace(): the root box first (blas.rs:136-139)
            hit.t = INFINITY;
            hit.prim = RAYCA_NONE;
            hit.u = hit.v = 0.0f;
            limit = t_stop < FLT_MAX ? cull_limit<true>(sc, fr, t_stop) : INFINITY;
            stack.clear();
            float tmin;
            if (STATS) cnt.boxes++;
            cur = slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin)
                      ? (WIDE ? sc.root_ref4 : (!HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref))
                      : kTerminated;
            has = true;
          }
        }
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        pool_next += n_idle < avail ? n_idle : avail;
      }
    }
    for (;;) {  // (RAYCA_REFILL_SCHED 0 of k_flat_refill)
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)RAYCA_QREFILL_LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF>(sc, ray, fr, limit, cur, stack, cnt);
    }
    if (cur & kLeafFlag) {
      test_leaf<true, SPH, STATS>(sc, ray, fr, cur, t_stop, hit, limit, cnt);
      cur = query_found(hit, t_stop) ? kTerminated : stack.pop();
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
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}

// ---- probe visibility at points (rayca_hip_probe_lookup_device) with lane refill --------------------------------------------------
// k_ambient_refill's sibling, written beside it so that the existing listings stay what they are: the same work counters,
// threshold and leave-K, node_step / test_leaf, stack plan and persistent grid, on the same 4-wide fp16 nodes.  Item = i * 8 + k,
// corner k of point i's cell: a lane that takes an item reads the point's 24 B, computes cell and corner in registers (probes.inc)
// and makes the ray from the lifted point to the probe's centre, t_stop = 1; a batch of 64 items is the eight rays of eight
// neighbouring points, whose origins coincide per point.  An item whose corner is no candidate (no weight, or an invalid probe)
// and the items of an inactive point retire at once.  A retiring lane whose ray was occluded ORs bit 8 + k into the point's word.
template <bool SPH, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_QREFILL_WAVES) void k_probe_refill(DevScene sc, ProbeIo a, uint32_t* heads, TraceCounters* counters, TraceLaunch tl) {
  constexpr bool WIDE = RAYCA_WF_BOUNCE_WIDE != 0, SPILL = true, HALF = RAYCA_WF_BOUNCE_HALF != 0;   // (as k_query_refill)
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  const uint32_t count = a.count * 8u, n_batches = (count + 63u) >> 6;   // (the host refuses count x 8 >= 2^32)
  const bool kept = a.kept != nullptr;
  constexpr float t_stop = 1.0f;
  WorkCursor wc{};
  LaneCounters cnt{};
  bool has = false;
  uint32_t cur = kTerminated, item = 0;
  DRay ray{};
  FastRay fr{};
  DHit hit{};
  float limit = INFINITY;
  uint32_t pool_next = 0, pool_end = 0;
  bool dry = false;
  for (;;) {
    const uint32_t n_active = (uint32_t)__popcll(__ballot(cur != kTerminated));
    if (n_active <= (dry ? 0u : (uint32_t)RAYCA_QREFILL_THRESHOLD)) {
      if (has && cur == kTerminated) {  // retire: bit 8 + k of point i, iff the ray was occluded (i < count: nothing else is ever written)
        if (query_found(hit, t_stop)) atomicOr(&a.mask[item >> 3], 1u << (8u + (item & 7u)));
        has = false;
      }
      if (dry && n_active == 0u) break;  // every lane reaches this: n_active and dry are wave-uniform
      while (!dry) {
        const unsigned long long idle = __ballot(!has);
        if (idle == 0ull) break;
        if (pool_next == pool_end) {
          const uint32_t batch = next_batch(heads, n_batches, home, wc, tl.ticket);
          if (batch == RAYCA_NONE) {
            dry = true;
            break;
          }
          pool_next = batch * 64u;
          pool_end = min(pool_next + 64u, count);
        }
        const uint32_t avail = pool_end - pool_next;
        const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
        if (!has && rank < avail) {
          item = pool_next + rank;
          const ProbePoint pt = probe_point(a, item >> 3);
          if (pt.active) {   // (an item that traces nothing is skipped: the lane asks again)
            const ProbeCorner pc = probe_corner(a, probe_cell(a, pt.p), item & 7u, kept);
            if (pc.candidate) {
              const AmbientRay pr = probe_ray(pt, pc.c, a.bias);
              ray = make_ray(pr.o, pr.d);
              fr = make_fast(sc, ray, HALF);   // prologue of trace(): the root box first (blas.rs:136-139)
              hit.t = INFINITY;
              hit.prim = RAYCA_NONE;
              hit.u = hit.v = 0.0f;
              limit = cull_limit<true>(sc, fr, t_stop);
              stack.clear();
              float tmin;
              if (STATS) cnt.boxes++;
              cur = slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin)
                        ? (WIDE ? sc.root_ref4 : (!HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref))
                        : kTerminated;
              has = true;
            }
          }
        }
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        pool_next += n_idle < avail ? n_idle : avail;
      }
    }
    for (;;) {  // (RAYCA_REFILL_SCHED 0 of k_flat_refill)
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)RAYCA_QREFILL_LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF>(sc, ray, fr, limit, cur, stack, cnt);
    }
    if (cur & kLeafFlag) {
      test_leaf<true, SPH, STATS>(sc, ray, fr, cur, t_stop, hit, limit, cnt);
      cur = query_found(hit, t_stop) ? kTerminated : stack.pop();
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
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}

// ---- direct light at points (rayca_hip_direct_device) with lane refill ----------------------------------------------------------
// k_probe_refill's sibling, written beside it so that the existing listings stay what they are: the same work counters,
// threshold and leave-K, node_step / test_leaf, stack plan and persistent grid, on the same 4-wide fp16 nodes.  Item = i * N + j,
// sample j of point i: a lane that takes an item reads the point's 12 B (24 B with a normal) and the light's record and makes the
// sample in registers (direct.inc direct_sample); a batch of 64 items is the full sample set of 64 / N neighbouring points.  An
// item that traces nothing -- an inactive point, a dropped or an empty sample -- retires at once.  The search starts as
// k_shadow_refill::start_ray starts it: any-hit with the cull bound for a point light (t_stop = its distance), closest hit for a
// quad light (t_stop = FLT_MAX) -- with the slack of k_query_refill, since a caller's points lie anywhere.  A retiring lane whose
// sample was lit ORs bit j into the point's word with one 64-bit atomic; an unlit one writes nothing.
template <bool SPHERE, bool SPH, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_QREFILL_WAVES) void k_direct_refill(DevScene sc, DirectIo a, uint32_t* heads, TraceCounters* counters, TraceLaunch tl) {
  constexpr bool WIDE = RAYCA_WF_BOUNCE_WIDE != 0, SPILL = true, HALF = RAYCA_WF_BOUNCE_HALF != 0;   // (as k_query_refill)
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t lane = __lane_id();
  const uint32_t home = xcc_id();
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  const uint32_t count = a.count * a.samples, n_batches = (count + 63u) >> 6;   // (the host refuses count x samples >= 2^32)
  WorkCursor wc{};
  LaneCounters cnt{};
  uint32_t n_traced = 0;   // the wave's traced samples
  bool has = false;
  uint32_t cur = kTerminated, item = 0;
  float t_stop = FLT_MAX;
  DRay ray{};
  FastRay fr{};
  DHit hit{};
  float limit = INFINITY;
  uint32_t pool_next = 0, pool_end = 0;
  bool dry = false;
  for (;;) {
    const uint32_t n_active = (uint32_t)__popcll(__ballot(cur != kTerminated));
    if (n_active <= (dry ? 0u : (uint32_t)RAYCA_QREFILL_THRESHOLD)) {
      if (has && cur == kTerminated) {  // retire: bit j of point i, iff the sample was lit (i < count: nothing else is ever written)
        if (direct_lit(sc, hit, t_stop)) {
          const uint32_t i = item / a.samples, j = item - i * a.samples;
          atomicOr(&a.mask[i], 1ull << j);
        }
        has = false;
      }
      if (dry && n_active == 0u) break;  // every lane reaches this: n_active and dry are wave-uniform
      while (!dry) {
        const unsigned long long idle = __ballot(!has);
        if (idle == 0ull) break;
        if (pool_next == pool_end) {
          const uint32_t batch = next_batch(heads, n_batches, home, wc, tl.ticket);
          if (batch == RAYCA_NONE) {
            dry = true;
            break;
          }
          pool_next = batch * 64u;
          pool_end = min(pool_next + 64u, count);
        }
        const uint32_t avail = pool_end - pool_next;
        const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
        bool started = false;
        if (!has && rank < avail) {
          item = pool_next + rank;
          const uint32_t i = item / a.samples, j = item - i * a.samples;
          const DirectPoint pt = direct_point<SPHERE>(a, i);
          if (pt.active) {   // (an item that traces nothing is skipped: the lane asks again)
            const DirectSample s = direct_sample<SPHERE>(sc.lights, a, pt, i, j);
            if (!s.dropped && !s.empty) {
              ray = make_ray(s.o, s.omega);
              t_stop = s.t_stop;
              fr = make_fast(sc, ray, HALF);   // prologue of trace(): the root box first (blas.rs:136-139)
              hit.t = INFINITY;
              hit.prim = RAYCA_NONE;
              hit.u = hit.v = 0.0f;
              limit = t_stop < FLT_MAX ? cull_limit<true>(sc, fr, t_stop) : INFINITY;
              stack.clear();
              float tmin;
              if (STATS) cnt.boxes++;
              started = true;
              cur = slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin)
                        ? (WIDE ? sc.root_ref4 : (!HALF && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref))
                        : kTerminated;
              has = true;
            }
          }
        }
        n_traced += (uint32_t)__popcll(__ballot(started));   // (wave-uniform: a scalar, not a lane's register)
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        pool_next += n_idle < avail ? n_idle : avail;
      }
    }
    for (;;) {  // (RAYCA_REFILL_SCHED 0 of k_flat_refill)
      const bool searching = !(cur & kLeafFlag) && cur != kTerminated;
      const uint32_t n = (uint32_t)__popcll(__ballot(searching));
      if (n == 0u) break;
      if (n < (uint32_t)RAYCA_QREFILL_LEAVE_K && __ballot((cur & kLeafFlag) != 0u) != 0ull) break;
      if (searching) cur = node_step<true, true, WIDE, SPILL, STATS, HALF>(sc, ray, fr, limit, cur, stack, cnt);
    }
    if (cur & kLeafFlag) {
      test_leaf<true, SPH, STATS>(sc, ray, fr, cur, t_stop, hit, limit, cnt);
      cur = (t_stop < FLT_MAX && query_found(hit, t_stop)) ? kTerminated : stack.pop();   // a point light: any hit in front of it ends the search
    }
  }
  if (a.count_traced && lane == 0) atomicAdd(&counters->shadow, (unsigned long long)n_traced);
  if (STATS) {
    unsigned long long b = cnt.boxes, t = cnt.tris, sb = cnt.slot_boxes, stt = cnt.slot_tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
      sb += __shfl_down(sb, off);
      stt += __shfl_down(stt, off);
    }
    if (lane == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
      atomicAdd(&counters->box_slots, sb);
      atomicAdd(&counters->tri_slots, stt);
    }
  }
}

// The pickers: flags only, but for k_flat_refill, which reads WIDE, SPILL and HALF of a flavour -- of the six kTravFast* in
// production; the 4-wide forms always have the spill path, and the other flavours have no form of their own.
using QueryRefillKernel = void (*)(DevScene, QueryIo, uint32_t*, TraceCounters*, TraceLaunch);
QueryRefillKernel pick_query(bool occluded, bool sph, bool stats) {
  return with_flags([](auto OCCLUDED, auto SPH, auto STATS) -> QueryRefillKernel { return k_query_refill<OCCLUDED, SPH, STATS>; }, occluded, sph, stats);
}

using AmbientRefillKernel = void (*)(DevScene, AmbientIo, uint32_t*, TraceCounters*, TraceLaunch);
AmbientRefillKernel pick_ambient(bool rot, bool sph, bool stats) {
  return with_flags([](auto ROT, auto SPH, auto STATS) -> AmbientRefillKernel { return k_ambient_refill<ROT, SPH, STATS>; }, rot, sph, stats);
}

using ProbeRefillKernel = void (*)(DevScene, ProbeIo, uint32_t*, TraceCounters*, TraceLaunch);
ProbeRefillKernel pick_probe(bool sph, bool stats) {
  return with_flags([](auto SPH, auto STATS) -> ProbeRefillKernel { return k_probe_refill<SPH, STATS>; }, sph, stats);
}

using DirectRefillKernel = void (*)(DevScene, DirectIo, uint32_t*, TraceCounters*, TraceLaunch);
DirectRefillKernel pick_direct(bool sphere, bool sph, bool stats) {
  return with_flags([](auto SPHERE, auto SPH, auto STATS) -> DirectRefillKernel { return k_direct_refill<SPHERE, SPH, STATS>; }, sphere, sph, stats);
}

using ShadowRefillKernel = void (*)(DevScene, FrameParams, const QueuedRay*, const uint32_t*, WfBuffers, PathBuffers, uint32_t, uint32_t*, TraceCounters*, TraceLaunch);
ShadowRefillKernel pick_shadow(bool gen0, bool sph, bool stats) {
  return with_flags([](auto GEN0, auto SPH, auto STATS) -> ShadowRefillKernel { return k_shadow_refill<GEN0, SPH, STATS>; }, gen0, sph, stats);
}

using QueueRefillKernel = void (*)(DevScene, const QueuedRay*, const uint32_t*, float4*, uint32_t*, TraceCounters*, TraceLaunch);
QueueRefillKernel pick_queue(bool sph, bool stats, bool slack) {
  return with_flags([](auto SPH, auto STATS, auto SLACK) -> QueueRefillKernel { return k_queue_refill<SPH, STATS, SLACK>; }, sph, stats, slack);
}

using RefillKernel = void (*)(DevScene, FrameParams, uint32_t*, uint8_t*, float4*, TraceCounters*, TraceLaunch);
RefillKernel pick(const RefillFlavour& f) {
  return with_flavour([](auto T, auto SPH, auto STATS) -> RefillKernel { return k_flat_refill<SPH, T.WIDE, T.SPILL, STATS, T.HALF>; }, f.trav, f.sph, f.stats);
}

RAYCA_NO_PK_END
}  // namespace

const void* flat_refill_kernel(const RefillFlavour& f) { return reinterpret_cast<const void*>(pick(f)); }

void launch_flat_refill(const RefillFlavour& f, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const FrameParams& fp, uint32_t* heads,
                        uint8_t* rgba8, float4* rgba32f, TraceCounters* counters, const TraceLaunch& tl) {
  hipLaunchKernelGGL(pick(f), dim3(grid), dim3(kBlock), lds_bytes, stream, sc, fp, heads, rgba8, rgba32f, counters, tl);
}

const void* queue_refill_kernel(bool sph, bool stats, bool slack) { return reinterpret_cast<const void*>(pick_queue(sph, stats, slack)); }

void launch_queue_refill(bool sph, bool stats, bool slack, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const QueuedRay* in_rays,
                         const uint32_t* in_count, float4* hits, uint32_t* heads, TraceCounters* counters, const TraceLaunch& tl) {
  hipLaunchKernelGGL(pick_queue(sph, stats, slack), dim3(grid), dim3(kBlock), lds_bytes, stream, sc, in_rays, in_count, hits, heads, counters, tl);
}

const void* query_refill_kernel(bool occluded, bool sph, bool stats) {
  return reinterpret_cast<const void*>(pick_query(occluded, sph, stats));
}

void launch_query_refill(bool occluded, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const QueryIo& q,
                         uint32_t* heads, TraceCounters* counters, const TraceLaunch& tl) {
  hipLaunchKernelGGL(pick_query(occluded, sph, stats), dim3(grid), dim3(kBlock), lds_bytes, stream, sc, q, heads, counters, tl);
}

const void* ambient_refill_kernel(bool rot, bool sph, bool stats) {
  return reinterpret_cast<const void*>(pick_ambient(rot, sph, stats));
}

void launch_ambient_refill(bool rot, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const AmbientIo& a,
                           uint32_t* heads, TraceCounters* counters, const TraceLaunch& tl) {
  hipLaunchKernelGGL(pick_ambient(rot, sph, stats), dim3(grid), dim3(kBlock), lds_bytes, stream, sc, a, heads, counters, tl);
}

const void* probe_refill_kernel(bool sph, bool stats) {
  return reinterpret_cast<const void*>(pick_probe(sph, stats));
}

void launch_probe_refill(bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const ProbeIo& a, uint32_t* heads,
                         TraceCounters* counters, const TraceLaunch& tl) {
  hipLaunchKernelGGL(pick_probe(sph, stats), dim3(grid), dim3(kBlock), lds_bytes, stream, sc, a, heads, counters, tl);
}

const void* direct_refill_kernel(bool sphere, bool sph, bool stats) {
  return reinterpret_cast<const void*>(pick_direct(sphere, sph, stats));
}

void launch_direct_refill(bool sphere, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const DirectIo& a, uint32_t* heads,
                          TraceCounters* counters, const TraceLaunch& tl) {
  hipLaunchKernelGGL(pick_direct(sphere, sph, stats), dim3(grid), dim3(kBlock), lds_bytes, stream, sc, a, heads, counters, tl);
}

const void* shadow_refill_kernel(bool gen0, bool sph, bool stats) {
  return reinterpret_cast<const void*>(pick_shadow(gen0, sph, stats));
}

void launch_shadow_refill(bool gen0, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const FrameParams& fp,
                          const QueuedRay* in_rays, const uint32_t* in_count, const ShadowRefillArgs& a, uint32_t depth, uint32_t* heads,
                          TraceCounters* counters, const TraceLaunch& tl) {
  WfBuffers wb{};
  wb.sh_ray = a.sh_ray;
  wb.sh_x = a.sh_x;
  wb.nls = a.nls;
  PathBuffers pb{};
  pb.direct = a.direct;
  pb.state = a.state;
  pb.npix = a.npix;
  hipLaunchKernelGGL(pick_shadow(gen0, sph, stats), dim3(grid), dim3(kBlock), lds_bytes, stream, sc, fp, in_rays, in_count, wb,
                     pb, depth, heads, counters, tl);
}

}  // namespace rayca
