// select.inc -- how a launch gets its kernel and its plan (host code of kernels.hip, included from api.inc): the kernel pickers, the
// stack and traversal plans, the engine choice, the persistent grid, the environment knobs that steer them, and a self-test of the
// pickers that needs no device.  Reads RaycaScene, FrameCtx and the kernels; flavours and the flag dispatcher are flavour.hpp's.
#ifndef RAYCA_WF_LDS_ENTRIES
#define RAYCA_WF_LDS_ENTRIES 16u
#endif

struct LaunchPlan {
  int mode;          // kModeFlat / kModePath / kModeGeneral
  bool ordered, stats;
  bool wavefront;    // traversal split from shading (wavefront.inc) instead of the fused k_generation
  uint32_t generations;
};


// ---- the kernel pickers: run-time flags and a Trav into the template arguments of one kernel family (flavour.hpp) ------------------
// Each picker names only the template arguments its family is instantiated for; what it narrows is said in its comment.
// stats: the counting instantiation (RaycaRenderOptions.collect_stats); the counters cost registers in
// the traversal loop (measured: +15 % frame time on the depth-1 path kernel), so production launches
// use the instantiation without them

// k_generation: every flavour; Flat is generation 0, fused (the kernel writes the pixel) or not; Path has a last-vertex form
// (`last`: last_form below), which Flat does not read, and is fused only as generation 0 on that form without the counters
// (fuse_resolve below: the frame's only generation) -- every other Path tuple does not read `fused`
using GenKernel = void (*)(GenArgs);
GenKernel pick_kernel(int mode, bool gen0, bool fused, Trav t, bool sph, bool stats, bool last) {
  const bool flat = mode == kModeFlat;
  return with_flavour([](auto T, auto FLAT, auto A, auto SPH, auto STATS, auto LAST, auto PF) -> GenKernel {   // A: fused (Flat) / generation 0 (Path); PF: fused (Path)
    return k_generation<FLAT ? kModeFlat : kModePath, FLAT || A, T.ORDERED, (FLAT && A) || (!FLAT && A && LAST && !STATS && PF), T.FAST, SPH, T.WIDE, T.SPILL, STATS,
                        T.HALF, !FLAT && LAST>;
  }, t, flat, flat ? fused : gen0, sph, stats, last, !flat && fused);
}

// k_trace_rays: ignores HALF (caller-supplied rays traverse the f32 nodes): six distinct traversals
using TraceKernel = void (*)(DevScene, const float*, uint32_t, float*, uint32_t*, float*, TraceCounters*, TraceLaunch);
TraceKernel pick_trace_kernel(Trav t, bool sph, bool stats) {
  return with_flavour([](auto T, auto SPH, auto STATS) -> TraceKernel { return k_trace_rays<T.ORDERED, T.FAST, SPH, T.WIDE, T.SPILL, STATS>; }, t, sph, stats);
}

// k_query_rays (rayca_hip_query_device, one ray per lane: the flavours that entry falls back to, see there): ORDERED and FAST of the
// flavour on the binary f32 nodes with the spill path -- so only kTravExact, kTravExactAll and kTravFastAll have a form of their
// own -- and OCCLUDED only for the ordered forms (exhaustive: closest hits only)
using QueryKernel = void (*)(DevScene, QueryIo, TraceCounters*, TraceLaunch);
QueryKernel pick_query_kernel(Trav t, bool sph, bool stats, bool occluded) {
  return with_flavour([](auto T, auto SPH, auto STATS, auto OCCLUDED) -> QueryKernel {
    return k_query_rays<T.ORDERED, T.FAST, SPH, false, true, STATS, T.ORDERED && OCCLUDED>;
  }, t, sph, stats, occluded);
}

// ---- wavefront engine: one generation = k_wf_trace, k_wf_shade, k_wf_shadow (wavefront.inc) -------------------
using WfTraceKernel = void (*)(DevScene, FrameParams, const QueuedRay*, const uint32_t*, WfBuffers, TraceCounters*, TraceLaunch);
using WfShadowKernel = void (*)(DevScene, FrameParams, const QueuedRay*, const uint32_t*, WfBuffers, PathBuffers, uint32_t, TraceCounters*, TraceLaunch);
using WfShadeKernel = void (*)(DevScene, FrameParams, const QueuedRay*, const uint32_t*, QueuedRay*, uint32_t*, WfBuffers, PathBuffers, uint32_t, uint8_t*,
                               float4*, unsigned long long*);
// k_wf_trace, k_wf_shadow: FAST and SPILL of the flavour, on the node format they are compiled for: kTravFast, kTravFastSpill, kTravExact
WfTraceKernel pick_wf_trace(bool gen0, Trav t, bool sph, bool stats) {
  return with_flavour([](auto T, auto GEN0, auto SPH, auto STATS) -> WfTraceKernel { return k_wf_trace<GEN0, T.FAST, SPH, T.SPILL, STATS>; }, t, gen0, sph, stats);
}
WfShadowKernel pick_wf_shadow(bool gen0, Trav t, bool sph, bool stats) {
  return with_flavour([](auto T, auto GEN0, auto SPH, auto STATS) -> WfShadowKernel { return k_wf_shadow<GEN0, T.FAST, SPH, T.SPILL, STATS>; }, t, gen0, sph, stats);
}
// k_wf_shade: flags only.  Flat is generation 0, fused or not, and Path never fused, as k_generation.  rays: generation 0 of
// rayca_hip_radiance_device -- queue-fed, and a path's first vertex (k_wf_shade's RAYS); its Flat form finalises in place
WfShadeKernel pick_wf_shade(int mode, bool gen0, bool fused, bool sph, bool rays) {
  const bool flat = mode == kModeFlat;
  return with_flags([](auto FLAT, auto A, auto SPH, auto RAYS) -> WfShadeKernel {   // A: fused (Flat) / generation 0 (Path); not read with RAYS
    return k_wf_shade<FLAT ? kModeFlat : kModePath, !RAYS && (FLAT || A), FLAT && (RAYS || A), SPH, RAYS>;
  }, flat, flat ? fused : gen0, sph, rays);
}

// k_general (the per-pixel stack machine, general.inc): ordered, with the spill path; flags only
using GeneralKernel = void (*)(DevScene, FrameParams, uint32_t*, PathBuffers, GFrameStore, TraceCounters*, TraceLaunch);
GeneralKernel pick_general_kernel(bool fast, bool sph, bool stats) {
  return with_flags([](auto FAST, auto SPH, auto STATS) -> GeneralKernel { return k_general<true, FAST, SPH, true, STATS>; }, fast, sph, stats);
}

// k_surface (surface.inc): no traversal
using SurfaceKernel = void (*)(DevScene, SurfaceIo);
SurfaceKernel pick_surface_kernel(bool sph) {
  return with_flags([](auto SPH) -> SurfaceKernel { return k_surface<SPH>; }, sph);
}

// k_nearest (nearest.inc): flags only.  WITHIN ends at the first candidate that counts, so it has the culled form alone
using NearestKernel = void (*)(DevScene, NearestIo, TraceCounters*, TraceLaunch);
NearestKernel pick_nearest_kernel(bool within, bool cull, bool spill, bool stats) {
  return with_flags([](auto WITHIN, auto CULL, auto SPILL, auto STATS) -> NearestKernel { return k_nearest<WITHIN && CULL, CULL, SPILL, STATS>; }, within, cull, spill, stats);
}

// k_sample_surface (sample.inc): no traversal.  geom: point_out or normal_out is given, the drawn slot's record is read
using SampleKernel = void (*)(DevScene, SurfaceSampleIo);
SampleKernel pick_sample_kernel(bool geom) {
  return with_flags([](auto GEOM) -> SampleKernel { return k_sample_surface<GEOM>; }, geom);
}

// k_hits (hits.inc): ORDERED and FAST of the flavour on the binary f32 nodes with the spill path, as pick_query_kernel -- so
// kTravExact, kTravExactAll and kTravFastAll have a form of their own and every other flavour is kTravFastSpill's
using HitsKernel = void (*)(DevScene, HitsIo, TraceCounters*, TraceLaunch);
HitsKernel pick_hits_kernel(Trav t, bool sph, bool stats, bool both, bool count_all) {
  return with_flavour([](auto T, auto SPH, auto STATS, auto BOTH, auto COUNT_ALL) -> HitsKernel {
    return k_hits<T.ORDERED, T.FAST, SPH, STATS, BOTH, COUNT_ALL>;
  }, t, sph, stats, both, count_all);
}

// k_signed (signed.inc): flags only -- NEAR: a distance output is asked for (the nearest phase is compiled in), CULL: the ordered and
// culled searches, GRID: the points are made from a grid, FAST: the scene's reference-leaf filter; the rule and the number of
// directions are run-time values
using SignedKernel = void (*)(DevScene, SignedIo, TraceCounters*, TraceLaunch);
SignedKernel pick_signed_kernel(bool near, bool cull, bool grid, bool fast, bool stats) {
  return with_flags([](auto NEAR, auto CULL, auto GRID, auto FAST, auto STATS) -> SignedKernel { return k_signed<NEAR, CULL, GRID, FAST, STATS>; }, near, cull, grid, fast, stats);
}

// k_ambient_rays (ambient.inc, rayca_hip_ambient_device where k_ambient_refill of refill.hip cannot run): ordered, binary f32 nodes
// with the spill path, as pick_query_kernel's OCCLUDED forms -- so kTravFastSpill or kTravExact: the scene's FAST alone; flags only
using AmbientKernel = void (*)(DevScene, AmbientIo, TraceCounters*, TraceLaunch);
AmbientKernel pick_ambient_kernel(bool fast, bool sph, bool stats, bool rot) {
  return with_flags([](auto FAST, auto SPH, auto STATS, auto ROT) -> AmbientKernel { return k_ambient_rays<FAST, SPH, STATS, ROT>; }, fast, sph, stats, rot);
}
// k_ambient_finish: the fold without the direction loop reads no rotation
using AmbientFinishKernel = void (*)(AmbientIo);
AmbientFinishKernel pick_ambient_finish(bool bent, bool rot) {
  return with_flags([](auto BENT, auto ROT) -> AmbientFinishKernel { return k_ambient_finish<BENT, BENT && ROT>; }, bent, rot);
}

// k_enqueue_gather, k_gather_fold (gather.inc, rayca_hip_gather_device): flags only.  The fold makes directions only for sh_out, so
// without it the rotation is not read
using GatherEnqueueKernel = void (*)(GatherIo, uint32_t, uint32_t, QueuedRay*, uint32_t*);
GatherEnqueueKernel pick_gather_enqueue(bool rot) {
  return with_flags([](auto ROT) -> GatherEnqueueKernel { return k_enqueue_gather<ROT>; }, rot);
}
using GatherFoldKernel = void (*)(GatherIo);
GatherFoldKernel pick_gather_fold(bool sh, bool weights, bool rot) {
  return with_flags([](auto SH, auto WEIGHTS, auto ROT) -> GatherFoldKernel { return k_gather_fold<SH, WEIGHTS, SH && ROT>; }, sh, weights, rot);
}
// The rays of one internal frame of rayca_hip_gather_device (whole points; a point of 64 samples always fits): 2^22 rays are 128 MiB
// of queue entries and 64 MiB of radiance records, and enough work for every CU at any depth.
constexpr uint32_t kGatherFrameRays = 1u << 22;

// k_probe_rays (probes.inc, rayca_hip_probe_lookup_device where k_probe_refill of refill.hip cannot run): as pick_ambient_kernel
using ProbeKernel = void (*)(DevScene, ProbeIo, TraceCounters*, TraceLaunch);
ProbeKernel pick_probe_kernel(bool fast, bool sph, bool stats) {
  return with_flags([](auto FAST, auto SPH, auto STATS) -> ProbeKernel { return k_probe_rays<FAST, SPH, STATS>; }, fast, sph, stats);
}
// k_probe_fold: the call's two flags, and whether it has a kept array
using ProbeFoldKernel = void (*)(ProbeIo);
ProbeFoldKernel pick_probe_fold(bool vis, bool normal, bool kept) {
  return with_flags([](auto VIS, auto NORMAL, auto KEPT) -> ProbeFoldKernel { return k_probe_fold<VIS, NORMAL, KEPT>; }, vis, normal, kept);
}

// k_direct_rays (direct.inc, rayca_hip_direct_device where k_direct_refill of refill.hip cannot run): as pick_ambient_kernel;
// sphere: the call has no normals
using DirectKernel = void (*)(DevScene, DirectIo, TraceCounters*, TraceLaunch);
DirectKernel pick_direct_kernel(bool sphere, bool fast, bool sph, bool stats) {
  return with_flags([](auto SPHERE, auto FAST, auto SPH, auto STATS) -> DirectKernel { return k_direct_rays<SPHERE, FAST, SPH, STATS>; }, sphere, fast, sph, stats);
}
// k_direct_fold: the call's mode, and whether it has sh_out (sphere mode only: the host refuses sh_out with normals)
using DirectFoldKernel = void (*)(const DevLight*, DirectIo);
DirectFoldKernel pick_direct_fold(bool sphere, bool sh) {
  return with_flags([](auto SPHERE, auto SH) -> DirectFoldKernel { return k_direct_fold<SPHERE, SPHERE && SH>; }, sphere, sh);
}

// LDS part of the node stack: enough for the whole tree if that fits 24 entries (24 KiB per block),
// else 24 entries + a global spill area for the rest
#ifndef RAYCA_MAX_LDS_ENTRIES
#define RAYCA_MAX_LDS_ENTRIES 24
#endif
constexpr uint32_t kMaxLdsEntries = RAYCA_MAX_LDS_ENTRIES;
struct StackPlan {
  uint32_t lds_entries, spill_entries;
  size_t lds_bytes;
};
StackPlan plan_stack(uint32_t need, uint32_t max_entries = kMaxLdsEntries) {
  StackPlan p;
  const uint32_t want = need + 1u;
  p.lds_entries = want < max_entries ? ((want + 3u) / 4u) * 4u : max_entries;
  if (p.lds_entries == 0) p.lds_entries = 4;
  p.spill_entries = want > p.lds_entries ? want - p.lds_entries : 0u;
  p.lds_bytes = (size_t)p.lds_entries * kBlock * 4u;
  return p;
}
// A launch's node stack: the LDS part, and the spill area (a column per thread of the grid: entry e of thread t at
// ovf[e * ovf_stride + t]) when the plan needs one.  `block_threads`: the workgroup the kernel is launched with (StackPlan.lds_bytes
// is a 256-thread block's: fused_generation scales it for k_generation).  The context's one spill area grows to the largest launch.
int32_t bind_stack(FrameCtx* c, const StackPlan& sp, uint32_t grid, TraceLaunch& tl, uint32_t block_threads = kBlock) {
  tl = TraceLaunch{};
  tl.lds_entries = sp.lds_entries;
  if (sp.spill_entries) {
    tl.ovf_stride = grid * block_threads;
    const int32_t rc = grow_behind_pass(c, c->stack_spill, (size_t)sp.spill_entries * tl.ovf_stride * 4u);
    if (rc != RAYCA_OK) return rc;
    tl.ovf = static_cast<uint32_t*>(c->stack_spill.ptr);
  }
  return RAYCA_OK;
}

// The dynamic LDS of a k_hits launch: the node stack's rows, then the list's -- k rows of t and k rows of slots, kBlock words each
// (k <= RAYCA_HITS_MAX: at most 24 + 32 rows, 56 KiB)
size_t hits_lds_bytes(const StackPlan& sp, uint32_t k) { return sp.lds_bytes + (size_t)2u * k * kBlock * sizeof(uint32_t); }

// ---- the environment knobs that steer selection and planning: read once, at the first call that needs any of them --------------
// A path frame's LDS rows by the waves per SIMD its kernel is compiled for (trace_core.inc path_waves): at five, with the compact
// parked context, four rows -- 7 680 B per wave, twenty waves per CU; at four, twelve -- 9 728 B (10 KiB with seven quads), sixteen
// waves, the rows cost no wave there and four rows alone cost 1 % (DESIGN 4.1, r8).  RAYCA_PATH_LDS_ENTRIES in the environment
// replaces both.
#ifndef RAYCA_PATH_LDS_ENTRIES
#define RAYCA_PATH_LDS_ENTRIES (RAYCA_CTX_COMPACT ? 4 : 12)
#endif
#ifndef RAYCA_PATH_LDS_ENTRIES_FOUR_WAVES
#define RAYCA_PATH_LDS_ENTRIES_FOUR_WAVES 12
#endif
struct Knobs {
  int format;                 // RAYCA_NODE_FORMAT=0..3: the node format of every generation, bit 0 = 4-wide, bit 1 = fp16 boxes (RAYCA_WIDE=0/1: the older spelling, f32 formats); -1 = the scene times them
  int wavefront;              // RAYCA_WAVEFRONT=0/1: the engine RAYCA_ENGINE_AUTO takes; negative (unset: -1) = by the number of generations
  bool wf_refill;             // RAYCA_WF_REFILL=0: bounce generations' closest hits one ray per lane (k_wf_trace), not on k_queue_refill
  int wf_shadow_refill;       // RAYCA_WF_SHADOW_REFILL: shadow rays on k_shadow_refill 0 = never, 1 = bounce generations (default), 2 = every generation
  int refill;                 // RAYCA_REFILL=0/1: Flat camera rays on k_generation / k_flat_refill; -1 = the scene times them
  uint32_t grid_mult;         // RAYCA_GRID_MULT: blocks per CU of the fused engine's persistent grids (experiments); 0 = what the kernel admits
  uint32_t ticket;            // RAYCA_TICKET: batches per work ticket of the fused engine; 0 = by the size of the frame
  uint32_t path_lds_entries;  // RAYCA_PATH_LDS_ENTRIES: LDS part of a path frame's node stack, clamped to 4..kMaxLdsEntries; 0 = by the kernel's waves
  bool last_form;             // RAYCA_LAST_FORM=0: every generation of a path frame on k_generation's general form (A/B runs and tests); implies fuse_resolve off
  bool fuse_resolve;          // RAYCA_FUSE_RESOLVE=0: the one-sample depth-1 path frame stays generation + k_resolve, two launches (A/B runs and tests)
};
const Knobs& knobs() {
  static const Knobs k = [] {
    const auto env = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    Knobs n{};
    n.format = getenv("RAYCA_NODE_FORMAT") ? env("RAYCA_NODE_FORMAT", 0) & 3 : (getenv("RAYCA_WIDE") ? (env("RAYCA_WIDE", 0) ? 1 : 0) : -1);
    n.wavefront = env("RAYCA_WAVEFRONT", -1);
    n.wf_refill = env("RAYCA_WF_REFILL", 1) != 0;
    n.wf_shadow_refill = env("RAYCA_WF_SHADOW_REFILL", 1);
    n.refill = getenv("RAYCA_REFILL") ? (env("RAYCA_REFILL", 0) != 0 ? 1 : 0) : -1;
    n.grid_mult = (uint32_t)env("RAYCA_GRID_MULT", 0);
    n.ticket = (uint32_t)env("RAYCA_TICKET", 0);
    n.path_lds_entries = getenv("RAYCA_PATH_LDS_ENTRIES") ? std::min(std::max((uint32_t)env("RAYCA_PATH_LDS_ENTRIES", 0), 4u), kMaxLdsEntries) : 0u;
    n.last_form = env("RAYCA_LAST_FORM", 1) != 0;
    n.fuse_resolve = n.last_form && env("RAYCA_FUSE_RESOLVE", 1) != 0;
    return n;
  }();
  return k;
}

// Which node format a generation traverses.  Measured on MI355X (atrium, 1080p, A/B in one run):
// coherent camera/shadow rays are VALU-bound and the binary tree wins (0.37 vs 0.43 ms for the primary
// generation: the 4-wide node tests more boxes and sorts), incoherent bounce rays are latency-bound
// and the 4-wide tree wins (-9 % on the 4-bounce frame).
// Knobs.format pins the format of every generation instead of letting the scene time them: for profiling sessions,
// where counter collection perturbs the timing.
int format_forced() { return knobs().format; }
int wide_forced() {
  const int f = format_forced();
  return f < 0 ? -1 : (f & 1);
}
bool use_wide(uint32_t generation) {
  const int forced = wide_forced();
  return forced >= 0 ? forced != 0 : generation > 0;
}
uint32_t path_lds_entries(int waves_per_simd) {
  if (const uint32_t forced = knobs().path_lds_entries) return forced;
  return std::min(std::max((uint32_t)(waves_per_simd >= 5 ? RAYCA_PATH_LDS_ENTRIES : RAYCA_PATH_LDS_ENTRIES_FOUR_WAVES), 4u), kMaxLdsEntries);
}

// Does generation g of a frame run k_generation's last-vertex form (LAST, kernels.hip)?  Exactly when the test of the kernel's tail,
// `depth < limit`, is false for every vertex of the generation: a path frame's generations from `limit` on.  Under NEE that is the
// frame's last generation (max_depth 1: generation 0, the bench frame); with direct_sampler NONE the limit is max_depth and no
// generation of a frame reaches it.  last_form_rule is the arithmetic alone (rayca_hip_selftest checks it), last_form adds the knob.
bool last_form_rule(int mode, uint32_t direct_sampler, uint32_t max_depth, uint32_t g) {
  const uint32_t limit = direct_sampler != RAYCA_SAMPLER_NONE ? (max_depth ? max_depth - 1u : 0u) : max_depth;
  return mode == kModePath && g >= limit;
}
bool last_form(int mode, const RaycaConfig& c, uint32_t g) { return knobs().last_form && last_form_rule(mode, c.direct_sampler, c.max_depth, g); }

// Does a path frame's generation kernel write the pixel itself (k_generation's FUSED with GEN0 && LAST, kernels.hip), with no record
// and no k_resolve?  A camera frame of the fused engine with one sample per pixel and one generation, that generation on the
// last-vertex form, and not a counting frame: every lane's path then ends inside the one launch, and k_resolve would only read each
// record once.  Counting frames keep the two launches (their instantiation is the one with the counters), and so do caller-supplied
// rays, more samples, deeper paths, paths without a direct sampler, and the other engines.  fuse_resolve_rule is the arithmetic alone
// (rayca_hip_selftest checks it), fuse_resolve adds the knobs.
bool fuse_resolve_rule(int mode, bool wavefront, bool caller_rays, bool stats, uint32_t spp, uint32_t generations, uint32_t direct_sampler, uint32_t max_depth) {
  return mode == kModePath && !wavefront && !caller_rays && !stats && spp == 1u && generations == 1u && last_form_rule(mode, direct_sampler, max_depth, 0u);
}
bool fuse_resolve(const LaunchPlan& plan, const RaycaConfig& c, bool caller_rays) {
  return knobs().fuse_resolve && knobs().last_form &&
         fuse_resolve_rule(plan.mode, plan.wavefront, caller_rays, plan.stats, c.samples_per_pixel, plan.generations, c.direct_sampler, c.max_depth);
}

// What plan_traversal reads of a scene.
struct TreeFacts {
  bool fast;               // the reference-leaf filter is present (RAYCA_BUILDER_SAH)
  bool formats;            // the 4-wide and fp16 node arrays are there (formats_ready) ...
  bool half_nodes;         // ... the fp16 ones among them
  uint32_t depth, depth4;  // stack need of the binary and of the 4-wide tree
};
// flavour for one launch + its stack plan (the flavour's traits say whether it walks the 4-wide tree or the fp16 nodes)
struct TravPlan {
  Trav trav;
  StackPlan stack;
};
// format_choice: -1 = default, else bit 0 = 4-wide nodes, bit 1 = fp16 nodes
TravPlan plan_traversal(const TreeFacts& tf, bool ordered, uint32_t generation, int format_choice, uint32_t max_lds_entries) {
  TravPlan tp{};
  const bool fast = tf.fast;
  const bool wide = ordered && fast && tf.formats && (format_choice >= 0 ? (format_choice & 1) != 0 : use_wide(generation));
  const bool half = ordered && fast && format_choice >= 0 && (format_choice & 2) != 0 && tf.formats && tf.half_nodes;
  tp.stack = plan_stack(wide ? tf.depth4 : tf.depth, max_lds_entries);  // (also decides between the kernels with and without the spill path)
  if (!ordered) tp.trav = fast ? kTravFastAll : kTravExactAll;
  else if (!fast) tp.trav = kTravExact;
  else if (wide) tp.trav = half ? kTravFastWideHalf : kTravFastWide;
  else if (tp.stack.spill_entries) tp.trav = half ? kTravFastSpillHalf : kTravFastSpill;
  else tp.trav = half ? kTravFastHalf : kTravFast;
  return tp;
}
TravPlan plan_traversal(const RaycaScene* s, bool ordered, uint32_t generation, int format_choice = -1, uint32_t max_lds_entries = kMaxLdsEntries) {
  const bool formats = formats_ready(s);
  const TreeFacts tf{s->dev.ref_leaf_of != nullptr, formats, formats && s->dev_full.nodes_h != nullptr, s->host.max_depth, s->host.max_depth4};
  return plan_traversal(tf, ordered, generation, format_choice, max_lds_entries);
}

// RAYCA_ENGINE_AUTO: which of the two generation-by-generation engines.  Measured with two frames in flight at 1080p
// (tests/gpu_engine_depth_probe.py), fused vs wavefront: atrium depth 1 0.449 vs 0.567 ms, depth 2 1.80 vs 1.88,
// depth 3 4.06 vs 3.23, depth 4 6.24 vs 4.54, depth 5 8.42 vs 5.86; Cornell 0.186 vs 0.118 ... 2.21 vs 1.27: the lean
// trace kernels win once incoherent bounce generations dominate.  So: wavefront from three generations up.
// Knobs.wavefront overrides.
bool wavefront_by_default(uint32_t generations) {
  const int forced = knobs().wavefront;
  if (forced >= 0) return forced != 0;
  return generations >= 3u;
}

// Can the generation kernels (k_generation + k_resolve) render this Config?  They cover Flat and the
// Pathtracer with Nee/None direct and Cosine/Hemisphere indirect sampling, one indirect sample per vertex
// and no roulette; everything else runs on the per-pixel stack machine (k_general).
// The two halves of that question: the field of the Config that takes it off the generation kernels (nullptr: none does), which
// needs no scene, and the one thing the scene adds.
const char* generation_kernels_gap(const RaycaConfig& c) {
  if (c.integrator == RAYCA_INTEGRATOR_FLAT) return nullptr;
  if (c.integrator != RAYCA_INTEGRATOR_PATHTRACER) return "integrator";
  if (c.russian_roulette) return "russian_roulette";
  if (c.direct_sampler != RAYCA_SAMPLER_NONE && c.direct_sampler != RAYCA_SAMPLER_NEE) return "direct_sampler";
  const uint32_t limit = c.direct_sampler != RAYCA_SAMPLER_NONE ? (c.max_depth ? c.max_depth - 1u : 0u) : c.max_depth;
  const bool bounces = limit > 0 && c.max_depth > 0;
  if (bounces) {
    if (c.indirect_sampler != RAYCA_SAMPLER_COSINE && c.indirect_sampler != RAYCA_SAMPLER_HEMISPHERE) return "indirect_sampler";
    if (c.light_samples != 1) return "light_samples";
  }
  return nullptr;
}
bool nee_meets_directional_light(const RaycaScene* s, const RaycaConfig& c) {
  if (c.integrator == RAYCA_INTEGRATOR_PATHTRACER && c.direct_sampler == RAYCA_SAMPLER_NEE)
    for (const HostLight& l : s->host.lights)
      if (l.kind == RAYCA_LIGHT_DIRECTIONAL) return true;  // todo!() in the reference (nee.rs:178): k_general reports it
  return false;
}
bool generation_kernels_cover(const RaycaScene* s, const RaycaConfig& c) {
  return generation_kernels_gap(c) == nullptr && !nee_meets_directional_light(s, c);
}

// A scene with nothing in it: what every call that traverses it or reads its tables answers.
int32_t refuse_empty_scene(const RaycaScene* s) {
  if (s->host.blas.empty() || s->prim_count == 0) return fail(RAYCA_ERR_EMPTY_SCENE, "empty TLAS (tlas.rs:272)");
  return RAYCA_OK;
}

int32_t validate_config(const RaycaScene* s, const RaycaConfig& c, uint32_t engine, LaunchPlan& plan) {
  if (c.samples_per_pixel == 0 || c.light_samples == 0) return fail(RAYCA_ERR_BAD_ARG, "samples_per_pixel and light_samples must be > 0");
  if (c.integrator > RAYCA_INTEGRATOR_PATHTRACER) return fail(RAYCA_ERR_BAD_ARG, "unknown integrator");
  if (c.direct_sampler > RAYCA_SAMPLER_MIS || c.indirect_sampler > RAYCA_SAMPLER_MIS) return fail(RAYCA_ERR_BAD_ARG, "unknown sampler");
  if (engine > RAYCA_ENGINE_FUSED) return fail(RAYCA_ERR_BAD_ARG, "unknown engine");
  const uint32_t generations_if_path = c.integrator == RAYCA_INTEGRATOR_PATHTRACER ? c.max_depth : 1u;
  plan.wavefront = plan.ordered && (engine == RAYCA_ENGINE_WAVEFRONT || (engine == RAYCA_ENGINE_AUTO && wavefront_by_default(generations_if_path)));
  if (c.integrator == RAYCA_INTEGRATOR_FLAT) {
    plan.mode = kModeFlat;
    plan.generations = 1;
    return RAYCA_OK;
  }
  if (engine == RAYCA_ENGINE_GENERAL || !generation_kernels_cover(s, c)) {
    if (!plan.ordered) return fail(RAYCA_ERR_UNSUPPORTED, "exhaustive traversal is only offered with the generation kernels");
    plan.mode = kModeGeneral;
    plan.generations = 1;
    return RAYCA_OK;
  }
  plan.mode = kModePath;
  plan.generations = c.max_depth;  // generation g traces depth g; depth >= max_depth returns None
  return RAYCA_OK;
}

// VGPRs of a kernel (hipFuncGetAttributes costs microseconds per call: looked up once per kernel)
int32_t kernel_registers(const void* k, uint32_t& regs) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, uint32_t>> cache;
  std::lock_guard<std::mutex> lock(mu);
  for (const auto& e : cache)
    if (e.first == k) { regs = e.second; return RAYCA_OK; }
  hipFuncAttributes fa{};
  HIP_TRY(hipFuncGetAttributes(&fa, k));
  regs = fa.numRegs > 0 ? (uint32_t)fa.numRegs : 128u;
  cache.emplace_back(k, regs);
  return RAYCA_OK;
}

// Grid of a persistent kernel, whose waves take batches (64 rays or one 8x8 tile) off a work counter until none are
// left.  Persistent waves need no co-residency (there are no inter-block waits), so the grid only has to fill every CU.
// The policy counts in units of four waves, one per SIMD -- a 256-thread block: units per CU = what registers and LDS admit
// (512 VGPRs per lane per SIMD, allocated in granules of 8; 160 KiB of LDS per CU), and no more waves than there are batches.
// `block_waves` (1, 2 or 4) is the workgroup the kernel is launched with: `lds_bytes` is one workgroup's, and the grid comes
// out in workgroups -- the same waves per CU whatever the workgroup (k_generation: kGenWaves; every other kernel: 4).
// `per_cu_forced` != 0 replaces the units per CU (RAYCA_GRID_MULT, for experiments).
// `capped`: at most 8 units per CU, and fewer with frames in flight (the stack machine goes without both).  A frame
// that takes every wave slot of the chip keeps the next frame's waves out until its own retire; with fewer slots per
// frame the waves of two frames are resident side by side and one frame's slow tiles run under the other's work
// (DESIGN.md, "the frames leave each other room"; tests/gpu_inflight_probe.py with RAYCA_GRID_MULT).
// grid_policy is the arithmetic alone (no device: rayca_hip_selftest checks it), persistent_grid looks the registers up.
uint32_t grid_policy(uint32_t regs, size_t lds_bytes, uint32_t batches, bool capped, uint32_t in_flight, uint32_t per_cu_forced, uint32_t cu_count,
                     uint32_t block_waves) {
  const uint32_t blocks_per_unit = 4u / block_waves;
  uint32_t per_cu = per_cu_forced;
  if (per_cu == 0) {
    const size_t unit_lds = lds_bytes * blocks_per_unit;
    per_cu = std::min(512u / (((regs + 7u) / 8u) * 8u), unit_lds ? (uint32_t)((160u * 1024u) / unit_lds) : 8u);
    if (capped) {
      per_cu = std::max(1u, std::min(per_cu, 8u));
      if (in_flight >= 4u) per_cu = (per_cu + 1u) / 2u;
      else if (in_flight >= 2u) per_cu = (per_cu * 3u + 3u) / 4u;
    }
    per_cu = std::max(1u, per_cu);
  }
  const uint32_t need = (batches + block_waves - 1u) / block_waves;
  return std::min(cu_count * per_cu * blocks_per_unit, need ? need : 1u);
}
int32_t persistent_grid(const RaycaScene* s, const void* kernel, size_t lds_bytes, uint32_t batches, bool capped, uint32_t in_flight,
                        uint32_t per_cu_forced, uint32_t& grid, uint32_t block_waves = 4u) {
  uint32_t regs = 0;
  if (per_cu_forced == 0) {
    const int32_t rc = kernel_registers(kernel, regs);
    if (rc != RAYCA_OK) return rc;
  }
  grid = grid_policy(regs, lds_bytes, batches, capped, in_flight, per_cu_forced, (uint32_t)s->cu_count, block_waves);
  return RAYCA_OK;
}
// work tickets (next_batch) of the fused engine: pairs of batches while every wave still gets four batches or more, single
// batches for small frames
uint32_t ticket_policy(uint32_t batches, uint32_t grid, uint32_t block_waves) { return batches >= 4u * block_waves * grid ? 2u : 1u; }

// Self-test of grid_policy and ticket_policy (rayca_hip_selftest; no device): worked examples on a 256-CU chip, and for every
// tuple of a sweep that the grid is the same number of waves whatever the workgroup, and never more waves than batches ask for.
int32_t selftest_grid_policy(std::string& err) {
  struct Case { uint32_t regs; size_t wave_lds; uint32_t batches; bool capped; uint32_t in_flight, forced, waves; const char* what; };
  constexpr uint32_t kCus = 256u, kPathLds = 4u * 256u + 104u * 64u;   // per wave: 4 stack rows + the parked context = 7 680 B (fused_generation)
  const Case cases[] = {
      {96u, kPathLds, 32400u, true, 4u, 0u, 3072u, "the 1080p path frame, four in flight: 12 waves per CU"},
      {96u, kPathLds, 32400u, true, 2u, 0u, 4096u, "the 1080p path frame, two in flight: 16 waves per CU"},
      {96u, kPathLds, 32400u, true, 1u, 0u, 5120u, "the 1080p path frame alone: 20 waves per CU, by its 96 registers and by its LDS"},
      {64u, kPathLds, 32400u, false, 1u, 0u, 5120u, "its LDS alone admits 20 waves per CU (21 in single waves: counted in units of four)"},
      {120u, 12u * 256u + 104u * 64u, 32400u, true, 1u, 0u, 4096u, "a counting or sphere path frame, four waves per SIMD and twelve rows, 9 728 B: 16 waves per CU"},
      {112u, 12u * 256u + 7u * 1024u, 32400u, true, 4u, 0u, 2048u, "the path frame with seven quads, twelve rows and 112 registers, four in flight: 8 waves per CU"},
      {112u, 12u * 256u + 7u * 1024u, 32400u, true, 1u, 0u, 4096u, "the same alone: 16 waves per CU"},
      {96u, 24u * 256u, 32400u, true, 1u, 0u, 5120u, "a Flat frame at 96 VGPRs: registers admit 5 waves per SIMD, LDS 6"},
      {64u, 0u, 32400u, false, 1u, 0u, 8192u, "no LDS, uncapped: 8 waves per SIMD"},
      {40u, 256u, 1u << 20, false, 1u, 0u, 12288u, "uncapped at 40 VGPRs and a little LDS: 12 waves per SIMD"},
      {40u, 256u, 1u << 20, true, 1u, 0u, 8192u, "the same, capped: 8"},
      {96u, kPathLds, 32400u, true, 4u, 2u, 2048u, "RAYCA_GRID_MULT=2 replaces the policy"},
      {256u, 96u * 1024u, 32400u, true, 4u, 0u, 1024u, "a kernel nothing admits still gets one wave per SIMD"},
  };
  const auto fail_case = [&](const std::string& what) { err = "grid_policy: " + what; return RAYCA_ERR_BAD_ARG; };
  for (const Case& c : cases)
    for (uint32_t w : {1u, 2u, 4u}) {
      const uint32_t grid = grid_policy(c.regs, c.wave_lds * w, c.batches, c.capped, c.in_flight, c.forced, kCus, w);
      if (grid * w != c.waves) return fail_case(std::string(c.what) + ": " + std::to_string(grid) + " workgroups of " + std::to_string(w) + " waves, expected " + std::to_string(c.waves) + " waves");
    }
  // frames with fewer tiles than waves: one workgroup per `w` batches, rounded up; an empty frame still launches one
  const uint32_t small[][4] = {{0u, 1u, 1u, 1u}, {1u, 1u, 1u, 1u}, {6u, 6u, 3u, 2u}, {42u, 42u, 21u, 11u}, {2047u, 2047u, 1024u, 512u}};   // batches; grid at 1, 2, 4 waves
  for (const auto& r : small)
    for (uint32_t i = 0; i < 3u; ++i)
      if (const uint32_t grid = grid_policy(96u, kPathLds << i, r[0], true, 4u, 0u, kCus, 1u << i); grid != r[1 + i])
        return fail_case(std::to_string(r[0]) + " batches in workgroups of " + std::to_string(1u << i) + " waves: " + std::to_string(grid) + " workgroups, expected " + std::to_string(r[1 + i]));
  for (uint32_t regs : {24u, 64u, 96u, 125u, 128u, 200u})
    for (uint32_t wave_lds : {0u, 1024u, 6144u, 10240u, 16384u})
      for (uint32_t batches : {0u, 1u, 5u, 700u, 32400u, 129600u})
        for (uint32_t in_flight : {1u, 2u, 3u, 4u, 8u})
          for (int capped = 0; capped < 2; ++capped) {
            const uint32_t w4 = grid_policy(regs, (size_t)wave_lds * 4u, 1u << 30, capped != 0, in_flight, 0u, kCus, 4u) * 4u;
            for (uint32_t w : {1u, 2u, 4u}) {
              const uint32_t full = grid_policy(regs, (size_t)wave_lds * w, 1u << 30, capped != 0, in_flight, 0u, kCus, w);
              const uint32_t grid = grid_policy(regs, (size_t)wave_lds * w, batches, capped != 0, in_flight, 0u, kCus, w);
              const std::string tuple = "(" + std::to_string(regs) + " VGPRs, " + std::to_string(wave_lds) + " B per wave, " + std::to_string(batches) + " batches, " +
                                        std::to_string(in_flight) + " in flight, capped " + std::to_string(capped) + ", " + std::to_string(w) + " waves per workgroup)";
              if (full * w != w4 || w4 % (4u * kCus) != 0u) return fail_case(tuple + ": " + std::to_string(full * w) + " waves fill the chip, " + std::to_string(w4) + " in 256-thread blocks");
              if (grid == 0u || grid > full || (grid < full && grid != std::max(1u, (batches + w - 1u) / w))) return fail_case(tuple + ": " + std::to_string(grid) + " workgroups");
            }
          }
  // tickets: pairs while every wave gets four batches or more
  const uint32_t tickets[][4] = {{32400u, 2048u, 1u, 2u}, {32400u, 512u, 4u, 2u}, {32400u, 4096u, 1u, 2u}, {8192u, 2048u, 1u, 2u}, {8191u, 2048u, 1u, 1u}, {8191u, 512u, 4u, 1u}, {6u, 6u, 1u, 1u}};
  for (const auto& t : tickets)
    if (ticket_policy(t[0], t[1], t[2]) != t[3])
      return fail_case("ticket_policy(" + std::to_string(t[0]) + " batches, " + std::to_string(t[1]) + " workgroups of " + std::to_string(t[2]) + " waves) is not " + std::to_string(t[3]));
  return RAYCA_OK;
}

// What one generation of the fused engine launches (choose_generation): its node format (decided by timing on this scene,
// RaycaScene::Tune, or forced by Knobs.format), and for Flat camera rays k_generation or the lane-refill kernel.
struct GenChoice {
  int format;          // -1 = default, else bit 0 = 4-wide nodes, bit 1 = fp16 nodes
  bool calibrating;    // a node-format calibration launch
  bool refill;         // k_flat_refill instead of k_generation
  bool refill_cal;     // a kernel calibration launch
};

// ---- self-test of the selection (rayca_hip_selftest): needs no device, the host stubs of the kernels have addresses without one ------
// One picker family: `pick(t, i)` for every flavour of `travs` and every combination i of `bits` flags (bit n of i is the n-th flag
// the name lists) gets a kernel, and two tuples get the same one exactly when `id(t, i)`, the family's narrowing spelled by hand, is equal.
struct PickerFamily {
  const char* picker;
  std::vector<Trav> travs;
  int bits;
  std::function<const void*(Trav, uint32_t)> pick;
  std::function<uint32_t(Trav, uint32_t)> id;
};
int32_t check_family(const PickerFamily& f, std::string& err) {
  struct Picked { const void* kernel; uint32_t id; std::string tuple; };
  std::vector<Picked> v;
  for (Trav t : f.travs)
    for (uint32_t i = 0; i < (1u << f.bits); ++i) v.push_back({f.pick(t, i), f.id(t, i), "trav " + std::to_string(t) + ", flags " + std::to_string(i)});
  for (size_t i = 0; i < v.size(); ++i) {
    if (!v[i].kernel) { err = std::string(f.picker) + ": (" + v[i].tuple + ") gets no kernel"; return RAYCA_ERR_BAD_ARG; }
    for (size_t j = 0; j < i; ++j)
      if ((v[i].kernel == v[j].kernel) != (v[i].id == v[j].id)) {
        err = std::string(f.picker) + ": (" + v[j].tuple + ") and (" + v[i].tuple + (v[i].id == v[j].id ? ") must be one kernel and are two" : ") must be two kernels and are one");
        return RAYCA_ERR_BAD_ARG;
      }
  }
  return RAYCA_OK;
}
int32_t selftest_kernel_selection(std::string& err) {
  const auto b = [](uint32_t i, int n) { return (i >> n & 1u) != 0; };
  const auto P = [](auto kernel) { return reinterpret_cast<const void*>(kernel); };
  const auto mode = [](bool flat) { return flat ? kModeFlat : kModePath; };
  std::vector<Trav> all, none{kTravFast}, wf{kTravFast, kTravFastSpill, kTravExact}, fast{kTravFast, kTravFastSpill, kTravFastWide, kTravFastHalf, kTravFastSpillHalf, kTravFastWideHalf};
  for (int t = 0; t < kTravCount; ++t) all.push_back((Trav)t);
  // the flavours by name, not by the traits table: what the fp16 flavours traverse on f32 nodes, and which are exhaustive
  const auto f32_of = [](Trav t) { return t == kTravFastHalf ? kTravFast : t == kTravFastSpillHalf ? kTravFastSpill : t == kTravFastWideHalf ? kTravFastWide : t; };
  const auto query_of = [](Trav t) { return t == kTravExact || t == kTravExactAll || t == kTravFastAll ? t : kTravFastSpill; };
  const auto exhaustive = [](Trav t) { return t == kTravExactAll || t == kTravFastAll; };
  const auto every = [](Trav t, uint32_t i) { return (uint32_t)t << 8 | i; };   // no narrowing: every tuple its own kernel
  const PickerFamily families[] = {
      {"pick_kernel(trav; sph, stats, flat, gen0, fused, last)", all, 6,
       [&](Trav t, uint32_t i) { return P(pick_kernel(mode(b(i, 2)), b(i, 3), b(i, 4), t, b(i, 0), b(i, 1), b(i, 5))); },
       [&](Trav t, uint32_t i) {   // Flat reads neither gen0 nor last; Path reads fused only as generation 0 on the last-vertex form without the counters
         return (uint32_t)t << 8 | (i & 7u) | ((b(i, 2) ? b(i, 4) : b(i, 3)) ? 8u : 0u) | (!b(i, 2) && b(i, 5) ? 16u : 0u) |
                (!b(i, 2) && b(i, 3) && b(i, 5) && !b(i, 1) && b(i, 4) ? 32u : 0u);
       }},
      {"pick_trace_kernel(trav; sph, stats)", all, 2, [&](Trav t, uint32_t i) { return P(pick_trace_kernel(t, b(i, 0), b(i, 1))); },
       [&](Trav t, uint32_t i) { return (uint32_t)f32_of(t) << 8 | i; }},
      {"pick_query_kernel(trav; sph, stats, occluded)", all, 3, [&](Trav t, uint32_t i) { return P(pick_query_kernel(t, b(i, 0), b(i, 1), b(i, 2))); },
       [&](Trav t, uint32_t i) { return (uint32_t)query_of(t) << 8 | (i & 3u) | (!exhaustive(t) && b(i, 2) ? 4u : 0u); }},
      {"pick_wf_trace(trav; sph, stats, gen0)", wf, 3, [&](Trav t, uint32_t i) { return P(pick_wf_trace(b(i, 2), t, b(i, 0), b(i, 1))); }, every},
      {"pick_wf_shadow(trav; sph, stats, gen0)", wf, 3, [&](Trav t, uint32_t i) { return P(pick_wf_shadow(b(i, 2), t, b(i, 0), b(i, 1))); }, every},
      {"pick_wf_shade(sph, flat, rays, gen0, fused)", none, 5, [&](Trav, uint32_t i) { return P(pick_wf_shade(mode(b(i, 1)), b(i, 3), b(i, 4), b(i, 0), b(i, 2))); },
       [&](Trav, uint32_t i) { return (i & 7u) | (!b(i, 2) && (b(i, 1) ? b(i, 4) : b(i, 3)) ? 8u : 0u); }},   // a caller's rays: neither gen0 nor fused is read
      {"pick_general_kernel(fast, sph, stats)", none, 3, [&](Trav, uint32_t i) { return P(pick_general_kernel(b(i, 0), b(i, 1), b(i, 2))); }, every},
      {"pick_surface_kernel(sph)", none, 1, [&](Trav, uint32_t i) { return P(pick_surface_kernel(b(i, 0))); }, every},
      {"pick_nearest_kernel(within, cull, spill, stats)", none, 4, [&](Trav, uint32_t i) { return P(pick_nearest_kernel(b(i, 0), b(i, 1), b(i, 2), b(i, 3))); },
       [&](Trav, uint32_t i) { return b(i, 1) ? i : i & ~1u; }},   // the exhaustive form does not read within
      {"pick_sample_kernel(geom)", none, 1, [&](Trav, uint32_t i) { return P(pick_sample_kernel(b(i, 0))); }, every},
      {"pick_hits_kernel(trav; sph, stats, both, count_all)", all, 4, [&](Trav t, uint32_t i) { return P(pick_hits_kernel(t, b(i, 0), b(i, 1), b(i, 2), b(i, 3))); },
       [&](Trav t, uint32_t i) { return (uint32_t)query_of(t) << 8 | i; }},
      {"pick_signed_kernel(near, cull, grid, fast, stats)", none, 5,
       [&](Trav, uint32_t i) { return P(pick_signed_kernel(b(i, 0), b(i, 1), b(i, 2), b(i, 3), b(i, 4))); }, every},
      {"pick_ambient_kernel(fast, sph, stats, rot)", none, 4, [&](Trav, uint32_t i) { return P(pick_ambient_kernel(b(i, 0), b(i, 1), b(i, 2), b(i, 3))); }, every},
      {"pick_ambient_finish(bent, rot)", none, 2, [&](Trav, uint32_t i) { return P(pick_ambient_finish(b(i, 0), b(i, 1))); },
       [&](Trav, uint32_t i) { return b(i, 0) ? i : 0u; }},   // without bent_out no direction is made: rot is not read
      {"pick_gather_enqueue(rot)", none, 1, [&](Trav, uint32_t i) { return P(pick_gather_enqueue(b(i, 0))); }, every},
      {"pick_gather_fold(sh, weights, rot)", none, 3, [&](Trav, uint32_t i) { return P(pick_gather_fold(b(i, 0), b(i, 1), b(i, 2))); },
       [&](Trav, uint32_t i) { return b(i, 0) ? i : i & 3u; }},   // without sh_out no direction is made: rot is not read
      {"pick_probe_kernel(fast, sph, stats)", none, 3, [&](Trav, uint32_t i) { return P(pick_probe_kernel(b(i, 0), b(i, 1), b(i, 2))); }, every},
      {"pick_probe_fold(vis, normal, kept)", none, 3, [&](Trav, uint32_t i) { return P(pick_probe_fold(b(i, 0), b(i, 1), b(i, 2))); }, every},
      {"pick_direct_kernel(sphere, fast, sph, stats)", none, 4, [&](Trav, uint32_t i) { return P(pick_direct_kernel(b(i, 0), b(i, 1), b(i, 2), b(i, 3))); }, every},
      {"pick_direct_fold(sphere, sh)", none, 2, [&](Trav, uint32_t i) { return P(pick_direct_fold(b(i, 0), b(i, 1))); },
       [&](Trav, uint32_t i) { return b(i, 0) ? i : 0u; }},   // with normals there is no sh_out: sh is not read
      {"flat_refill_kernel(trav; sph, stats)", fast, 2, [&](Trav t, uint32_t i) { return flat_refill_kernel(RefillFlavour{t, b(i, 0), b(i, 1)}); }, every},
      {"queue_refill_kernel(sph, stats, slack)", none, 3, [&](Trav, uint32_t i) { return queue_refill_kernel(b(i, 0), b(i, 1), b(i, 2)); }, every},
      {"query_refill_kernel(occluded, sph, stats)", none, 3, [&](Trav, uint32_t i) { return query_refill_kernel(b(i, 0), b(i, 1), b(i, 2)); }, every},
      {"ambient_refill_kernel(rot, sph, stats)", none, 3, [&](Trav, uint32_t i) { return ambient_refill_kernel(b(i, 0), b(i, 1), b(i, 2)); }, every},
      {"probe_refill_kernel(sph, stats)", none, 2, [&](Trav, uint32_t i) { return probe_refill_kernel(b(i, 0), b(i, 1)); }, every},
      {"direct_refill_kernel(sphere, sph, stats)", none, 3, [&](Trav, uint32_t i) { return direct_refill_kernel(b(i, 0), b(i, 1), b(i, 2)); }, every},
      {"shadow_refill_kernel(gen0, sph, stats)", none, 3, [&](Trav, uint32_t i) { return shadow_refill_kernel(b(i, 0), b(i, 1), b(i, 2)); }, every},
  };
  for (const PickerFamily& f : families)
    if (const int32_t rc = check_family(f, err); rc != RAYCA_OK) return rc;
  // the traits table against plan_traversal: the flavour it returns is the traversal that was asked for, on a stack plan the
  // kernel of that flavour can run on
  for (uint32_t i = 0; i < 64; ++i)
    for (int format_choice = -1; format_choice < 4; ++format_choice)
      for (uint32_t depth : {3u, 40u}) {   // stack need below and above the LDS part
        const bool ordered = b(i, 0), generation = b(i, 5);
        const TreeFacts tf{b(i, 1), b(i, 2), b(i, 3), depth, b(i, 4) ? depth : depth / 2u + 1u};
        const TravPlan tp = plan_traversal(tf, ordered, generation, format_choice, kMaxLdsEntries);
        const TravTraits tr = traits(tp.trav);
        const bool wide = ordered && tf.fast && tf.formats && (format_choice >= 0 ? (format_choice & 1) != 0 : use_wide(generation));
        const bool half = ordered && tf.fast && tf.formats && tf.half_nodes && format_choice >= 0 && (format_choice & 2) != 0;
        const char* what = tr.ordered != ordered ? "ORDERED is not what was asked for" : tr.fast != tf.fast ? "FAST is not the scene's"
                         : tr.wide != wide ? "WIDE is not the node format asked for" : tr.half != half ? "HALF is not the node format asked for"
                         : tr.wide && !tr.spill ? "WIDE without SPILL" : tr.half && !(tr.ordered && tr.fast) ? "HALF without ORDERED and FAST"
                         : tp.stack.spill_entries && !tr.spill ? "a stack plan with spill entries for a flavour without SPILL" : nullptr;
        if (what) {
          err = std::string("plan_traversal(fast ") + std::to_string(tf.fast) + ", formats " + std::to_string(tf.formats) + ", half_nodes " + std::to_string(tf.half_nodes) +
                ", depth " + std::to_string(tf.depth) + ", depth4 " + std::to_string(tf.depth4) + "; ordered " + std::to_string(ordered) + ", generation " +
                std::to_string(generation) + ", format_choice " + std::to_string(format_choice) + ") gives flavour " + std::to_string(tp.trav) + ": " + what;
          return RAYCA_ERR_BAD_ARG;
        }
      }
  // last_form_rule: the generations of a frame on the last-vertex form, as a bit mask
  struct LastCase { int mode; uint32_t direct_sampler, max_depth, generations, mask; const char* what; };
  const LastCase last_cases[] = {
      {kModePath, RAYCA_SAMPLER_NEE, 1u, 1u, 1u, "max_depth 1 under NEE: generation 0"},
      {kModePath, RAYCA_SAMPLER_NEE, 2u, 2u, 2u, "max_depth 2 under NEE: generation 1 only"},
      {kModePath, RAYCA_SAMPLER_NEE, 3u, 3u, 4u, "max_depth 3 under NEE: generation 2 only"},
      {kModePath, RAYCA_SAMPLER_NONE, 1u, 1u, 0u, "max_depth 1 without a direct sampler: none"},
      {kModePath, RAYCA_SAMPLER_NONE, 3u, 3u, 0u, "max_depth 3 without a direct sampler: none"},
      {kModeFlat, RAYCA_SAMPLER_NEE, 1u, 1u, 0u, "a Flat frame: none"},
  };
  for (const LastCase& c : last_cases) {
    uint32_t mask = 0;
    for (uint32_t g = 0; g < c.generations; ++g) mask |= last_form_rule(c.mode, c.direct_sampler, c.max_depth, g) ? 1u << g : 0u;
    if (mask != c.mask) {
      err = std::string("last_form_rule: ") + c.what + ", got generations " + std::to_string(mask) + " (a bit each)";
      return RAYCA_ERR_BAD_ARG;
    }
  }
  // fuse_resolve_rule: the path frames whose one launch writes the pixel
  struct FuseCase { int mode; bool wavefront, caller_rays, stats; uint32_t spp, generations, direct_sampler, max_depth; bool fused; const char* what; };
  const FuseCase fuse_cases[] = {
      {kModePath, false, false, false, 1u, 1u, RAYCA_SAMPLER_NEE, 1u, true, "the one-sample depth-1 frame under NEE (the bench frame)"},
      {kModePath, false, false, true, 1u, 1u, RAYCA_SAMPLER_NEE, 1u, false, "a counting frame"},
      {kModePath, false, false, false, 4u, 1u, RAYCA_SAMPLER_NEE, 1u, false, "four samples per pixel"},
      {kModePath, false, false, false, 1u, 2u, RAYCA_SAMPLER_NEE, 2u, false, "max_depth 2"},
      {kModePath, false, false, false, 1u, 3u, RAYCA_SAMPLER_NEE, 3u, false, "max_depth 3"},
      {kModePath, false, false, false, 1u, 1u, RAYCA_SAMPLER_NONE, 1u, false, "no direct sampler: generation 0 is on the general form"},
      {kModePath, true, false, false, 1u, 1u, RAYCA_SAMPLER_NEE, 1u, false, "the wavefront engine"},
      {kModePath, false, true, false, 1u, 1u, RAYCA_SAMPLER_NEE, 1u, false, "a caller's rays"},
      {kModeGeneral, false, false, false, 1u, 1u, RAYCA_SAMPLER_NEE, 1u, false, "the stack machine"},
      {kModeFlat, false, false, false, 1u, 1u, RAYCA_SAMPLER_NEE, 1u, false, "a Flat frame (fused by its own rule)"},
  };
  for (const FuseCase& c : fuse_cases)
    if (fuse_resolve_rule(c.mode, c.wavefront, c.caller_rays, c.stats, c.spp, c.generations, c.direct_sampler, c.max_depth) != c.fused) {
      err = std::string("fuse_resolve_rule: ") + c.what + (c.fused ? " must be fused" : " must not be fused");
      return RAYCA_ERR_BAD_ARG;
    }
  return RAYCA_OK;
}
