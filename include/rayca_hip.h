/*
 * rayca_hip.h -- C ABI of librayca_hip.so, the MI355X (gfx950) path-tracing core that sits behind
 * rayca-soft's `Scene` / `Draw::draw()` surface.
 *
 * The reference (Fahien/rayca, Rust) has NO FFI for this path: the interface being replaced is the
 * pure-Rust trait
 *
 *     pub trait Draw { fn draw(&mut self, scene: &Scene, image: &mut Image); }
 *                                                       rayca-soft/src/draw.rs:7-9
 *
 * implemented by `SoftRenderer { pub config: Config }` (rayca-soft/src/scene.rs:11-14,88-154).
 * Everything `draw` does from `SceneDrawInfo::new(scene)` (scene.rs:90) to the RGBA8 store
 * (scene.rs:148) happens behind this ABI; what crosses it is a flat, pointer+size restatement of
 * `&Scene`, `Config` and `&mut Image`:
 *
 *   RaycaSceneDesc  <- rayca-model Scene/Model/Node/Mesh/Primitive/Geometry/Material/Texture/Image/
 *                      Camera/Light                      rayca-model/src/{scene,model,node,...}.rs
 *   RaycaConfig     <- rayca_soft::Config                 rayca-soft/src/config.rs:10-49
 *   rgba8 / rgba32f <- rayca_model::Image (RGBA8, row-major, top-left origin)
 *                                                         rayca-model/src/image.rs:26-36
 *
 * Plain C: fixed-width scalars, pointers and counts only.  No torch / HIP types in signatures
 * (device pointers and streams travel as void*).  Every entry point returns an int32 status
 * (RAYCA_OK == 0, negative on error) and never aborts; `rayca_hip_last_error` returns the
 * thread-local message of the last failure.  The reference panics in the same situations
 * (no camera scene.rs:109, empty TLAS tlas.rs:272, bad index type primitive.rs:258).
 */
#ifndef RAYCA_HIP_H
#define RAYCA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAYCA_ABI_VERSION 2u   /* 2: RaycaRenderOptions.wait_event / record_event, RaycaStats.class_ms / class_launches,
                                  RaycaMultiOptions.context, rayca_hip_render_multi_issue / _wait, rayca_hip_scene_reap.
                                  Added since, without a new version (no layout changed): rayca_hip_scene_update; the resident
                                  draw: RaycaRenderer, the rayca_hip_renderer_ entries, rayca_hip_scene_desc_compare, RAYCA_DRAW_;
                                  rayca_hip_query_device; the surface queries: RaycaSurfaceQuery, rayca_hip_surface_device,
                                  rayca_hip_camera_rays_device; the denoiser: RaycaDenoise, rayca_hip_denoise_device;
                                  temporal accumulation: RaycaCameraPose, rayca_hip_scene_camera, RaycaAccumulate,
                                  rayca_hip_accumulate_device; the variance-guided denoiser: RaycaDenoiseVariance,
                                  rayca_hip_denoise_variance_device; guided upsampling: RaycaUpsample,
                                  rayca_hip_upsample_device; exposure metering and tone mapping: RaycaMeter,
                                  rayca_hip_meter_device, RaycaTonemap, rayca_hip_tonemap_device, RAYCA_TONEMAP_;
                                  radiance along caller-supplied rays: RaycaRadiance, rayca_hip_radiance_device;
                                  nearest-point queries: RaycaNearest, rayca_hip_nearest_device, RAYCA_NEAREST_;
                                  ambient occlusion: RaycaAmbient, rayca_hip_ambient_device;
                                  multi-hit ray queries: RaycaHits, rayca_hip_hits_device, RAYCA_HITS_;
                                  adaptive sampling: RaycaSamplePlan, rayca_hip_sample_plan_device, RaycaFilmFold,
                                  rayca_hip_film_fold_device;
                                  irradiance gathering: RaycaGather, rayca_hip_gather_device;
                                 irradiance volumes: RaycaProbeLookup, rayca_hip_probe_lookup_device;
                                  signed distance and occupancy: RaycaSigned, rayca_hip_signed_device, RAYCA_SIGNED_;
                                  surface sampling: RaycaSurfaceCdf, rayca_hip_surface_cdf_device, RaycaSurfaceSample,
                                  rayca_hip_surface_sample_device */
#define RAYCA_NONE 0xFFFFFFFFu /* Handle::NONE, rayca-util/src/pack.rs:61-64 */

/* ---- status codes -------------------------------------------------------------------------- */
enum {
  RAYCA_OK = 0,
  RAYCA_ERR_BAD_ARG = -1,
  RAYCA_ERR_NO_CAMERA = -2,   /* assert!(!camera_draw_infos.is_empty())      scene.rs:109 */
  RAYCA_ERR_EMPTY_SCENE = -3, /* Tlas::intersects assert                      tlas.rs:272  */
  RAYCA_ERR_HIP = -4,
  RAYCA_ERR_OOM = -5,
  RAYCA_ERR_UNSUPPORTED = -6, /* todo!()/unimplemented!() arms of the reference, or a Config the
                                 kernels do not cover yet: fails loudly, never falls back to CPU */
  RAYCA_ERR_NO_DEVICE = -7,
  RAYCA_ERR_BVH_DEPTH = -8,
  RAYCA_ERR_RCCL = -9 /* the frame-end gather of rayca_hip_render_multi: RCCL missing, or one of its calls failed */
};

/* ---- enums crossing the ABI as uint32, in the reference's #[repr(u32)] order ---------------- */
/* rayca-soft/src/integrator/mod.rs:32-41 */
enum {
  RAYCA_INTEGRATOR_SCRATCHER = 0,
  RAYCA_INTEGRATOR_RAYTRACER = 1,
  RAYCA_INTEGRATOR_FLAT = 2,
  RAYCA_INTEGRATOR_ANALYTIC_DIRECT = 3,
  RAYCA_INTEGRATOR_DIRECT = 4,
  RAYCA_INTEGRATOR_PATHTRACER = 5
};
/* rayca-soft/src/sampler/mod.rs:41-50 */
enum {
  RAYCA_SAMPLER_NONE = 0,
  RAYCA_SAMPLER_NEE = 1,
  RAYCA_SAMPLER_HEMISPHERE = 2,
  RAYCA_SAMPLER_COSINE = 3,
  RAYCA_SAMPLER_BRDF = 4,
  RAYCA_SAMPLER_MIS = 5
};
/* rayca-model/src/material/mod.rs:15-20 */
enum { RAYCA_MATERIAL_PBR = 0, RAYCA_MATERIAL_PHONG = 1, RAYCA_MATERIAL_GGX = 2 };
/* rayca-model/src/light/mod.rs:15-19 */
enum { RAYCA_LIGHT_DIRECTIONAL = 0, RAYCA_LIGHT_POINT = 1, RAYCA_LIGHT_QUAD = 2 };
/* rayca-model Geometry enum (TriangleMesh | Sphere) */
enum { RAYCA_GEOMETRY_TRIANGLE_MESH = 0, RAYCA_GEOMETRY_SPHERE = 1 };
/* rayca-geometry/src/triangle.rs:180-201 ComponentType (glTF numbers) */
enum { RAYCA_INDEX_U8 = 5121, RAYCA_INDEX_U16 = 5123, RAYCA_INDEX_U32 = 5125 };
/* rayca-math/src/color/mod.rs:19-25 ColorType */
enum { RAYCA_COLOR_RGB8 = 0, RAYCA_COLOR_RGBA8 = 1, RAYCA_COLOR_RGBA32F = 2 };

/* ---- Config -------------------------------------------------------------------------------- */
/* Field-for-field mirror of rayca_soft::Config (config.rs:10-49); defaults in
 * rayca_hip_config_default().  `seed` is the one addition: the reference draws from a thread-local
 * OS-seeded fastrand (sampler/cosine.rs:66-67), which is not reproducible; here random numbers are
 * a counter-based function of (seed, pixel, sample, depth, dimension). */
typedef struct RaycaConfig {
  uint32_t bvh;               /* bool, default 1.  0 => Tlas max_depth(0): one leaf per model    */
  uint32_t light_samples;     /* default 1 */
  uint32_t light_stratify;    /* bool, default 0 */
  uint32_t samples_per_pixel; /* default 1 */
  uint32_t russian_roulette;  /* bool, default 0 */
  uint32_t direct_sampler;    /* RAYCA_SAMPLER_*, default NEE */
  uint32_t indirect_sampler;  /* RAYCA_SAMPLER_*, default COSINE */
  uint32_t integrator;        /* RAYCA_INTEGRATOR_*, default PATHTRACER */
  uint32_t max_depth;         /* default 5 */
  float gamma;                /* default 1.0 */
  uint32_t seed;              /* counter-based RNG key (no reference counterpart) */
  uint32_t reserved;
} RaycaConfig;

/* ---- scene description --------------------------------------------------------------------- */
/* rayca_math::Trs: translation, rotation quaternion (x,y,z,w), scale.   rayca-math/src/trs.rs:75-86
 * Applied scale -> rotate -> translate (trs.rs:264-273). */
typedef struct RaycaTrs {
  float translation[3];
  float rotation[4];
  float scale[3];
} RaycaTrs;

/* One entry per node of the flattened scene graph: the Scene root, Scene nodes, each Model's root
 * and its nodes (rayca-model/src/node.rs:11-32).  `parent` indexes this same array (-1 for the
 * top).  Parents must precede children.  World transforms are composed inside the library exactly
 * as SceneDrawInfo::traverse_* does (scene.rs:206-282): world(i) = world(parent) * local(i) with
 * the reference's Trs x Trs (trs.rs:211-221); for a top node world = local (scene.rs:207).
 * `model` groups mesh nodes into one BLAS per model (bvh/primitive.rs:385-393); BLASes are created
 * in ascending `model` order (the reference iterates a HashMap, i.e. leaves this unspecified). */
typedef struct RaycaNode {
  int32_t parent;
  uint32_t model;
  uint32_t mesh;   /* index into meshes, or RAYCA_NONE */
  uint32_t camera; /* index into cameras, or RAYCA_NONE */
  uint32_t light;  /* index into lights, or RAYCA_NONE */
  RaycaTrs trs;    /* node-local */
} RaycaNode;

/* rayca_model::Mesh = list of primitives (mesh.rs:32-35): a contiguous range of `primitives`. */
typedef struct RaycaMesh {
  uint32_t first_primitive;
  uint32_t primitive_count;
} RaycaMesh;

/* rayca_model::Primitive { geometry, material } (primitive.rs:9-14) with the Geometry inlined.
 * Triangle mesh: vertices [first_vertex, first_vertex+vertex_count) of the vertex arrays; indices
 * are `index_count` values of `index_type` starting at byte `index_byte_offset` of `index_bytes`
 * (byte-packed like TriangleIndices, rayca-geometry/src/triangle.rs:215-307), relative to
 * first_vertex.  Sphere: model-space center + radius (rayca-geometry/src/sphere.rs:38-44). */
typedef struct RaycaPrimitive {
  uint32_t geometry;  /* RAYCA_GEOMETRY_* */
  uint32_t material;  /* index into materials, or RAYCA_NONE -> Material::DEFAULT (pbr white) */
  uint32_t first_vertex;
  uint32_t vertex_count;
  uint64_t index_byte_offset;
  uint32_t index_count;
  uint32_t index_type; /* RAYCA_INDEX_* */
  float sphere_center[3];
  float sphere_radius;
} RaycaPrimitive;

/* Material (material/mod.rs:15-20) flattened over its three payloads:
 *   Pbr   (material/pbr.rs:58-66): color, albedo/normal/metallic_roughness textures, factors
 *   Phong (material/phong.rs:10-34): ambient, emission, diffuse, specular, shininess
 *   Ggx   (material/ggx.rs:10-23):  diffuse, specular, roughness                      */
typedef struct RaycaMaterial {
  uint32_t kind; /* RAYCA_MATERIAL_* */
  uint32_t albedo_texture;
  uint32_t normal_texture;
  uint32_t metallic_roughness_texture; /* texture indices or RAYCA_NONE */
  float color[4];
  float metallic_factor;
  float roughness_factor;
  float shininess;
  float pad0;
  float ambient[4];
  float emission[4];
  float diffuse[4];
  float specular[4];
} RaycaMaterial;

/* Texture -> image (texture.rs:35-39); sampler is always the default nearest/wrap one
 * (material/pbr.rs:96, sampler.rs:11-30). */
typedef struct RaycaTexture {
  uint32_t image;
} RaycaTexture;

/* Image payload (image.rs:26-36): `color_type` texels, row-major, at `byte_offset` of image_bytes.
 * Every image of a descriptor, referenced by a texture or not, is checked when the descriptor is taken; RAYCA_ERR_BAD_ARG
 * with a message naming the image unless
 *   - color_type is one of RAYCA_COLOR_RGB8 (3 bytes a texel), RAYCA_COLOR_RGBA8 (4) and RAYCA_COLOR_RGBA32F (16);
 *   - byte_offset + width x height x texel size <= image_byte_count (evaluated without overflow);
 *   - an RGBA32F image's byte_offset is a multiple of 4: its texels are read as floats. */
typedef struct RaycaImage {
  uint32_t width;
  uint32_t height;
  uint32_t color_type; /* RAYCA_COLOR_* */
  uint32_t pad0;
  uint64_t byte_offset;
} RaycaImage;

/* Camera: only yfov reaches the hot path (camera.rs:74-76 get_angle). */
typedef struct RaycaCamera {
  float yfov_radians;
} RaycaCamera;

/* Light (light/{point,quad,directional}.rs). */
typedef struct RaycaLight {
  uint32_t kind; /* RAYCA_LIGHT_* */
  uint32_t material; /* quad light material (light/quad.rs:21), or RAYCA_NONE */
  float intensity;
  float pad0;
  float color[4];
  float attenuation[3]; /* point: (const, linear, quadratic), default (0,0,1) point.rs:20 */
  float pad1;
  float ab[3]; /* quad edges, light/quad.rs:17-18 */
  float pad2;
  float ac[3];
  float pad3;
} RaycaLight;

typedef struct RaycaSceneDesc {
  uint32_t abi_version; /* RAYCA_ABI_VERSION */
  uint32_t flags;       /* 0 */

  const RaycaNode* nodes;
  uint32_t node_count;
  const RaycaMesh* meshes;
  uint32_t mesh_count;
  const RaycaPrimitive* primitives;
  uint32_t primitive_count;

  /* vertex attribute arrays (rayca-geometry/src/vertex.rs:137-142), SoA, vertex_count entries.
   * positions is required; any other pointer may be NULL, meaning the Vertex::default() value
   * (color white, normal +Z, tangent/bitangent zero, uv zero  vertex.rs:164-175). */
  uint32_t vertex_count;
  const float* positions;  /* 3 per vertex */
  const float* colors;     /* 4 per vertex */
  const float* normals;    /* 3 per vertex */
  const float* tangents;   /* 3 per vertex */
  const float* bitangents; /* 3 per vertex */
  const float* uvs;        /* 2 per vertex */

  const uint8_t* index_bytes;
  uint64_t index_byte_count;

  const RaycaMaterial* materials;
  uint32_t material_count;
  const RaycaTexture* textures;
  uint32_t texture_count;
  const RaycaImage* images;
  uint32_t image_count;
  const uint8_t* image_bytes;
  uint64_t image_byte_count;

  const RaycaCamera* cameras;
  uint32_t camera_count;
  const RaycaLight* lights;
  uint32_t light_count;
} RaycaSceneDesc;

/* ---- build / render options (no reference counterpart: knobs of this implementation) -------- */
enum {
  /* bit-for-bit restatement of Blas::set_primitives_recursive (bvh/blas.rs:261-316: SAH over 63
   * planes x 3 axes) and TlasNode::replace_models_recursive (bvh/tlas.rs:74-134), evaluated with an
   * exact binned sweep instead of 189 passes over the primitives */
  RAYCA_BUILDER_REFERENCE = 0,
  /* the same builder with ONE change: the candidate boxes of evaluate_sah start empty instead of at
   * AABB::default() (= the origin, bvh/blas.rs:66-67 + bvh/aabb.rs:9-13).  The reference's seed
   * makes every off-origin cluster unsplittable (leaves of 10^2..10^4 triangles on Sponza-class
   * scenes); without it the tree is a regular SAH tree.  Closest hits are unchanged: depth ties are
   * still resolved by the reference's primitive order, which is computed as well and uploaded as a
   * per-primitive rank. */
  RAYCA_BUILDER_SAH = 1
};
enum {
  /* front-to-back, best-t culled traversal (default).  The closest hit is order independent
   * except for exact depth ties, which "lowest primitive index wins" resolves the way the
   * reference's strict-< DFS does (bvh/blas.rs:151,161,169). */
  RAYCA_TRAVERSAL_ORDERED = 0,
  /* visits exactly the boxes BvhNode::intersects visits (bvh/blas.rs:129-177): every child whose
   * box passes the slab test, no culling by the current best t.  Slow; used to verify ORDERED. */
  RAYCA_TRAVERSAL_EXHAUSTIVE = 1
};

enum {
  /* generation-by-generation rendering where the Config allows it (Flat; Pathtracer with Nee/None direct
   * and Cosine/Hemisphere indirect sampling, one indirect sample per vertex, no roulette) -- FUSED up to two
   * generations, WAVEFRONT from three (measured) -- else the stack machine */
  RAYCA_ENGINE_AUTO = 0,
  /* always the per-pixel stack machine (k_general): every IntegratorStrategy / SamplerStrategy the
   * reference has.  Same results as AUTO where both apply (tested); slower. */
  RAYCA_ENGINE_GENERAL = 1,
  /* the generation kernels' frames with traversal split from shading: lean one-thread-per-ray trace
   * kernels + a streaming shade kernel per generation (wavefront.inc).  Same Configs as the generation
   * kernels, same bits (tested). */
  RAYCA_ENGINE_WAVEFRONT = 2,
  /* the fused persistent kernel per generation (k_generation) */
  RAYCA_ENGINE_FUSED = 3
};

enum {
  /* camera rays of a one-sample Flat frame on a RAYCA_BUILDER_SAH scene: the scene times both kernels on its first
   * large frames and keeps the faster (same bits) */
  RAYCA_CAMERA_AUTO = 0,
  RAYCA_CAMERA_GENERATION = 1, /* the fused generation kernel: a wave keeps its 64 rays until the slowest has finished */
  RAYCA_CAMERA_REFILL = 2      /* lane refill (refill.hip): finished lanes take new pixels while long rays keep theirs */
};

typedef struct RaycaBuildOptions {
  uint32_t builder;   /* RAYCA_BUILDER_* */
  uint32_t device;    /* HIP device ordinal */
  /* 1: run the BLAS builder on the host threads instead of the GPU (bvh_build.hip).  Same tree, same boxes,
   * same primitive order either way (tested); the GPU builder is used from 4096 primitives per BLAS up. */
  uint32_t build_on_host;
  uint32_t reserved[5];
} RaycaBuildOptions;

/* Which rows of the frame this call renders (multi-GPU tile sharding): rows are dealt to `parts`
 * participants in bands of `band_rows`; participant `part` renders bands part, part+parts, ...
 * Output holds only those rows, packed in ascending row order.  parts==1 => the whole frame. */
typedef struct RaycaTile {
  uint32_t part;
  uint32_t parts;
  uint32_t band_rows;
  uint32_t reserved;
} RaycaTile;

typedef struct RaycaRenderOptions {
  uint32_t traversal;     /* RAYCA_TRAVERSAL_* */
  uint32_t collect_stats; /* 1: run the instrumented kernel variant that counts boxes/triangles */
  RaycaTile tile;         /* all zero => whole frame */
  void* stream;           /* hipStream_t to launch on, NULL => the scene's own stream */
  uint32_t engine;        /* RAYCA_ENGINE_*: which kernel family renders the frame */
  /* Frame context 0..7.  Each context owns its work buffers and its default stream, so frames rendered with
   * different contexts (and different streams) may be in flight at the same time; calls that use the same
   * context are serialised.  The scene (BVH, triangles, materials) is shared. */
  uint32_t context;
  uint32_t camera_rays;   /* RAYCA_CAMERA_* */
  uint32_t reserved;      /* must be zero (as every `reserved` field of this header) */
  /* Two hipEvent_t handles (or NULL), so that a frame loop needs ONE call per frame: the frame's stream waits for
   * `wait_event` before its first kernel (e.g. "the previous gather out of this buffer has finished") and `record_event`
   * is recorded on it behind the last one (e.g. for the comm stream to wait on).  rayca_hip_render_device only. */
  void* wait_event;
  void* record_event;
} RaycaRenderOptions;

/* Kernel classes RaycaStats.class_ms / class_launches are indexed by */
enum {
  RAYCA_KERNEL_GENERATION = 0,    /* k_generation: the fused persistent kernel of a generation (kernels.hip)        */
  RAYCA_KERNEL_FLAT_REFILL = 1,   /* k_flat_refill: camera rays with lane refill (refill.hip)                        */
  RAYCA_KERNEL_WF_TRACE = 2,      /* k_wf_trace: closest hits, one ray per lane (wavefront.inc)                      */
  RAYCA_KERNEL_QUEUE_REFILL = 3,  /* k_queue_refill: closest hits of a bounce generation, lane refill (refill.hip)   */
  RAYCA_KERNEL_WF_SHADE = 4,      /* k_wf_shade: shading, NEE set-up, bounce sampling (wavefront.inc)                */
  RAYCA_KERNEL_WF_SHADOW = 5,     /* k_wf_shadow: shadow rays + direct sum, one pixel per lane (wavefront.inc)       */
  RAYCA_KERNEL_SHADOW_REFILL = 6, /* k_shadow_refill: the same with lane refill (refill.hip)                         */
  RAYCA_KERNEL_OTHER = 7,         /* k_general (the stack machine), k_resolve, k_trace_rays, k_query_refill / _rays, k_surface, k_nearest, k_hits */
  RAYCA_KERNEL_CLASSES = 8
};

/* Filled by every render call (all counters are per call, summed over spp and generations). */
typedef struct RaycaStats {
  uint64_t rays_primary;
  uint64_t rays_shadow;      /* NEE / light samples EVALUATED (the reference's count).  A sample that cannot contribute (zero
                              * in r, g, b, finite alpha) is counted here although no shadow ray is traversed for it: such a
                              * sample tests no box, not even the root's, so boxes_tested may be smaller than the number of
                              * rays where many samples are skipped and the tree is shallow (RAYCA_NEE_SKIP=0 traces them all;
                              * so do exhaustive traversal and a scene whose tree is a single leaf) */
  uint64_t rays_bounce;
  uint64_t boxes_tested;     /* only with collect_stats: AABB slab tests (32 B each)            */
  uint64_t triangles_tested; /* only with collect_stats: ray/triangle tests (36 B each)         */
  uint64_t hits_shaded;      /* only with collect_stats */
  /* only with collect_stats: SIMD-slot accounting of the traversal.  Every trip a wave
   * takes through the node loop books 64 x (boxes per node) slots, every trip through the leaf loop 64
   * slots, whatever the number of lanes still taking part: what the lock-step wave pays.
   * boxes_tested / wave_box_slots is the lane utilisation of the node loop. */
  uint64_t wave_box_slots;
  uint64_t wave_triangle_slots;
  float kernel_ms;           /* HIP-event time over all kernels of the frame, on the launch stream */
  float trace_kernel_ms;     /* the traversal kernels alone (the roofline kernel)                */
  uint32_t kernel_launches;
  uint32_t trace_kernel_launches;
  uint32_t rows_rendered;
  /* node format of this frame's launches: bit 0 = generation 0 used 4-wide nodes, bit 1 = the bounce
   * generations did, bits 2 / 3 = the same for fp16 node boxes, bit 8 = this was a calibration frame (the scene
   * is still timing the formats), bit 9 = a calibration frame of the camera-ray kernel choice (Flat frames: fused
   * generation kernel or lane-refill kernel, timed FIRST, on 4-wide f32 nodes; the node formats are timed afterwards on
   * the kernel that won), bit 10 = this frame's camera rays ran on
   * the lane-refill kernel, bit 11 = the scene's 4-wide / fp16 node formats were still being made when this frame was
   * issued (a thread started by rayca_hip_scene_create encodes and uploads them; until then frames traverse the binary
   * f32 nodes and nothing is timed -- same pixels either way), bit 12 = where "binary f32" nodes are traversed by the
   * conservative (RAYCA_BUILDER_SAH) kernels they are read as 48-B centre / half-extent records (three 16-B loads per
   * node instead of four; 0: 64-B min / max nodes), bit 13 = a fused-engine path frame whose one generation kernel wrote the
   * pixel itself: one sample per pixel, max_depth 1 under NEE, not a counting frame -- one launch, no k_resolve
   * (RAYCA_FUSE_RESOLVE=0 in the environment keeps the two launches -- same pixels either way), bit 16 + g (g < 16) = generation g of a fused-engine path frame ran
   * the generation kernel's last-vertex form, the one without the bounce code (no vertex of that generation samples a
   * bounce; RAYCA_LAST_FORM=0 in the environment keeps every generation on the general form -- same pixels either way).
   * Wavefront-engine frames report the formats their kernels are compiled for (bits 0-3). */
  uint32_t node_format;
  /* HIP-event time (ms, summed over the launches of the call) and number of launches per kernel class (RAYCA_KERNEL_*):
   * class_ms[k] / class_launches[k] is the live average launch duration of that kernel -- what bench.py prices its
   * roofline with, and what the rocprofv3 kernel trace of the same command must agree with. */
  float class_ms[8];
  uint32_t class_launches[8];
} RaycaStats;

typedef struct RaycaSceneInfo {
  uint32_t triangle_count;
  uint32_t sphere_count;
  uint32_t blas_count;
  uint32_t node_count;      /* device BVH nodes (64 B each: two child boxes) */
  uint32_t max_depth;       /* traversal stack entries per ray (LDS) the device BVH needs */
  uint32_t light_count;
  uint64_t device_bytes;    /* HBM resident for this scene */
  float build_ms;           /* rayca_hip_scene_create of this scene: flatten + BVH build + binary-node layout + upload,
                               i.e. until a frame can be rendered (the other node formats follow on their own thread) */
  float runtime_init_ms;    /* what that call spent before it: HIP context + code object load, ~0 except for a
                               process's first scene on a device */
} RaycaSceneInfo;

typedef struct RaycaScene RaycaScene; /* opaque: owns the device-resident scene + BVH */

/* ---- entry points -------------------------------------------------------------------------- */

uint32_t rayca_hip_version(void);
/* number of visible HIP devices; 0 (not an error) when there is none */
int32_t rayca_hip_device_count(void);
/* Host-side self-checks that need no GPU: the outward fp16 rounding of the steering boxes (exhaustive over all finite
 * halves), and the multi-threaded device-layout passes of scene_create against their sequential forms on a random
 * tree (identical arrays).  RAYCA_OK or an error with a message in rayca_hip_last_error. */
int32_t rayca_hip_selftest(void);
/* copies the calling thread's last error message (NUL terminated) */
void rayca_hip_last_error(char* buf, size_t len);

/* Config::default() -- rayca-soft/src/config.rs:51-55 */
void rayca_hip_config_default(RaycaConfig* out);

/* The first half of SoftRenderer::draw (scene.rs:90-99): SceneDrawInfo::new, BvhScene::from_scene,
 * Tlas::builder()...build.  Flattens the graph, builds the BVH (cfg->bvh==0 => max_depth 0) and
 * uploads everything to HBM.  The reference repeats this on every draw; here the handle may be
 * reused for any number of render calls. `cfg` may be NULL (defaults); only cfg->bvh is read. */
int32_t rayca_hip_scene_create(const RaycaSceneDesc* desc, const RaycaConfig* cfg,
                               const RaycaBuildOptions* opts, RaycaScene** out);
/* Drop of the BvhScene / Tlas at the end of draw() (scene.rs:154).  Returns at once: the scene's last frames are waited for and
 * its device memory, streams and host arrays released by a thread of the library (7-27 ms of hipFree / hipStreamDestroy that
 * a host rebuilding the scene for every frame would otherwise pay per frame).  The handle is invalid from the call on.
 * Pending releases are completed before the next rayca_hip_scene_create allocates, by rayca_hip_scene_reap, and when the
 * library is unloaded. */
int32_t rayca_hip_scene_destroy(RaycaScene* scene);
/* Waits until every scene handed to rayca_hip_scene_destroy so far has been released (a host that wants the device memory
 * back at a known point).  No reference counterpart. */
int32_t rayca_hip_scene_reap(void);
int32_t rayca_hip_scene_info(const RaycaScene* scene, RaycaSceneInfo* out);
/* rayca_hip_scene_create returns as soon as frames can be rendered -- on the binary f32 nodes; the 4-wide and fp16
 * node formats a RAYCA_BUILDER_SAH scene times against them are encoded and uploaded by a thread of their own, and
 * frames pick them up when they are there (RaycaStats.node_format bit 11).  This waits for that thread: for hosts
 * that want every frame from the first on to be eligible for every format (benchmarks, tests).  Never required:
 * the pixels are the same with every format.  No reference counterpart. */
int32_t rayca_hip_scene_finish(RaycaScene* scene);

/* Re-reads from `desc` what SceneDrawInfo::new re-reads per draw (scene.rs:88-115, 190-282) and what does not move
 * geometry: the camera, the lights, the materials.  `desc` is the whole descriptor the caller would hand to
 * rayca_hip_scene_create for the edited scene; read are only `nodes` (of which only `trs` may differ from creation),
 * `cameras`, `lights`, `materials` and `texture_count`.  The vertex, index, texture and image arrays are NOT read.  Every
 * count (node, mesh, primitive, vertex, index byte, material, texture, image, image byte, camera, light) must equal the
 * scene's, a node's parent / model / mesh / camera / light must be those it was created with, and a material's texture
 * indices must be RAYCA_NONE or in range: else RAYCA_ERR_BAD_ARG.
 *
 * After RAYCA_OK every frame rendered from the handle (any engine, any Config, every render entry point) is bit-identical,
 * RGBA8, RGBA32F and error codes alike, to the same frame rendered from a new rayca_hip_scene_create(desc) with the same
 * cfg->bvh and builder.  An edit that would move geometry is refused with RAYCA_ERR_UNSUPPORTED and a message naming the first
 * offending node or light: the world transform of a node with a mesh changes (a moved ancestor counts), or the local or world
 * transform of a quad light's node, its ab, ac or material, or a light's kind changes to or from RAYCA_LIGHT_QUAD (the quad's
 * two triangles are in the BVH).  A refused edit changes nothing.
 *
 * Frames issued before the call render the old state, frames issued after it the new one.  A camera-only edit waits for
 * nothing and touches no device memory; a light or material edit first waits for the scene's frames in flight, then
 * overwrites the device tables in place.  No reference counterpart (the reference rebuilds everything per draw). */
int32_t rayca_hip_scene_update(RaycaScene* scene, const RaycaSceneDesc* desc);

/* The second half of SoftRenderer::draw (scene.rs:101-150): the pixel loop.  Renders
 * width x height with camera_draw_infos[0] and writes RGBA8 (rgba8.rs:75-84) and/or the
 * pre-quantisation float colour (after /spp and gamma, before the u8 conversion) to HOST memory.
 * Either output pointer may be NULL.  Synchronous. */
int32_t rayca_hip_render(RaycaScene* scene, const RaycaConfig* cfg, uint32_t width,
                         uint32_t height, const RaycaRenderOptions* opts, uint8_t* rgba8_out,
                         float* rgba32f_out, RaycaStats* stats_out);

/* Same frame, outputs left in DEVICE memory (hipMalloc'd by the caller, e.g. a torch tensor's
 * data_ptr) on opts->stream; asynchronous unless stats_out is non-NULL (stats need the events).
 * This is the entry the multi-GPU path uses: each rank renders its RaycaTile into device memory
 * and the frame-end gather (RCCL) runs on the same stream. */
int32_t rayca_hip_render_device(RaycaScene* scene, const RaycaConfig* cfg, uint32_t width,
                                uint32_t height, const RaycaRenderOptions* opts,
                                void* d_rgba8_out, void* d_rgba32f_out, RaycaStats* stats_out);

/* ---- the resident draw(): a renderer handle that reuses, updates or rebuilds -------------------------------------------
 * `Draw::draw(&mut self, scene, image)` (draw.rs:7-9) hands over the whole scene on every call and promises nothing about
 * what changed since the last one.  A RaycaRenderer keeps the scene of its last draw resident, together with an exact host
 * copy of the descriptor it was made from, compares every new descriptor against that copy and does the least that gives
 * the frame a new scene would give: */
enum { RAYCA_DRAW_REUSED = 0,    /* descriptor identical to the resident one: render only             */
       RAYCA_DRAW_UPDATED = 1,   /* differs only in what rayca_hip_scene_update accepts: update+render */
       RAYCA_DRAW_REBUILT = 2 }; /* anything else, or no resident scene: create (+ destroy the old)    */
/* indices of rayca_hip_renderer_last_draw's ms_out (host wall time, milliseconds) */
enum { RAYCA_DRAW_MS_COMPARE = 0, /* descriptor against the kept copy              */
       RAYCA_DRAW_MS_UPDATE = 1,  /* rayca_hip_scene_update, 0 unless UPDATED      */
       RAYCA_DRAW_MS_BUILD = 2,   /* rayca_hip_scene_create, 0 unless REBUILT      */
       RAYCA_DRAW_MS_RENDER = 3,  /* the render call incl. the copy to the host    */
       RAYCA_DRAW_MS_COUNT = 4 };
/* indices of its counters_out */
enum { RAYCA_DRAW_N_BUILDS = 0, RAYCA_DRAW_N_UPDATES = 1, RAYCA_DRAW_N_REUSES = 2, /* totals since renderer_create */
       RAYCA_DRAW_N_KEPT_BYTES = 3,  /* host memory the renderer holds for comparisons */
       RAYCA_DRAW_N_COUNT = 4 };

typedef struct RaycaRenderer RaycaRenderer; /* opaque: owns the resident RaycaScene and the kept copy of its descriptor */

/* Touches no GPU.  `opts` are the build options of every scene the renderer creates; NULL means RAYCA_BUILDER_SAH, device 0,
 * device builder (NOT the default of rayca_hip_scene_create: SAH scenes are tested bit-identical to REFERENCE ones). */
int32_t rayca_hip_renderer_create(const RaycaBuildOptions* opts, RaycaRenderer** out);
/* One draw().  The frame -- RGBA8, RGBA32F, statistics and error code alike -- is that of rayca_hip_scene_create(desc, cfg,
 * the renderer's build options) + rayca_hip_render(cfg, width, height, opts, ...) + rayca_hip_scene_destroy; every field of
 * `opts` keeps its meaning.  What it costs depends on `desc` against the descriptor of the previous draw:
 *   - everything equal (every count, table and array bit for bit, which optional vertex arrays are NULL, cfg->bvh): REUSED;
 *   - counts, meshes, primitives, vertex arrays, indices, textures, images, node parent / model / mesh / camera / light and
 *     cfg->bvh equal, and the differences in nodes' trs, cameras, lights and materials pass rayca_hip_scene_update's own
 *     check for moved geometry: UPDATED (that call, then the kept nodes / cameras / lights / materials are refreshed);
 *   - anything else, no resident scene yet, or rayca_hip_renderer_invalidate since: REBUILT.  The new scene is created
 *     first and the old one destroyed after; a failed create leaves the old scene resident and returns the error.  A
 *     descriptor without a camera is refused (RAYCA_ERR_NO_CAMERA) before anything is built, so that it evicts nothing.
 * A descriptor that is wrong in any scene (version, a null table with a non-zero count, a material's texture index out of
 * range, a node index out of range) is RAYCA_ERR_BAD_ARG.  `action_out` (may be NULL) receives RAYCA_DRAW_*, RAYCA_NONE on error.
 * Calls on one renderer are serialised by a mutex of its own; `desc` is not referenced after the call returns. */
int32_t rayca_hip_renderer_draw(RaycaRenderer* r, const RaycaSceneDesc* desc, const RaycaConfig* cfg, uint32_t width,
                                uint32_t height, const RaycaRenderOptions* opts, uint8_t* rgba8_out, float* rgba32f_out,
                                RaycaStats* stats_out, uint32_t* action_out);
/* The last draw that returned RAYCA_OK: its action (RAYCA_NONE before the first), ms_out[RAYCA_DRAW_MS_COUNT] (zeros before
 * the first), and counters_out[RAYCA_DRAW_N_COUNT], which are totals up to now.  Any of the three may be NULL. */
int32_t rayca_hip_renderer_last_draw(const RaycaRenderer* r, uint32_t* action_out, float* ms_out, uint64_t* counters_out);
/* the resident handle (for rayca_hip_scene_info, rayca_hip_scene_finish, ...), NULL before the first draw; the renderer owns
 * it, and the next REBUILT draw destroys it */
int32_t rayca_hip_renderer_scene(RaycaRenderer* r, RaycaScene** out);
/* the next draw rebuilds, whatever it is handed */
int32_t rayca_hip_renderer_invalidate(RaycaRenderer* r);
/* hands the resident scene to rayca_hip_scene_destroy and releases the kept copy; NULL is RAYCA_OK */
int32_t rayca_hip_renderer_destroy(RaycaRenderer* r);
/* GPU-free: what a renderer holding `resident` (created with cfg->bvh = resident_bvh) does when handed `next` with next_bvh */
int32_t rayca_hip_scene_desc_compare(const RaycaSceneDesc* resident, uint32_t resident_bvh,
                                     const RaycaSceneDesc* next, uint32_t next_bvh, uint32_t* action_out);

/* ---- several devices, one process ----------------------------------------------------------------------
 * Image rows shard across the devices exactly as RaycaTile shards them across ranks (bands of band_rows rows dealt
 * round-robin); every device holds the whole scene; the only exchange is ONE gather of RGBA8 rows to scenes[0]'s device
 * at frame end, then one de-interleave kernel there.  The multi-PROCESS form of the same frame (one rank per GPU,
 * torch.distributed / RCCL) is rayca_amd/distributed.py on top of rayca_hip_render_device; this entry is for a host that is
 * one process -- a Rust or C program calling this header. */
enum {
  /* ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd over xGMI; librccl is opened at first use (RAYCA_ERR_RCCL if it is
   * not installed) */
  RAYCA_GATHER_RCCL = 0,
  /* hipMemcpyPeerAsync from every device to scenes[0]'s: no collective library involved */
  RAYCA_GATHER_PEER_COPY = 1
};
typedef struct RaycaMultiOptions {
  uint32_t traversal;        /* RAYCA_TRAVERSAL_* */
  uint32_t collect_stats;    /* as RaycaRenderOptions.collect_stats */
  uint32_t band_rows;        /* 0 => 8 */
  uint32_t gather;           /* RAYCA_GATHER_* */
  uint32_t engine;           /* RAYCA_ENGINE_* */
  uint32_t output_on_device; /* 1: rgba8_out is device memory of scenes[0]'s device, 0: host memory */
  uint32_t context;          /* frame context 0..7 of every scene (RaycaRenderOptions.context): frames issued with different
                                contexts overlap on the devices (rayca_hip_render_multi_issue) */
  uint32_t reserved;
} RaycaMultiOptions;

/* One frame on `count` devices.  scenes[i] is a handle created (from the same RaycaSceneDesc) on the device that renders
 * part i; scenes[0]'s device assembles the frame.  rgba8_out receives width x height RGBA8 (host memory unless
 * opts->output_on_device).  stats_out: NULL or `count` entries, one per device.  count == 1 is rayca_hip_render.
 * Synchronous: rayca_hip_render_multi_issue + rayca_hip_render_multi_wait on frame context opts->context. */
int32_t rayca_hip_render_multi(RaycaScene* const* scenes, uint32_t count, const RaycaConfig* cfg, uint32_t width,
                               uint32_t height, const RaycaMultiOptions* opts, void* rgba8_out,
                               RaycaStats* stats_out);

/* The same frame, asynchronously: queues the rendering of every part (frame context opts->context of every scene, each on
 * that context's own stream), the one exchange, the de-interleave and the copy into rgba8_out, and returns.  A host that
 * issues frames with contexts 0, 1, 2, 3 in turn and waits for a context only before it re-uses it keeps four frames in
 * flight on every device -- the tail of one frame then runs under the head of the next, which is what a frame-at-a-time
 * loop leaves on the table (one GPU, 1080p primary + shadow: 0.51 -> 0.38 ms per frame; a rank's eighth 0.19 -> 0.06 ms).
 * rgba8_out (and host memory it points to) must stay valid until the matching wait, and so must every scene handle: wait
 * for the frames a scene takes part in before rayca_hip_scene_destroy.  Frames of one context are serialised.  No statistics (they need a synchronisation per frame: use rayca_hip_render_multi).
 * The drop-in host loop (draw.rs:7-9 called per frame) is `issue(ctx = f % 4)`, `wait(ctx = (f + 1) % 4)`. */
int32_t rayca_hip_render_multi_issue(RaycaScene* const* scenes, uint32_t count, const RaycaConfig* cfg, uint32_t width,
                                     uint32_t height, const RaycaMultiOptions* opts, void* rgba8_out);
/* Waits until the frame last issued with frame context `context` on these scenes has landed in its rgba8_out.  A frame's
 * errors are returned by its issue; the wait returns only an error of the synchronisation itself (the frame then stays
 * pending), and RAYCA_OK at once if nothing is pending on that context. */
int32_t rayca_hip_render_multi_wait(RaycaScene* const* scenes, uint32_t count, uint32_t context);

/* RAYCA_OK if librccl can be opened and offers what RAYCA_GATHER_RCCL uses, else RAYCA_ERR_RCCL with the reason in
 * rayca_hip_last_error.  Needs no GPU. */
int32_t rayca_hip_rccl_status(void);

/* Number of rows a RaycaTile covers in a frame of `height` rows (host-side helper, no GPU). */
uint32_t rayca_hip_tile_rows(const RaycaTile* tile, uint32_t height);

/* Debug/parity entry (the analogue of Tlas::intersects, bvh/tlas.rs:271-275): trace `count`
 * caller-supplied rays (origin xyz, dir xyz; 6 floats per ray, HOST memory) and return per ray
 * t (f32::MAX on miss), primitive index in the scene's post-build primitive order (RAYCA_NONE on
 * miss) and the barycentrics u,v.  Synchronous, ordered on context 0 like a frame: it starts behind
 * a frame still in flight there.  */
int32_t rayca_hip_trace_rays(RaycaScene* scene, const RaycaRenderOptions* opts, uint32_t count,
                             const float* rays, float* t_out, uint32_t* prim_out, float* uv_out,
                             RaycaStats* stats_out);

/* Ray queries on DEVICE memory: closest hit or occlusion for `count` caller-supplied rays, each with a distance bound.
 * Rays, bounds and results stay on the device and the call is asynchronous on the caller's stream, so a host that makes
 * its rays on the GPU (visibility between point pairs, depth maps from its own ray generator, picking, AO sampling) never
 * copies them.
 *   A hit counts iff t < tmax, strictly.  tmax = +inf or FLT_MAX: unbounded.  tmax NaN or <= 0: miss / not occluded.
 *   RAYCA_QUERY_CLOSEST   per ray exactly the record rayca_hip_trace_rays returns if that record's t < tmax, else the miss
 *                         record (t = FLT_MAX, prim = RAYCA_NONE, u = v = 0): same bits, same tie rule.  Any of the three
 *                         outputs may be NULL, not all.
 *   RAYCA_QUERY_OCCLUDED  one byte per ray: 1 iff CLOSEST with the same tmax reports a hit.  A ray's search ends at its first
 *                         hit in front of tmax.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event,
 * record_event, collect_stats and traversal as for rayca_hip_render_device; RAYCA_TRAVERSAL_EXHAUSTIVE is offered for CLOSEST
 * only (RAYCA_ERR_UNSUPPORTED for OCCLUDED); tile, engine and camera_rays must be zero.  Calls on one context are serialised
 * and share its work buffers with that context's frames; queries and frames on different contexts overlap.  With
 * stats_out the call waits for the result: rays_primary (CLOSEST) or rays_shadow (OCCLUDED) = count, the kernel's time
 * under RAYCA_KERNEL_OTHER.  count == 0 is RAYCA_OK and launches nothing; nothing outside [0, count) of an output is
 * written.  RAYCA_ERR_BAD_ARG (before any GPU work): NULL scene / query / rays, unknown kind, non-zero reserved, no output
 * for the kind, context > 7.  RAYCA_ERR_EMPTY_SCENE as rayca_hip_trace_rays. */
enum { RAYCA_QUERY_CLOSEST = 0, RAYCA_QUERY_OCCLUDED = 1 };
struct RaycaQuery {
  uint32_t kind;       /* RAYCA_QUERY_* */
  uint32_t count;
  const void* rays;    /* DEVICE: count x 6 f32 (origin xyz, direction xyz; the direction need not be normalised) */
  const void* tmax;    /* DEVICE: count f32, or NULL => tmax_all for every ray */
  float tmax_all;
  uint32_t reserved;   /* must be zero */
  void* t_out;         /* CLOSEST, DEVICE: count f32, FLT_MAX on miss */
  void* prim_out;      /* CLOSEST, DEVICE: count u32, RAYCA_NONE on miss; post-build primitive order */
  void* uv_out;        /* CLOSEST, DEVICE: count x 2 f32, 0 on miss */
  void* occluded_out;  /* OCCLUDED, DEVICE: count u8, 1 / 0 */
};
typedef struct RaycaQuery RaycaQuery;
int32_t rayca_hip_query_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaQuery* query,
                               RaycaStats* stats_out);

/* Nearest-point queries on DEVICE memory: for `count` caller-supplied points the nearest point of the scene's surface within a
 * radius, and how far away it is -- distance fields, clearance and collision tests, snapping samples onto a mesh, picking by
 * proximity.  Points, radii and results stay on the device and the call is asynchronous on the caller's stream.
 *
 * The specification, in f32 with every operation rounded on its own (+ - * /, comparisons and selects; no square root, which
 * is why the SQUARED distance is returned).  x.y = (x0*y0 + x1*y1) + x2*y2.
 *   Candidates: every triangle slot of the scene (post-build primitive order; the two triangles of a quad light count, as they
 *   do for closest hits).  A scene with spheres is refused: RAYCA_ERR_UNSUPPORTED.
 *   Nearest point q on triangle (a, b, c) = the slot's world-space vertices 0, 1, 2, to the point p (Ericson, Real-Time
 *   Collision Detection 5.1.5):
 *     ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c                        (componentwise)
 *     d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp
 *     vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4
 *     the first of these tests that holds decides (s, t):
 *       d1 <= 0 and d2 <= 0                          vertex a   (s, t) = (0, 0)
 *       d3 >= 0 and d4 <= d3                         vertex b   (s, t) = (1, 0)
 *       vc <= 0 and d1 >= 0 and d3 <= 0              edge ab    s = d1 / (d1 - d3), t = 0
 *       d6 >= 0 and d5 <= d6                         vertex c   (s, t) = (0, 1)
 *       vb <= 0 and d2 >= 0 and d6 <= 0              edge ac    s = 0, t = d2 / (d2 - d6)
 *       va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    edge bc    t = (d4 - d3) / ((d4 - d3) + (d5 - d6)), s = 1 - t
 *       none                                         interior   s = vb / ((va + vb) + vc), t = vc / ((va + vb) + vc), then
 *                                                               s = s < 0 ? 0 : s, s = s > 1 ? 1 : s, t = t < 0 ? 0 : t,
 *                                                               t = t > 1 - s ? 1 - s : t
 *     (the selects of the interior branch change nothing unless rounding has left va, vb, vc with mixed signs -- a point very
 *     far away, a needle -- and then keep q on the triangle)
 *     q = (a + ab*s) + ac*t componentwise; in the three vertex regions q is the vertex itself.  d = p - q, dist2 = d.d.
 *     A candidate whose dist2 is NaN is no candidate: a degenerate triangle whose quotient is 0 / 0 (two equal vertices in the
 *     region of their edge, va + vb + vc = 0 in the interior branch), vertices whose products overflow (a NaN fails every
 *     comparison it enters and ends in the interior branch).  Other degenerate triangles are the segment or point they are.
 *   Bound: r2 = radius * radius.  A candidate counts iff dist2 < r2, strictly.  radius = +inf or FLT_MAX is unbounded (r2 =
 *   +inf); a candidate with dist2 = +inf never counts.  A radius that is NaN or <= 0 gives a miss; a point with a coordinate
 *   that is not finite gives a miss.
 *   Result: among the candidates that count the smallest dist2 wins; on equal dist2 the lowest slot.  (Ties are common: the
 *   nearest points of two triangles that share a vertex or an edge are often the same three floats.  Slots differ between
 *   builders, and so may the winner of a tie.)
 *   RAYCA_NEAREST_CLOSEST  per point dist2, the slot, q and (u, v) = ((1 - s) - t, s): the weights of vertex 0 and vertex 1,
 *                          the convention of hit records, so that prim_out / uv_out can be handed to
 *                          rayca_hip_surface_device as they are (colour, material, flags).  A miss is dist2 = FLT_MAX,
 *                          prim = RAYCA_NONE, zeros elsewhere.  Any of the four outputs may be NULL, not all.
 *   RAYCA_NEAREST_WITHIN   one byte per point: 1 iff CLOSEST with the same radius reports a hit.  A point's search ends at the
 *                          first candidate that counts.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event,
 * collect_stats and traversal as for rayca_hip_query_device; RAYCA_TRAVERSAL_EXHAUSTIVE visits every node and every triangle
 * without the cull, gives the same results bit for bit and is offered for CLOSEST only (RAYCA_ERR_UNSUPPORTED for WITHIN);
 * tile, engine and camera_rays must be zero.  Ordered on its context like a query.  With stats_out the call waits: the kernel's
 * time under RAYCA_KERNEL_OTHER (with collect_stats it includes reading the counters back), kernel_launches = 1, boxes_tested
 * and triangles_tested under collect_stats, every rays_* field 0.  count == 0 is RAYCA_OK and launches nothing; nothing outside
 * [0, count) of an output is written.
 * RAYCA_ERR_BAD_ARG, before any GPU work and before the scene is looked at, in this order: NULL scene / query, NULL points,
 * unknown kind, non-zero reserved, no output for the kind; then context > 7, a non-zero field of opts that does not apply;
 * then RAYCA_ERR_UNSUPPORTED for EXHAUSTIVE with WITHIN.  Then (count != 0) RAYCA_ERR_EMPTY_SCENE as the query, and
 * RAYCA_ERR_UNSUPPORTED for a scene with spheres. */
enum { RAYCA_NEAREST_CLOSEST = 0, RAYCA_NEAREST_WITHIN = 1 };
struct RaycaNearest {
  uint32_t kind;        /* RAYCA_NEAREST_* */
  uint32_t count;
  const void* points;   /* DEVICE: count x 3 f32 */
  const void* radius;   /* DEVICE: count f32, or NULL => radius_all for every point */
  float radius_all;
  uint32_t reserved;    /* must be zero */
  void* dist2_out;      /* CLOSEST, DEVICE: count f32, SQUARED distance, FLT_MAX on a miss */
  void* prim_out;       /* CLOSEST, DEVICE: count u32 slot (post-build primitive order), RAYCA_NONE on a miss */
  void* point_out;      /* CLOSEST, DEVICE: count x 3 f32, the nearest point, 0 on a miss */
  void* uv_out;         /* CLOSEST, DEVICE: count x 2 f32 in the convention of hit records, 0 on a miss */
  void* within_out;     /* WITHIN, DEVICE: count u8, 1 / 0 */
};
typedef struct RaycaNearest RaycaNearest;
int32_t rayca_hip_nearest_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaNearest* query,
                                 RaycaStats* stats_out);

/* Surface sampling on DEVICE memory: area-weighted random points on the scene's triangles -- training points for distance
 * fields (perturbed, into rayca_hip_signed_device), point clouds for Chamfer and Hausdorff distances (into
 * rayca_hip_nearest_device), the points and normals an occlusion or irradiance bake runs over (rayca_hip_ambient_device,
 * rayca_hip_gather_device), probe placement.  Two calls: rayca_hip_surface_cdf_device turns the slots' areas into a table of
 * exact integer prefix sums, rayca_hip_surface_sample_device draws from such a table.  A handle's geometry never changes
 * (rayca_hip_scene_update refuses every edit that moves it), so a table stays valid for as long as its handle lives.  No
 * reference counterpart.  Neither call traverses anything; tables, seeds' samples and results stay on the device and both
 * calls are asynchronous on the caller's stream.
 *
 * The specification, in f32 with every operation rounded on its own and in the association written here; behind the weight
 * everything is integer arithmetic, and no result depends on an order of execution, so a literal restatement
 * (tests/sample_literal.py) gives the same words.  T = the number of triangle slots.
 *   Candidates: every triangle slot of the scene (post-build primitive order; the two triangles of a quad light count, as they
 *   do for nearest points).  A scene with spheres is refused: RAYCA_ERR_UNSUPPORTED.
 *   Area of slot i, with a, b, c = the slot's world-space vertices 0, 1, 2:
 *     ab = b - a, ac = c - a                                                             (componentwise)
 *     n = (ab.y*ac.z - ab.z*ac.y, ab.z*ac.x - ab.x*ac.z, ab.x*ac.y - ab.y*ac.x)
 *     a2 = (n.x*n.x + n.y*n.y) + n.z*n.z
 *     area_i = sqrt(a2), correctly rounded: the build's sqrtf, which the compiler lowers to its correctly rounded f32 square
 *     root (its default for HIP; __fsqrt_rn of this toolchain is the approximate native instruction and is NOT used).  This is
 *     twice the triangle's area; the common factor changes no share.
 *     area_i counts as 0 if it is NaN or +inf (vertices whose products overflow), and if include[i] == 0.
 *   Weights: amax = the largest area_i, found as an integer maximum over the floats' bits (non-negative floats order as their
 *   bits do) -- the only atomic in either call.  With amax = m * 2^e, 0.5 <= m < 1:
 *     w_i = (uint32) floor(area_i * 2^(32 - e)).  The factor is an f32: an area that counts is the root of an a2 >= 2^-149, so
 *     2^-75 <= amax <= FLT_MAX and -96 <= 32 - e <= 106 (the kernel applies it as an exponent shift, ldexpf: the same product).
 *     area_i <= amax < 2^e, so w_i < 2^32.  The product is exact unless it underflows, and then the
 *     result is below 1 and w_i = 0: A TRIANGLE WHOSE AREA IS BELOW 2^-32 OF THE LARGEST HAS WEIGHT 0 AND IS NEVER DRAWN; every
 *     other weight is its area's share of amax to 2^-32 absolute.  amax = 0 (no area counts) makes every weight 0.
 *   Table: cdf_out[0] = 0, cdf_out[i + 1] = cdf_out[i] + w_i as uint64 -- an exact prefix sum in slot order, formed without
 *   atomics.  T <= 2^25 slots of weights below 2^32: every entry is below 2^57.
 *   Sample j (0 <= j < count) of a table cdf, with W(key, d) = the 32-bit hash word rng_f32 takes its mantissa from
 *   (rayca_math.hpp rng_word):
 *     key = rng_root(seed, (first_index + j) mod 2^32, sample)       the stream RaycaRadiance names the same way
 *     r = W(key, 0) * 2^32 + W(key, 1), total = cdf[T]
 *     target = floor(r * total / 2^64)                               the high half of the 128-bit product; < total
 *     prim = the slot i with cdf[i] <= target < cdf[i + 1]: it exists and is unique when total > 0, and its weight is not 0
 *     s0 = rng_f32(key, 2), t0 = rng_f32(key, 3)                     multiples of 2^-23 in [0, 1)
 *     if s0 + t0 > 1: s = 1 - s0, t = 1 - t0; else s = s0, t = t0
 *     Every one of these operations is exact: s0 + t0 is a multiple of 2^-23 below 2 and 1 - s0 one in (0, 1], each of at most
 *     24 significant bits; so is (1 - s) - t below, which lies in [0, 1] because s + t <= 1.  Hence s, t >= 0, s + t <= 1, and
 *     the fold maps the upper half of the unit square onto the lower: (s, t) is uniform over the triangle's 2^-23 lattice.
 *     prim_out[j]   = prim
 *     uv_out[j]     = ((1 - s) - t, s): the weights of vertex 0 and vertex 1, the convention of hit records, so that prim_out /
 *                     uv_out go to rayca_hip_surface_device as they are (colour, material, flags; no rays needed)
 *     point_out[j]  = (a + ab*s) + ac*t componentwise, as rayca_hip_nearest_device forms q
 *     normal_out[j] = (n.x / l, n.y / l, n.z / l), l = sqrt(a2): the geometric normal in winding order (a drawn slot has
 *                     0 < l < +inf)
 *     total == 0 makes every sample a miss: prim = RAYCA_NONE, zeros elsewhere.
 *   Consequences: sample j does not depend on count; any split of a sample set into consecutive calls, each with the
 *   first_index of its first sample, writes what one call writes.
 *   `cdf` need not come from rayca_hip_surface_cdf_device: any T + 1 non-decreasing uint64 with cdf[0] = 0 weighs the slots
 *   (per material, by a texture's importance); with an entry that decreases the slot drawn is unspecified but in range.
 * Not offered: stratified or systematic draws (target = (j + xi) * total / count needs a 128-bit quotient per sample, and the
 * draws are no longer independent of count); a table per model (include masks do that: one byte per slot); spheres.
 * opts (may be NULL) for both calls: stream (NULL => the context's own stream, and the call waits for it), context,
 * wait_event, record_event as for rayca_hip_nearest_device; collect_stats is accepted and counts nothing; traversal, tile,
 * engine and camera_rays must be zero.  Ordered on their context like a query.  With stats_out the call waits: the kernels'
 * time under RAYCA_KERNEL_OTHER, kernel_launches = 3 for the table (the maximum, the weights, the one-block scan) and 1 for a
 * draw, every rays_* field 0.  The table call keeps one scratch word on its context.  count == 0 is RAYCA_OK and launches
 * nothing; nothing outside [0, count) of an output, or [0, T] of cdf_out, is written.
 * RAYCA_ERR_BAD_ARG, before any GPU work and before the scene is looked at, in this order --
 *   table: NULL scene / arguments, non-zero reserved, non-zero flags, NULL cdf_out, cdf_out not 8-byte aligned;
 *   draw:  NULL scene / arguments, non-zero reserved, NULL cdf, cdf not 8-byte aligned, no output;
 * then context > 7, a non-zero field of opts that does not apply.  Then (the draw: for count != 0) RAYCA_ERR_EMPTY_SCENE as the
 * query, and last RAYCA_ERR_UNSUPPORTED for a scene with spheres. */
struct RaycaSurfaceCdf {
  const void* include;  /* DEVICE: T u8, 0 = the slot has area 0; or NULL => every slot */
  void* cdf_out;        /* DEVICE: (T + 1) u64, 8-byte aligned, required */
  uint32_t flags;       /* must be zero */
  uint32_t reserved;    /* must be zero */
};
typedef struct RaycaSurfaceCdf RaycaSurfaceCdf;
int32_t rayca_hip_surface_cdf_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaSurfaceCdf* table,
                                     RaycaStats* stats_out);
struct RaycaSurfaceSample {
  uint32_t count;
  uint32_t seed;         /* as RaycaConfig.seed */
  uint32_t sample;       /* RNG stream of the draws, as RaycaRadiance.sample */
  uint32_t first_index;  /* the index of sample 0; first_index + j wraps at 2^32 */
  const void* cdf;       /* DEVICE: (T + 1) u64, 8-byte aligned, required */
  void* prim_out;        /* DEVICE: count u32 slot (post-build primitive order), RAYCA_NONE on a miss; any of the four may be NULL, not all */
  void* uv_out;          /* DEVICE: count x 2 f32 in the convention of hit records, 0 on a miss */
  void* point_out;       /* DEVICE: count x 3 f32, 0 on a miss */
  void* normal_out;      /* DEVICE: count x 3 f32, unit length, 0 on a miss */
  uint32_t reserved;     /* must be zero (4 bytes of padding follow) */
};
typedef struct RaycaSurfaceSample RaycaSurfaceSample;
int32_t rayca_hip_surface_sample_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaSurfaceSample* draw,
                                        RaycaStats* stats_out);

/* Multi-hit ray queries on DEVICE memory: for `count` caller-supplied rays the first k hits along each ray, in order, or the
 * number of all of them -- thickness and transmission through layers, crossing counts, picking through a surface, x-ray and
 * depth-peeling views, inside / outside tests.  One traversal and one launch, where k closest-hit queries restarted "a little
 * past" the last hit cost k of each and either skip coincident surfaces or find the same one again.  Rays, bounds and results
 * stay on the device and the call is asynchronous on the caller's stream.
 *
 * The specification.  Every operation is f32 and rounded on its own.
 *   The hits of a ray: a hit is a primitive slot (post-build primitive order) whose test accepts the ray and whose hit the
 *   reference would have seen -- exactly the set RAYCA_QUERY_CLOSEST takes its minimum over:
 *     the test      Triangle::intersects on the slot's world-space vertices (v0, v1, v2) (rayca-geometry/src/triangle.rs:84-159,
 *                   which culls back faces), Sphere::intersects for a sphere slot (sphere.rs:101-163); it yields t and (u, v);
 *     "seen"        AABB::intersects (bvh/aabb.rs:74-93) accepts the ray on the box of the reference's leaf that holds the
 *                   primitive.  The boxes above a leaf in the reference's trees are nested and the box test is monotone in the
 *                   corners, so this is what the reference's own descent decides; a RAYCA_BUILDER_REFERENCE scene runs that
 *                   descent itself.
 *   A hit counts iff t < tmax, strictly.  tmax = +inf or FLT_MAX is unbounded, and unbounded means t < +inf: a t that is NaN
 *   or +inf never counts.  A tmax that is NaN or <= 0 leaves the ray without hits, and so does an origin or direction component
 *   that is not finite.
 *   Order: by (t, tie rank) -- t compared as floats; on equal t the primitive that comes first in the reference's primitive
 *   order (rayca_hip_scene_primitive_order) goes first, the rule closest hits resolve exact ties by.  Ranks are unique, so the
 *   order is total and the result does not depend on the order in which a traversal visits anything.
 *   Faces:
 *     RAYCA_HITS_FRONT  the test as it stands.
 *     RAYCA_HITS_BOTH   additionally, a triangle that the test rejects by its back-face line -- n = cross(v1 - v0, v2 - v0),
 *                       dot(d, n) > 0 -- is tested as the triangle (v0, v2, v1) with the same test.  That test yields t and
 *                       (u', v'), the weights of v0 and v2; the hit is reported with (u, v) = (u', (1 - u') - v') -- two
 *                       subtractions in this order -- the weights of vertex 0 and vertex 1 as every hit record carries them, and
 *                       with face = 1.  Every other hit has face = 0.  A sphere slot is one hit as Sphere::intersects computes
 *                       it under either setting, face 0.  "Seen" is the same for both faces.
 *   Result per ray: the first k counting hits in order, entry j of ray i at index i * k + j of each record output (ray-major):
 *   t, prim (the slot), (u, v), face.  Unused entries are the miss record (t = FLT_MAX, prim = RAYCA_NONE, u = v = 0, face = 0).
 *     count_all == 0  n_out = min(number of counting hits, k).
 *     count_all == 1  n_out = the number of ALL counting hits; the entries are the same.  The search is then bounded by tmax
 *                     alone.  k == 0 is allowed here: a crossing count with no record outputs.
 *   Consequences (for rays whose components are finite):
 *     with FRONT and k >= 1, entry 0 is bit for bit the record RAYCA_QUERY_CLOSEST writes for the same ray and tmax;
 *     n_out > 0 iff RAYCA_QUERY_OCCLUDED says 1;
 *     the first k entries of a call with k' > k are the entries of the call with k.
 * Any output may be NULL, not all; with k == 0 only n_out may be given, and it must be.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event,
 * collect_stats and traversal as for rayca_hip_nearest_device; RAYCA_TRAVERSAL_EXHAUSTIVE visits every node the reference's boxes
 * admit without the distance cull and gives the same results bit for bit; tile, engine and camera_rays must be zero.  Ordered on
 * its context like a query.  With stats_out the call waits: rays_primary = count, kernel_launches = 1, the kernel's time under
 * RAYCA_KERNEL_OTHER (with collect_stats it includes reading the counters back), boxes_tested and triangles_tested under
 * collect_stats.  count == 0 is RAYCA_OK and launches nothing; nothing outside [0, count * k) of a record output or [0, count) of
 * n_out is written.  Scenes with spheres are served.
 * RAYCA_ERR_BAD_ARG, before any GPU work and before the scene is looked at, in this order: NULL scene / query; NULL rays;
 * k > RAYCA_HITS_MAX; unknown faces; count_all > 1; non-zero reserved; k == 0 without count_all; no output, or a record output
 * with k == 0; context > 7; a non-zero field of opts that does not apply.  Then (count != 0) RAYCA_ERR_EMPTY_SCENE as the query. */
#define RAYCA_HITS_MAX 16u
enum { RAYCA_HITS_FRONT = 0, RAYCA_HITS_BOTH = 1 };
struct RaycaHits {
  uint32_t count, k;    /* k in 0..RAYCA_HITS_MAX; k == 0 needs count_all */
  const void* rays;     /* DEVICE: count x 6 f32, as RaycaQuery.rays */
  const void* tmax;     /* DEVICE: count f32, or NULL => tmax_all for every ray */
  float tmax_all;
  uint32_t faces;       /* RAYCA_HITS_* */
  uint32_t count_all;   /* 0 / 1 */
  uint32_t reserved;    /* must be zero */
  void* t_out;          /* DEVICE: count x k f32, FLT_MAX in unused entries */
  void* prim_out;       /* DEVICE: count x k u32 slot (post-build primitive order), RAYCA_NONE in unused entries */
  void* uv_out;         /* DEVICE: count x k x 2 f32 in the convention of hit records, 0 in unused entries */
  void* face_out;       /* DEVICE: count x k u8, 1 for a hit on the back of a triangle (RAYCA_HITS_BOTH), else 0 */
  void* n_out;          /* DEVICE: count u32 */
};
typedef struct RaycaHits RaycaHits;
int32_t rayca_hip_hits_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaHits* query, RaycaStats* stats_out);

/* Signed distance and occupancy on DEVICE memory: for `count` points the nearest surface point of the scene's triangles and
 * whether the point lies inside the surface -- signed distance fields, occupancy masks, voxelisation, collision and clearance
 * tests, and a signed-distance volume on a regular grid without a point buffer.  One launch where the composition costs a nearest
 * call, a ray buffer per direction (24 B per point and direction, written and read again), a crossing count per direction and a
 * reduction.  The rays are made in registers; points and results stay on the device; asynchronous on the caller's stream.
 *
 * The specification.  Every operation is f32 and rounded on its own.
 *   The points (source):
 *     RAYCA_SIGNED_POINTS  point i is (points[3i], points[3i + 1], points[3i + 2]).
 *     RAYCA_SIGNED_GRID    no point buffer is read.  With (nx, ny, nz) = grid_dims, point i has ix = i % nx, iy = (i / nx) % ny,
 *                          iz = i / (nx * ny) -- x runs fastest -- and per axis p = origin + (float)index * step: convert,
 *                          multiply, add.  count must equal nx * ny * nz (computed in 64 bits; at most 2^32 - 1).
 *   The distance part (dist2_out, prim_out, point_out, uv_out): bit for bit what RAYCA_NEAREST_CLOSEST writes for the same point
 *   and radius (radius / radius_all as in RaycaNearest) -- the candidates, the strict bound dist2 < radius * radius, the tie to
 *   the lowest slot, the miss record (dist2 = FLT_MAX, prim = RAYCA_NONE, zeros elsewhere), and the dead-point rule: a radius
 *   that is NaN or <= 0, or a coordinate that is not finite, gives a miss.  The search runs only if one of the four is given.
 *   The sign part (inside_out, votes_out, cross_out) does not depend on radius.  For direction j < n_dirs the ray is
 *   (p, dirs[j]), and its hits are those of rayca_hip_hits_device with RAYCA_HITS_BOTH, count_all and an unbounded tmax: the same
 *   test, the same "seen by the reference's leaf box" rule, the same t < +inf rule.
 *     front_j = the number of those hits with face 0, back_j = the number with face 1
 *     RAYCA_SIGNED_PARITY   vote_j = (front_j + back_j) & 1
 *     RAYCA_SIGNED_WINDING  vote_j = back_j > front_j.  A ray that leaves a closed, outward-wound solid exits it once more than it
 *                           enters it, so a point in the union of overlapping solids is inside, where parity calls the overlap
 *                           of two solids outside.
 *     votes  = the OR of vote_j << j over j < n_dirs
 *     inside = 2 * popcount(votes) > n_dirs ? 1 : 0                                        (a strict majority; n_dirs is odd)
 *     cross_out[(i * n_dirs + j) * 2 + 0 / 1] = front_j / back_j
 *   A point with a coordinate that is not finite has votes 0, inside 0 and every crossing 0.
 *   Consequences (for points whose coordinates are finite):
 *     front_j equals n_out of a multi-hit query with k = 0, count_all, RAYCA_HITS_FRONT and tmax_all = INFINITY on the ray
 *     (p, dirs[j]); front_j + back_j equals n_out of the same call with RAYCA_HITS_BOTH.
 *   What the sign is worth: it is only as good as the crossing counts.  It is meaningful for closed, consistently wound meshes.
 *   The reference's triangle test drops a hit whose unnormalised |n.d| < FLT_EPSILON, so a mesh of very small triangles loses
 *   crossings; a ray through an edge or a vertex may count both triangles or neither; points on or within rounding of a surface
 *   can land on either side.  That is why several directions vote, and votes_out is how a caller sees them disagree.  No component
 *   of a direction may be zero: the reference's box test gives an axis-aligned ray no hits at all.
 * Any output may be NULL, but one of inside_out, votes_out, cross_out must be given: without them the call is
 * rayca_hip_nearest_device.
 * opts (may be NULL): stream, context, wait_event, record_event, collect_stats and traversal as for rayca_hip_nearest_device;
 * RAYCA_TRAVERSAL_EXHAUSTIVE runs both searches without the cull and the ordering and gives the same results bit for bit; tile,
 * engine and camera_rays must be zero.  Ordered on its context like a query.  With stats_out the call waits: kernel_launches = 1,
 * rays_primary = count * n_dirs, the kernel's time under RAYCA_KERNEL_OTHER, and under collect_stats boxes_tested and
 * triangles_tested summed over both searches.  count == 0 is RAYCA_OK and launches nothing; nothing outside [0, count) of an
 * output ([0, count * n_dirs * 2) of cross_out) is written.
 * RAYCA_ERR_BAD_ARG, before any GPU work and before the scene is looked at, in this order: NULL scene / query; unknown source;
 * POINTS with NULL points; GRID with a zero dimension or nx * ny * nz != count; unknown rule; n_dirs not 1, 3 or 5; a component of
 * one of the first n_dirs directions that is zero, NaN or infinite; non-zero reserved; none of the three sign outputs; then
 * context > 7, a non-zero field of opts that does not apply.  Then (count != 0) RAYCA_ERR_EMPTY_SCENE as the query, and
 * RAYCA_ERR_UNSUPPORTED for a scene with spheres, as rayca_hip_nearest_device. */
enum { RAYCA_SIGNED_POINTS = 0, RAYCA_SIGNED_GRID = 1 };
enum { RAYCA_SIGNED_PARITY = 0, RAYCA_SIGNED_WINDING = 1 };
struct RaycaSigned {
  uint32_t count;
  uint32_t source;         /* RAYCA_SIGNED_POINTS / RAYCA_SIGNED_GRID */
  const void* points;      /* POINTS, DEVICE: count x 3 f32 */
  const void* radius;      /* DEVICE: count f32, or NULL => radius_all for every point */
  float radius_all;
  uint32_t rule;           /* RAYCA_SIGNED_PARITY / RAYCA_SIGNED_WINDING */
  uint32_t n_dirs;         /* 1, 3 or 5 */
  uint32_t reserved;       /* must be zero */
  float grid_origin[3];    /* GRID: the point of index (0, 0, 0) */
  float grid_step[3];      /* GRID: the spacing per axis */
  uint32_t grid_dims[3];   /* GRID: (nx, ny, nz), x fastest */
  float dirs[5][3];        /* the first n_dirs are used; no zero, NaN or infinite component */
  void* dist2_out;         /* DEVICE: count f32, SQUARED distance, FLT_MAX on a miss */
  void* prim_out;          /* DEVICE: count u32 slot (post-build primitive order), RAYCA_NONE on a miss */
  void* point_out;         /* DEVICE: count x 3 f32, the nearest point, 0 on a miss */
  void* uv_out;            /* DEVICE: count x 2 f32 in the convention of hit records, 0 on a miss */
  void* inside_out;        /* DEVICE: count u8, 1 / 0 */
  void* votes_out;         /* DEVICE: count u8, bit j = direction j's vote */
  void* cross_out;         /* DEVICE: count x n_dirs x 2 u32, (front, back) per direction */
};
typedef struct RaycaSigned RaycaSigned;
int32_t rayca_hip_signed_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaSigned* query, RaycaStats* stats_out);

/* Ambient occlusion on DEVICE memory: how open the scene is at `count` caller-supplied points -- `samples` occlusion rays over the
 * hemisphere of each point's normal, folded into one record per point: ambient occlusion on a G-buffer, sky visibility, per-vertex
 * baking, contact shadows.  The rays are made in registers inside the traversal kernel: no ray buffer is written or read, and the
 * surface records of rayca_hip_surface_device (point, normal) go in as they are.  Asynchronous on the caller's stream.
 *
 * The specification, in f32 with every operation rounded on its own (+ - * /, comparisons and selects; no square root, no
 * trigonometry).
 *   Per point i: position p; normal n (expected unit length, not checked); optionally a rotation (c, s); optionally a radius.
 *   Per call: a table `dirs` of dir_count local directions (lx, ly, lz), z along the normal; samples = S, 1 <= S <= 64; dir_first
 *   with dir_first + S <= dir_count; bias; radius_all.
 *   Frame (the branch-free basis of Duff et al. 2017, its sign taken by a comparison):
 *     sg = n.z >= 0 ? 1 : -1
 *     a  = -1 / (sg + n.z)
 *     b  = (n.x * n.y) * a
 *     T  = (1 + ((sg * n.x) * n.x) * a,  sg * b,  (-sg) * n.x)
 *     B  = (b,  sg + (n.y * n.y) * a,  -n.y)
 *   Sample j of point i:
 *     (lx, ly, lz) = dirs[dir_first + j]
 *     rx = c * lx - s * ly
 *     ry = s * lx + c * ly          (without a rotation array: rx = lx, ry = ly, and no operation is performed)
 *     d  = ((T * rx) + (B * ry)) + n * lz        componentwise
 *     o  = p + n * bias                          componentwise
 *   Occlusion: sample j is occluded iff rayca_hip_query_device(RAYCA_QUERY_OCCLUDED) reports 1 for the ray (o, d) with tmax = the
 *   point's radius: the same traversal, the same strict t < tmax, +inf / FLT_MAX unbounded, a radius that is NaN or <= 0 never
 *   occluded.  t is the ray parameter: a distance only as far as |d| is 1.
 *   Inactive points: a point is inactive iff n.x == 0 && n.y == 0 && n.z == 0, or any of the six inputs p, n is not finite.  (The
 *   zero test is what rayca_hip_surface_device writes for a miss: a G-buffer goes in as it is.)  An inactive point traces nothing
 *   and has every sample unoccluded.
 *   Outputs (any may be NULL, not all), per point:
 *     mask_out  u64      bit j = sample j occluded
 *     hits_out  u32      popcount of the mask
 *     open_out  f32      float(S - hits) / float(S)
 *     bent_out  3 x f32  acc = 0; for j ascending: if not occluded, acc = acc + d_j  (unnormalised: the caller normalises)
 *   An inactive point gives mask 0, hits 0, open 1, bent 0.  Results do not depend on the order in which rays are traced: the
 *   mask is assembled with integer OR only, and bent is summed from the finished mask in j order.
 * opts (may be NULL): stream, context, wait_event, record_event and collect_stats as for rayca_hip_query_device; traversal must be
 * RAYCA_TRAVERSAL_ORDERED (RAYCA_ERR_UNSUPPORTED for EXHAUSTIVE, as for an OCCLUDED query); tile, engine and camera_rays must be
 * zero.  Ordered on its context like a query.  Without mask_out the mask words live in the context's work buffers.  With
 * stats_out the call waits: rays_shadow = count x S, the time (clearing the mask words included) under RAYCA_KERNEL_OTHER,
 * kernel_launches = the kernels launched (the trace kernel, and the fold unless mask_out is the only output), boxes_tested and
 * triangles_tested under collect_stats.  count == 0 is RAYCA_OK and launches nothing; nothing outside [0, count) of an output is
 * written.  Scenes with spheres are served.
 * Refusals, before any GPU work and before the scene is looked at, in this order.  RAYCA_ERR_BAD_ARG: NULL scene / struct; NULL
 * points, normals, dirs; samples 0 or > 64; dir_first + samples > dir_count; non-zero reserved; no output; mask_out not aligned to
 * 8 bytes; bias not finite; count x samples >= 2^32; then context > 7, a non-zero field of opts that does not apply.  Then
 * RAYCA_ERR_UNSUPPORTED for EXHAUSTIVE.  Then (count != 0) RAYCA_ERR_EMPTY_SCENE as the query. */
struct RaycaAmbient {
  uint32_t count;
  uint32_t samples;       /* S: 1 .. 64 */
  const void* points;     /* DEVICE: count x 3 f32 */
  const void* normals;    /* DEVICE: count x 3 f32; (0, 0, 0) marks an inactive point */
  const void* rotations;  /* DEVICE: count x 2 f32 (cos, sin), or NULL => no rotation */
  const void* radius;     /* DEVICE: count f32, or NULL => radius_all for every point */
  const void* dirs;       /* DEVICE: dir_count x 3 f32 local directions, z along the normal */
  uint32_t dir_count;
  uint32_t dir_first;     /* sample j takes dirs[dir_first + j] */
  float radius_all;
  float bias;             /* o = p + n * bias; finite */
  uint32_t reserved;      /* must be zero */
  void* mask_out;         /* DEVICE: count u64, aligned to 8 bytes */
  void* hits_out;         /* DEVICE: count u32 */
  void* open_out;         /* DEVICE: count f32 */
  void* bent_out;         /* DEVICE: count x 3 f32 */
};
typedef struct RaycaAmbient RaycaAmbient;
int32_t rayca_hip_ambient_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaAmbient* ambient,
                                 RaycaStats* stats_out);

/* Surface records for hit records, on DEVICE memory: what is AT a hit, where rayca_hip_query_device says where the hit is.  Per
 * record (the ray, t, prim, u, v exactly as RAYCA_QUERY_CLOSEST writes them) the values a render kernel has in hand at the same
 * hit, bit for bit -- one function computes both:
 *   point     Hit.point: o + d * t (triangle.rs:122); a sphere's is its model-space hit taken back to the world (sphere.rs:155-163)
 *   normal    the shading normal: vertex normals interpolated and normalised (primitive.rs:172-182), the material's normal map
 *             applied (material/mod.rs:125-139, pbr.rs:104-123); a sphere's normal (primitive.rs:183-190)
 *   color     get_color(): geometry colour x Material::get_color (primitive.rs:142-148, material/mod.rs:107-113) -- what Flat shows
 *   diffuse   get_diffuse() (primitive.rs:150-155);  specular  get_specular() (material/mod.rs:141-151)
 *   rough     get_roughness() (material/mod.rs:173-185) and the material's shininess
 *   material  the primitive's material index, RAYCA_NONE for Material::DEFAULT
 *   flags     bits 0-1: RAYCA_MATERIAL_* of that material, bit 2: it is emissive (material/phong.rs:54-56), bit 3: the primitive
 *             is a sphere, bit 31: the record is a hit
 * Sphere::intersects builds its Hit from the inverse-transformed ray (sphere.rs:138,157-159); `point` and `normal` of a sphere are
 * derived from that model-space hit the way the render kernels derive them, so `point` is o + d * t only up to the rounding of the
 * trip through model space.
 * A record whose prim is RAYCA_NONE, or not below the scene's primitive count, is a miss and reads nothing of the scene: zeros in
 * every float output, RAYCA_NONE in material_out, 0 in flags_out.  Any output may be NULL, not all; when only color, material and
 * flags are asked for, nothing behind get_color() is evaluated (as for a Flat frame).  `rays` is required when point_out or
 * normal_out is asked for, else it may be NULL.  Nothing outside [0, count) of an output is written; count == 0 is RAYCA_OK and
 * launches nothing (the pointers of an empty batch are not looked at; opts and reserved are checked as always).  Outputs need only their elements' 4-byte alignment (16-byte aligned colour outputs are written 16 bytes a lane).
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event as
 * for rayca_hip_query_device; every other field must be zero.  Calls on one context are serialised with that context's frames and
 * queries on the device, calls on different contexts overlap; records issued after a rayca_hip_scene_update see the new
 * materials.  With stats_out the call waits: the kernel's time under RAYCA_KERNEL_OTHER, kernel_launches = 1.
 * RAYCA_ERR_BAD_ARG (before any GPU work): NULL scene / query, non-zero reserved, NULL t / prim / uv, NULL rays with point_out or
 * normal_out, no output, context > 7, a non-zero field of opts that does not apply.  RAYCA_ERR_EMPTY_SCENE as the query. */
struct RaycaSurfaceQuery {
  uint32_t count;
  uint32_t reserved;      /* must be zero */
  const void* rays;       /* DEVICE: count x 6 f32, the rays the hit records belong to */
  const void* t;          /* DEVICE: count f32 */
  const void* prim;       /* DEVICE: count u32, post-build primitive order */
  const void* uv;         /* DEVICE: count x 2 f32 */
  void* point_out;        /* DEVICE: count x 3 f32 */
  void* normal_out;       /* DEVICE: count x 3 f32 */
  void* color_out;        /* DEVICE: count x 4 f32 */
  void* diffuse_out;      /* DEVICE: count x 4 f32 */
  void* specular_out;     /* DEVICE: count x 4 f32 */
  void* rough_out;        /* DEVICE: count x 2 f32 (roughness, shininess) */
  void* material_out;     /* DEVICE: count u32 */
  void* flags_out;        /* DEVICE: count u32 */
};
typedef struct RaycaSurfaceQuery RaycaSurfaceQuery;
int32_t rayca_hip_surface_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaSurfaceQuery* query,
                                 RaycaStats* stats_out);

/* The camera rays a frame traces (scene.rs:117-141 + trs.rs:275-284 + ray.rs:74-91), to DEVICE memory: for camera_draw_infos[0]
 * the ray of sub-sample `sample` (< cfg->samples_per_pixel, else RAYCA_ERR_BAD_ARG) of every pixel, 6 f32 each (origin xyz,
 * direction xyz -- the layout rayca_hip_query_device reads), the bits the render kernels trace for the same width, height and
 * cfg->samples_per_pixel: the sub-pixel position is (x + ix * step) + offset in the reference's association (scene.rs:125-137).
 * Rows are packed as opts->tile says (all zero => the whole frame): rayca_hip_tile_rows(tile, height) x width rays are written.
 * Of cfg only samples_per_pixel is read.  opts (may be NULL): tile, stream (NULL => the context's own stream, and the call waits
 * for it), context, wait_event, record_event; traversal, collect_stats, engine and camera_rays must be zero.  Ordered on its
 * context like a frame.  RAYCA_ERR_NO_CAMERA and RAYCA_ERR_BAD_ARG (empty image, tile.part >= tile.parts, context > 7) as for a
 * render call. */
int32_t rayca_hip_camera_rays_device(RaycaScene* scene, const RaycaConfig* cfg, uint32_t width, uint32_t height, uint32_t sample,
                                     const RaycaRenderOptions* opts, void* d_rays_out);

/* Radiance along caller-supplied rays, on DEVICE memory: what light arrives along ray i, where rayca_hip_query_device says where
 * the ray hits.  out[i] is what the pixel of a one-sample frame of `cfg` receives whose camera ray is rays[i] and whose index
 * y * width + x is first_index + i: Integrator::trace on the ray (integrator/flat.rs:16-28, pathtracer.rs:68-106), BLACK + colour
 * (scene.rs:143-145), cfg->gamma and the quantisation of a render call (scene.rs:146-148).  The path of ray i draws its random
 * numbers from the stream of (cfg->seed, pixel index first_index + i, sample).  Hence, bit for bit:
 *   a frame   rays = rayca_hip_camera_rays_device(cfg with samples_per_pixel 1, w, h, sample 0), count = w * h, sample = 0,
 *             first_index = 0: both outputs equal rayca_hip_render_device(cfg, w, h)'s, on either engine, and rays_shadow,
 *             rays_bounce and (with collect_stats) hits_shaded of RaycaStats equal the frame's; rays_primary = count.
 *   chunks    any split of a ray set into consecutive calls, each with the first_index of its first ray, writes what one call does.
 *   Flat      (no random numbers) depends on the ray alone: on a hit r, g, b are 0 + rayca_hip_surface_device's `color` for the
 *             record rayca_hip_query_device returns for the ray, a miss is a render's miss pixel; a degenerate ray (NaN, zero
 *             direction) is shaded as whatever the query says of it.
 * Several samples are several calls with different `sample`, folded by the caller (e.g. rayca_hip_accumulate_device).
 * Configs: those the generation kernels render -- Flat; Pathtracer with direct sampler NEE or NONE, indirect sampler COSINE or
 * HEMISPHERE, no Russian roulette, and light_samples == 1 where the path bounces.  Everything else is RAYCA_ERR_UNSUPPORTED with
 * the field named in rayca_hip_last_error: the per-pixel stack machine has no ray-fed form.  cfg->samples_per_pixel and cfg->bvh
 * are not read.  No camera is needed.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event and
 * collect_stats as for rayca_hip_render_device; tile, engine and camera_rays must be zero, RAYCA_TRAVERSAL_EXHAUSTIVE is
 * RAYCA_ERR_UNSUPPORTED.  The call is ordered on its context like a frame and uses that context's work buffers (ray queues,
 * per-depth path records: 32 B a ray per queue, 36 B a ray and depth); calls and frames on different contexts overlap.  It is
 * asynchronous unless stats_out is given; then it waits and fills RaycaStats as a frame of the wavefront engine does, the pass
 * that queues the rays under RAYCA_KERNEL_OTHER, rows_rendered = 1.  Nothing outside [0, count) of an output is written.
 * Checked first, from the structs alone and in this order, as RAYCA_ERR_BAD_ARG: NULL scene / cfg / radiance, first_index + count
 * above 2^32 (or count above 2^31), non-zero reserved, NULL rays, no output, rgba32f_out not 16-byte aligned, unknown integrator or
 * sampler, light_samples == 0, then opts: context > 7, a non-zero field that does not apply.  Then RAYCA_ERR_UNSUPPORTED for the
 * traversal and the Config.  count == 0 is then RAYCA_OK and launches nothing.  Then the scene: RAYCA_ERR_EMPTY_SCENE as for a
 * query, RAYCA_ERR_UNSUPPORTED for a directional light under NEE (nee.rs:178). */
struct RaycaRadiance {
  uint32_t count;        /* rays */
  uint32_t sample;       /* RNG stream of the paths: ray i draws from rng_root(cfg->seed, first_index + i, sample) */
  uint32_t first_index;  /* the "pixel index" of ray 0; first_index + count <= 2^32 */
  uint32_t reserved;     /* must be zero */
  const void* rays;      /* DEVICE: count x 6 f32 (origin xyz, direction xyz; the direction need not be normalised) */
  void* rgba32f_out;     /* DEVICE: count x 4 f32, or NULL; 16-byte aligned */
  void* rgba8_out;       /* DEVICE: count x 4 u8, or NULL; not both NULL */
};
typedef struct RaycaRadiance RaycaRadiance;
int32_t rayca_hip_radiance_device(RaycaScene* scene, const RaycaConfig* cfg, const RaycaRenderOptions* opts, const RaycaRadiance* radiance,
                                  RaycaStats* stats_out);

/* Irradiance gathering on DEVICE memory: the light that arrives AT `count` caller-supplied points -- the radiance along `samples`
 * rays over the hemisphere (or, with a table that covers it, the sphere) of each point's normal, folded into one irradiance record
 * and nine spherical-harmonic coefficients per point: lightmap baking, irradiance probes, a final gather on a G-buffer.  The rays
 * are rayca_hip_ambient_device's, made in registers; the radiance is rayca_hip_radiance_device's, run by the same frame driver; the
 * fold has a fixed order.  No ray buffer is written or read, and the per-ray radiance is held for one internal frame at a time.
 *
 * The specification, in f32 with every operation rounded on its own.
 *   Rays.  Ray j of point i is sample j of point i of RaycaAmbient's comment, word for word: the same frame (T, B), the same
 *   rotation (c, s) -- without a rotation array rx = lx, ry = ly and no operation is performed --, the same
 *     d  = ((T * rx) + (B * ry)) + n * lz        with (lx, ly, lz) = dirs[dir_first + j]
 *     o  = p + n * bias
 *   (one function makes both calls' rays).  A point is inactive by the same rule: n.x == 0 && n.y == 0 && n.z == 0, or any of the
 *   six inputs p, n not finite.  There is no radius.  Keeping d unit is the caller's business: unit normals and unit dirs.
 *   Radiance.  L(i, j) is, bit for bit, what rayca_hip_radiance_device writes to rgba32f_out for the ray (o, d), the same cfg and
 *   `sample`, and the pixel index first_index + i * S + j (the path draws from the stream of (cfg->seed, that index, sample)).
 *   The Configs of that call are served, with its refusals; in addition cfg->gamma must be exactly 1 (a mean of gamma-encoded
 *   values means nothing): RAYCA_ERR_UNSUPPORTED naming RaycaConfig.gamma otherwise.
 *   Fold, per point, j ascending:
 *     kept = 0; E = (0, 0, 0); H[k] = (0, 0, 0) for k = 0 .. 8
 *     sample j counts iff L.r, L.g and L.b are all finite (x - x == 0 for each: a NaN or infinite sample stays out)
 *     for a sample that counts:
 *       c    = w[dir_first + j] * L     per r, g, b   (without `weights`: c = L, and no operation is performed)
 *       E    = E + c
 *       H[k] = H[k] + c * Y_k(d_j)      k = 0 .. 8, d_j the traced direction
 *       kept = kept + 1
 *     Y0 = 0.2820948f                    Y1 = 0.4886025f * d.y              Y2 = 0.4886025f * d.z
 *     Y3 = 0.4886025f * d.x              Y4 = 1.0925484f * (d.x * d.y)      Y5 = 1.0925484f * (d.y * d.z)
 *     Y6 = 0.3153916f * ((3.0f * (d.z * d.z)) - 1.0f)
 *     Y7 = 1.0925484f * (d.x * d.z)      Y8 = 0.5462742f * ((d.x * d.x) - (d.y * d.y))
 *     kept > 0: E = E / float(kept), H[k] = H[k] / float(kept), componentwise; otherwise they stay 0
 *   Outputs (any may be NULL, not all), per point:
 *     irradiance_out  4 x f32      (E.r, E.g, E.b, float(kept) / float(S))
 *     sh_out          9 x 4 x f32  [k] = (H[k].r, H[k].g, H[k].b, 0)
 *     kept_out        u32          kept
 *     samples_out     S x 4 x f32  L(i, j) itself, as the radiance call writes it
 *   An inactive point gives zeros everywhere, its S rows of samples_out included.  With cosine-distributed dirs and no weights E is
 *   the irradiance / pi; any other scale (a solid-angle weight for a uniform table, say) is the caller's, through `weights`.
 *   Inactive points in the queue: their S slots are queued as the ray o = d = (0, 0, 0), traced and shaded like any degenerate ray
 *   of a radiance call, and the result is discarded -- the queue of an internal frame is dense, entry = i * S + j.  Hence
 *   RaycaStats.rays_primary = count x S, inactive points included.
 *   Chunks.  The call runs whole points per internal frame: at most 2^22 rays a frame (at least one point), and at most
 *   chunk_points points where that is not zero.  The per-ray radiance lives in samples_out when given, else in a scratch of the
 *   frame context sized by the chunk, not by count x S.  The radiance call's results do not depend on chunking (its "chunks"
 *   above), and a point's fold reads its own S records alone, so every output is the same bits for every chunk_points.
 * opts (may be NULL), ordering and statistics as for rayca_hip_radiance_device: stream, context, wait_event, record_event,
 * collect_stats; tile, engine and camera_rays must be zero; ordered on its context like a frame; asynchronous unless stats_out is
 * given.  RaycaStats are a wavefront frame's, summed over the internal frames (node_format: ORed; rows_rendered: the number of
 * frames); the pass that queues the rays and the fold are under RAYCA_KERNEL_OTHER.  count == 0 is RAYCA_OK and launches nothing;
 * nothing outside [0, count) of an output is written.
 * Refusals, before any GPU work and before the scene is looked at, in this order.  RAYCA_ERR_BAD_ARG: NULL scene / cfg / struct;
 * NULL points, normals, dirs; samples 0 or > 64; dir_first + samples > dir_count; non-zero reserved; no output; irradiance_out,
 * sh_out or samples_out not 16-byte aligned; bias not finite; first_index + count x S above 2^32, or count x S above 2^31; then
 * the Config as the radiance call checks it (unknown integrator or sampler, light_samples == 0); then opts: context > 7, a
 * non-zero field that does not apply.  Then RAYCA_ERR_UNSUPPORTED: RAYCA_TRAVERSAL_EXHAUSTIVE, the Configs the radiance call
 * does not serve, gamma != 1.  count == 0 is then RAYCA_OK.  Then the scene: RAYCA_ERR_EMPTY_SCENE, RAYCA_ERR_UNSUPPORTED for a
 * directional light under NEE, as the radiance call. */
struct RaycaGather {
  uint32_t count;         /* points */
  uint32_t samples;       /* S: 1 .. 64 rays a point */
  const void* points;     /* DEVICE: count x 3 f32 */
  const void* normals;    /* DEVICE: count x 3 f32; (0, 0, 0) marks an inactive point (a G-buffer's miss) */
  const void* rotations;  /* DEVICE: count x 2 f32 (cos, sin), or NULL => no rotation */
  const void* dirs;       /* DEVICE: dir_count x 3 f32 local directions, z along the normal */
  const void* weights;    /* DEVICE: dir_count f32, or NULL => no weighting */
  uint32_t dir_count;
  uint32_t dir_first;     /* sample j takes dirs / weights [dir_first + j] */
  float bias;             /* o = p + n * bias; finite */
  uint32_t sample;        /* RNG stream of the paths, as RaycaRadiance.sample */
  uint32_t first_index;   /* ray (i, j) is "pixel" first_index + i * S + j of a radiance call */
  uint32_t chunk_points;  /* 0: the library's choice; else at most this many points per internal frame */
  uint32_t reserved[2];   /* must be zero */
  void* irradiance_out;   /* DEVICE: count x 4 f32, 16-byte aligned, or NULL */
  void* sh_out;           /* DEVICE: count x 9 x 4 f32, 16-byte aligned, or NULL */
  void* kept_out;         /* DEVICE: count u32, or NULL */
  void* samples_out;      /* DEVICE: count x S x 4 f32, 16-byte aligned, or NULL */
};
typedef struct RaycaGather RaycaGather;
int32_t rayca_hip_gather_device(RaycaScene* scene, const RaycaConfig* cfg, const RaycaRenderOptions* opts, const RaycaGather* gather,
                                RaycaStats* stats_out);

/* Irradiance volumes on DEVICE memory: the diffuse light at `count` caller-supplied points from a regular grid of SH9 probes -- the
 * nine-coefficient records rayca_hip_gather_device writes to sh_out for points at the probes' centres.  The eight probes of a
 * point's cell are blended by trilinear weight, by a wrapped normal term and, when asked for, by one short occlusion ray per probe,
 * so that light does not leak through walls; the blend is evaluated as the irradiance at the point's normal (Ramamoorthi and
 * Hanrahan 2001).  The rays are made in registers inside the traversal kernel: no ray buffer.  Asynchronous on the caller's stream.
 *
 * The specification, in f32 with every operation rounded on its own: + - * /, floor, min, max (maxNum), |x|, comparisons, selects
 * and integers; no square root, no trigonometry.
 *   Grid.  origin g (3 f32, finite), cell h (3 f32, finite, > 0), dims (nx, ny, nz), each >= 1, product <= 2^24.  Probe (ix, iy, iz)
 *   has index m = (iz * ny + iy) * nx + ix and centre c = g + float(i) * h per axis: one multiply, one add.  sh: M x 9 x 4 f32,
 *   exactly RaycaGather.sh_out's layout; .w is ignored.  kept: M u32 (RaycaGather.kept_out) or NULL; a probe with kept[m] == 0 is
 *   invalid.  Non-finite coefficients of a valid probe are the caller's business and propagate.
 *   Points.  points and normals are RaycaAmbient's, with the same inactive rule: n.x == 0 && n.y == 0 && n.z == 0, or any of the six
 *   values not finite.  Unit normals are expected and not checked.
 *   Cell, per axis a:
 *     f  = (p.a - g.a) / h.a
 *     f  = min(max(f, 0), float(dim_a - 1))
 *     i0 = min(uint(floor(f)), dim_a >= 2 ? dim_a - 2 : 0)
 *     t  = f - float(i0)
 *     i1 = min(i0 + 1, dim_a - 1)
 *   A point outside the grid takes the nearest boundary cell.
 *   Corners.  k = 0 .. 7 with bits bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1.  The index on an axis is b ? i1 : i0, the axis
 *   weight b ? t : 1 - t;  wt_k = (wx * wy) * wz.  Corner k is a candidate iff wt_k > 0 and its probe is valid.
 *   Visibility (flags & RAYCA_PROBE_VISIBILITY).
 *     o = p + n * bias,  d = c_k - o            componentwise
 *   A candidate corner is occluded iff rayca_hip_query_device(RAYCA_QUERY_OCCLUDED) reports 1 for the ray (o, d) with tmax = 1: the
 *   same traversal, the same strict t < tmax.  Corners that are not candidates trace nothing.
 *   Normal term (flags & RAYCA_PROBE_NORMAL_TERM).
 *     v  = c_k - p
 *     s  = (v.x * n.x + v.y * n.y) + v.z * n.z
 *     l2 = (v.x * v.x + v.y * v.y) + v.z * v.z
 *     q  = l2 > 0 ? (s * |s|) / l2 : 1
 *     wb = (q + 1) * 0.5
 *     wb = wb * wb + 0.0625f
 *   A signed squared cosine, wrapped.  Without the flag the term is absent and no operation is performed.
 *   Blend, for k ascending.  w_k = wt_k, times wb when the normal term is on.  A corner counts iff it is a candidate, is not
 *   occluded, and w_k > 0 (a NaN weight fails the comparison).  For a counting corner:
 *     wsum = wsum + w_k;  H[j] = H[j] + w_k * sh[m_k][j]    j = 0 .. 8, per r, g, b       (wsum and H from 0)
 *   Fallback.  If wsum is not > 0 and either flag is on: the blend is run again from wsum = 0, H = 0 over the candidates with
 *   w_k = wt_k alone, and the point is marked as a fallback (also when it has no candidate at all).
 *   If wsum > 0 after either pass: H[j] = H[j] / wsum.  Otherwise H = 0 and wsum = 0.
 *   Evaluate.  b_j = A_l(j) * Y_j(n), Y_j written exactly as in RaycaGather's comment with d = n; A = 3.1415927f for j = 0,
 *   2.0943952f for j = 1 .. 3, 0.7853982f for j = 4 .. 8.
 *     E = 0;  E = E + b_j * H[j]  for j ascending, per channel;  then E = max(E, 0)
 *   Outputs (any may be NULL, not all), per point:
 *     irradiance_out  4 x f32      (E.r, E.g, E.b, wsum)
 *     sh_out          9 x 4 x f32  the blended H, w = 0
 *     mask_out        u32          bits 0..7 the candidate corners, bits 8..15 the occluded corners, bit 16 the fallback
 *     radiance_out    4 x f32      L = albedo * (E * 0.31830987f) per r, g, b, then + base when given; alpha = base.a, or 1
 *   radiance_out needs albedo (count x 4 f32: a surface call's color or diffuse output) and optionally base (a direct-light frame).
 *   An inactive point gives zeros; its radiance_out is base's pixel, or (0, 0, 0, 1) without base.
 *   Order-free results: the trace kernel only ORs bit 8 + k of the point's mask word, with a 32-bit atomic; everything else is
 *   made from the finished word, in k order.
 * opts (may be NULL), ordering and statistics as for rayca_hip_ambient_device: stream, context, wait_event, record_event and
 * collect_stats; traversal must be RAYCA_TRAVERSAL_ORDERED; tile, engine and camera_rays must be zero.  Without mask_out the mask
 * words live in the context's work buffers.  With stats_out the call waits: rays_shadow = count x 8 with RAYCA_PROBE_VISIBILITY and
 * 0 without, the time and the launches (the trace kernel with visibility, and the fold) under RAYCA_KERNEL_OTHER, boxes_tested and
 * triangles_tested under collect_stats.  Nothing outside [0, count) of an output is written.  Scenes with spheres are served.
 * Refusals, before any GPU work and before the scene is looked at, in this order.  RAYCA_ERR_BAD_ARG: NULL scene / struct; NULL
 * points, normals, sh; unknown flag bits; a zero dim; dims product > 2^24; cell not finite or not > 0; origin not finite; bias not
 * finite; non-zero reserved; no output; radiance_out without albedo; irradiance_out, sh_out, radiance_out, albedo, base or sh not
 * 16-byte aligned, mask_out not 4-byte aligned; count x 8 >= 2^32; then context > 7, a non-zero field of opts that does not apply.
 * Then RAYCA_ERR_UNSUPPORTED for EXHAUSTIVE.  count == 0 is then RAYCA_OK and launches nothing.  Then, only with
 * RAYCA_PROBE_VISIBILITY, RAYCA_ERR_EMPTY_SCENE as the query: without the flag the scene is not read and an empty scene is no error. */
enum { RAYCA_PROBE_VISIBILITY = 1, RAYCA_PROBE_NORMAL_TERM = 2 };
struct RaycaProbeLookup {
  uint32_t count;         /* points */
  uint32_t flags;         /* RAYCA_PROBE_* */
  float origin[3];        /* g: the centre of probe (0, 0, 0); finite */
  float cell[3];          /* h: the spacing per axis; finite, > 0 */
  uint32_t dims[3];       /* nx, ny, nz: each >= 1, product <= 2^24 */
  float bias;             /* o = p + n * bias; finite */
  uint32_t reserved[2];   /* must be zero */
  const void* points;     /* DEVICE: count x 3 f32 */
  const void* normals;    /* DEVICE: count x 3 f32; (0, 0, 0) marks an inactive point (a G-buffer's miss) */
  const void* sh;         /* DEVICE: M x 9 x 4 f32, 16-byte aligned: RaycaGather.sh_out of the probes */
  const void* kept;       /* DEVICE: M u32 (RaycaGather.kept_out), or NULL => every probe is valid */
  const void* albedo;     /* DEVICE: count x 4 f32, 16-byte aligned, or NULL; required by radiance_out */
  const void* base;       /* DEVICE: count x 4 f32, 16-byte aligned, or NULL */
  void* irradiance_out;   /* DEVICE: count x 4 f32, 16-byte aligned, or NULL */
  void* sh_out;           /* DEVICE: count x 9 x 4 f32, 16-byte aligned, or NULL */
  void* mask_out;         /* DEVICE: count u32, or NULL */
  void* radiance_out;     /* DEVICE: count x 4 f32, 16-byte aligned, or NULL */
};
typedef struct RaycaProbeLookup RaycaProbeLookup;
int32_t rayca_hip_probe_lookup_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaProbeLookup* lookup,
                                      RaycaStats* stats_out);

/* Direct light at points on DEVICE memory: the light that arrives at `count` caller-supplied points straight from the scene's point
 * and quad lights -- the next-event-estimation sum of a path vertex (sampler/nee.rs:72-166) with the BRDF taken out, for points
 * that are no path vertices: the points of rayca_hip_surface_sample_device, mesh vertices, lightmap texels, the centres of a probe
 * grid, a G-buffer.  rayca_hip_gather_device never sees a point light (a hemisphere ray hits surfaces, not points); this call is
 * the other half of a bake.  The shadow rays are made in registers inside the traversal kernel: no ray buffer, no per-sample
 * intermediate.  Asynchronous on the caller's stream.
 *
 * The specification, in f32 with every operation rounded on its own.  Vectors are (x, y, z); dot(a, b) is
 * (((-0.0f + a.x * b.x) + a.y * b.y) + a.z * b.z) + 0.0f, the ordered four-lane sum of rayca-math with a zero w lane;
 * |a|^2 = dot(a, a), |a| = sqrt(|a|^2); normalized(a) = a / |a| per component when |a| > 2^-10, else a itself.  A light is the
 * record rayca_hip_scene_read_lights returns (position: the translation of the light's node-LOCAL transform, as the reference).
 *   Samples.  Sample j = (li - light_first) * light_samples + k for li in [light_first, light_first + light_count) and
 *   k < cfg->light_samples; N = light_count * light_samples must be 1 .. 64, one bit of the mask word each.  Callers with more
 *   lights chunk over light ranges: a sample does not depend on the range it is asked in.
 *   Modes.  With normals (hemisphere mode): o = p + n * bias per component (one multiply, one add); bias = 1e-4f, the reference's
 *   ray bias, reproduces a path vertex.  A point is inactive iff n.x == 0 && n.y == 0 && n.z == 0, or any of the six values is not
 *   finite (RaycaAmbient's rule).  Without normals (sphere mode): o = p, bias must be 0, and a point is inactive iff a coordinate
 *   is not finite.
 *   Point light (kind RAYCA_LIGHT_POINT), with x1 = position:
 *     v      = x1 - p                        dist = |v|        omega = normalized(v)
 *     w      = p - x1                        r2 = |w|^2        rr = sqrt(r2)
 *     fallof = (((-0.0f + att[0] * 1.0f) + att[1] * rr) + att[2] * r2) + 0.0f
 *     le     = (intensity * color.rgb) / fallof            alpha = color.a
 *     d_omega = 1.0f / |v|^2
 *   (le carries the reference's own 1 / fallof and d_omega its extra 1 / r^2).
 *   Quad light (any other kind that is served), with key = rng_root(cfg->seed, (first_index + i) mod 2^32, sample) -- the stream
 *   RaycaRadiance and RaycaSurfaceSample name -- and the random dimension D = 2 * (q(li) * light_samples + k), q(li) the number of
 *   quad lights of the WHOLE scene with an index below li (where a path vertex's dimension stands: with first_index + i a pixel
 *   index the draws are that pixel's generation-0 draws):
 *     sc = float(strate_count)               strate_count = light_stratify ? uint(sqrt(float(light_samples))) : 1
 *     u1 = rng_f32(key, D) / sc              u2 = rng_f32(key, D + 1) / sc
 *     x1 = (position + u1 * ab) + u2 * ac
 *     with light_stratify:  x1 = x1 + ((ab / sc) * float(k % strate_count) + (ac / sc) * float(k / strate_count))
 *     v      = x1 - p                        omega = normalized(v)
 *     le     = (intensity * color.rgb) * area              alpha = color.a
 *     d_omega = dot(normal, omega) / |v|^2
 *   (the reference's unnegated dot: the light counts from the side its normal points AWAY from, and negatively from the other).
 *   Contribution.  Hemisphere mode: ndot = clamp(dot(n, omega), 0, 1) (a NaN stays NaN) and x = (le * ndot) * d_omega per r, g, b.
 *   Sphere mode: x = le * d_omega.  y = x * alpha per r, g, b: what the reference's Color `+` adds.
 *   Classes.  A sample is dropped iff a component of y is not finite (a point on the light, say): it is neither traced nor added --
 *   a path vertex's pixel would be NaN; here "a NaN sample stays out", as in rayca_hip_gather_device.  A sample is void iff it is not
 *   dropped and y.r == 0 && y.g == 0 && y.b == 0 (it faces away, the intensity is 0, it underflowed): not traced, never lit; adding
 *   it would change no bit.  Every other sample is traced along the ray (o, omega).
 *   Lit.  Point light: lit iff rayca_hip_query_device(RAYCA_QUERY_OCCLUDED) reports 0 for (o, omega) with tmax = dist.  Quad light:
 *   lit iff RAYCA_QUERY_CLOSEST, unbounded, finds a hit whose material is emissive (bit 2 of rayca_hip_surface_device's flags): the
 *   reference's "lit iff the closest hit is emissive" (nee.rs:103-104).  Scenes with spheres are served, as by both queries.
 *   Fold, per point, j ascending over the lit samples, from zeros:
 *     hemisphere mode   E = E + y
 *     sphere mode       I = I + y;  with sh_out  H[k] = H[k] + y * Y_k(omega), k = 0 .. 8, Y_k exactly the nine expressions of
 *                       RaycaGather's comment with d = omega.  There is no division by a count.
 *   Outputs (any may be NULL, not all), per point:
 *     irradiance_out  4 x f32      hemisphere mode (E.r, E.g, E.b, float(lit) / float(N)); sphere mode (I.r, I.g, I.b, the same)
 *     sh_out          9 x 4 x f32  sphere mode only: [k] = (H[k].r, H[k].g, H[k].b, 0)
 *     mask_out        u64          bit j = sample j was traced and lit
 *     counts_out      u32          lit samples in the low 16 bits, dropped samples in the high 16
 *   An inactive point gives zeros everywhere.  Nothing outside [0, count) of an output is written.
 *   Units.  Hemisphere E is the irradiance (not / pi): a Lambert surface of albedo a radiates a * E / pi.  Sphere I is the incident
 *   radiance times solid angle, and sh_out is the integral of L Y_k over the sphere of the direct light: the units of
 *   rayca_hip_gather_device's sh_out under a uniform sphere table with weights of 4 pi, so the two add into one probe.
 *   Order-free results: the trace kernel only ORs bit j of the point's mask word, with a 64-bit atomic; everything else is made
 *   from the finished word, in j order.
 * Of cfg only light_samples, light_stratify and seed are read.  opts (may be NULL), ordering and statistics as for
 * rayca_hip_ambient_device: stream, context, wait_event, record_event and collect_stats; traversal must be RAYCA_TRAVERSAL_ORDERED;
 * tile, engine and camera_rays must be zero.  Without mask_out the mask words live in the context's work buffers.  With stats_out
 * the call waits: rays_shadow = the samples that were traced, the time and the launches (the trace kernel, and the fold unless
 * mask_out is the only output) under RAYCA_KERNEL_OTHER, boxes_tested and triangles_tested under collect_stats.
 * Refusals, before any GPU work and before the scene is looked at, in this order.  RAYCA_ERR_BAD_ARG: NULL scene / cfg / struct; NULL
 * points; light_count == 0; cfg->light_samples == 0, or N > 64; non-zero reserved; no output; sh_out with normals; a non-zero bias
 * without normals; irradiance_out or sh_out not 16-byte aligned, mask_out not 8-byte aligned, counts_out not 4-byte aligned; bias not
 * finite; first_index + count above 2^32; count x N >= 2^32; then context > 7, a non-zero field of opts that does not apply.  Then
 * RAYCA_ERR_UNSUPPORTED for EXHAUSTIVE.  count == 0 is then RAYCA_OK and launches nothing.  Then the scene: RAYCA_ERR_EMPTY_SCENE;
 * RAYCA_ERR_BAD_ARG for light_first + light_count above the scene's lights; RAYCA_ERR_UNSUPPORTED for a directional light in the
 * range (the reference's todo!() at nee.rs:178, as in the radiance call). */
struct RaycaDirect {
  uint32_t count;         /* points */
  uint32_t light_first;   /* the first light of the range */
  uint32_t light_count;   /* lights in the range: light_count * cfg->light_samples is 1 .. 64 */
  uint32_t sample;        /* RNG stream of the quad-light draws, as RaycaRadiance.sample */
  uint32_t first_index;   /* point i draws from the stream of "pixel" first_index + i */
  float bias;             /* hemisphere mode: o = p + n * bias; finite; sphere mode: must be 0 */
  uint32_t reserved[2];   /* must be zero */
  const void* points;     /* DEVICE: count x 3 f32 */
  const void* normals;    /* DEVICE: count x 3 f32, (0, 0, 0) marks an inactive point; or NULL => sphere mode */
  void* irradiance_out;   /* DEVICE: count x 4 f32, 16-byte aligned, or NULL */
  void* sh_out;           /* DEVICE: count x 9 x 4 f32, 16-byte aligned, or NULL; sphere mode only */
  void* mask_out;         /* DEVICE: count u64, or NULL */
  void* counts_out;       /* DEVICE: count u32, or NULL */
};
typedef struct RaycaDirect RaycaDirect;
int32_t rayca_hip_direct_device(RaycaScene* scene, const RaycaConfig* cfg, const RaycaRenderOptions* opts, const RaycaDirect* direct,
                                RaycaStats* stats_out);

/* The edge-avoiding a-trous wavelet denoiser, on a frame and its G-buffer in DEVICE memory: what rayca_hip_render_device wrote to
 * d_rgba32f_out (rendered with gamma 1) and what rayca_hip_surface_device wrote for the frame's camera rays go in, the filtered
 * frame comes out as RGBA32F and / or RGBA8, through the gamma and the quantisation of a render call.  No reference counterpart.
 * The scene handle gives the call its device and its frame context (stream, scratch images, ordering); the scene is not read, and
 * an empty scene is no error.  Everything is f32, every operation rounds once, in the association written here (no exp, no pow
 * inside the filter), so that a literal float32 restatement gives the same bits; max() is maxNum (a NaN operand gives the other).
 *   demodulate   only with albedo and iterations > 0: den = max(albedo, 1e-3f), c = color / den per r, g, b; alpha stays color's
 *   iteration i  (i = 0 .. iterations - 1, step s = 2^i): for dy = -2..2 (outer), dx = -2..2 (inner), q = (y + dy s, x + dx s)
 *                inside the image, sum (r, g, b) and wsum from 0:
 *                  w = k[|dx|] * k[|dy|], k = {0.375, 0.25, 0.0625}                                  (the 5 x 5 B3 spline)
 *                  sigma_color > 0:  d = c_p - c_q, dc = (d.r d.r + d.g d.g) + d.b d.b, w = w / (1 + dc * (1 / sigma_color^2))
 *                  normal:  dn = max((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0), squared normal_power_log2 times, w = w * dn
 *                  point:   e = x_q - x_p, pd = (n_p.x e.x + n_p.y e.y) + n_p.z e.z, w = w / (1 + (pd pd) * (1 / sigma_plane^2))
 *                  id:      the tap counts only where id_q == id_p
 *                  a tap whose w is not > 0 (zero, NaN) does not count; else sum += w * c_q, wsum += w
 *                wsum > 0: c_p' = sum / wsum, else c_p' = c_p (a NaN colour, the zero normal of a miss: the pixel passes through).
 *                The centre tap goes through the same formula; the colour weight uses the iteration's own input.
 *   output       remodulate c = c * den if demodulated; gamma != 1: powf(c, 1 / gamma) on r, g, b as a frame's last kernel;
 *                rgba32f_out, and rgba8_out quantised and packed as a frame's.  iterations == 0 runs this stage alone.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event as
 * for rayca_hip_surface_device; every other field, tile included, must be zero.  Ordered on its context like a frame; asynchronous
 * unless stats_out is given: then the call waits and reports the time of its launches (iterations + 1, + 1 with albedo) under
 * RAYCA_KERNEL_OTHER.  The context keeps two scratch images of 16 bytes a pixel.  color, albedo and rgba32f_out must be 16-byte
 * aligned (they are read and written 16 bytes a pixel), every other image as its elements (4 bytes).
 * RAYCA_ERR_BAD_ARG (before any GPU work): NULL scene / arguments / color, no output, width or height 0, width x height > 2^32 - 1,
 * iterations > 8, normal_power_log2 > 10, point without normal, point with sigma_plane not > 0, gamma not > 0, non-zero reserved,
 * a misaligned image, context > 7, a non-zero field of opts that does not apply.  RAYCA_ERR_UNSUPPORTED: a frame whose 64 x 4 pixel tiles number
 * 2^24 or more (one launch cannot cover it). */
struct RaycaDenoise {
  uint32_t width, height;        /* the whole frame; tiles do not apply (packed rows are not neighbours) */
  uint32_t iterations;           /* 0..8; iteration i uses step 2^i.  0: only the output stage (gamma, RGBA8) */
  uint32_t normal_power_log2;    /* 0..10: the normal weight is max(0, n_p.n_q) squared this many times */
  float sigma_color;             /* <= 0: no colour term */
  float sigma_plane;             /* world units; must be > 0 when `point` is given */
  float gamma;                   /* > 0; applied to the outputs exactly as a render call applies RaycaConfig.gamma; 1.0: none */
  uint32_t reserved;             /* must be zero */
  const void* color;             /* DEVICE H x W x 4 f32, required: what rayca_hip_render_device writes to d_rgba32f_out */
  const void* albedo;            /* DEVICE H x W x 4 f32 or NULL: demodulate before, remodulate after (surface color_out / diffuse_out) */
  const void* normal;            /* DEVICE H x W x 3 f32 or NULL (surface normal_out) */
  const void* point;             /* DEVICE H x W x 3 f32 or NULL; needs `normal` (surface point_out) */
  const void* id;                /* DEVICE H x W u32 or NULL: a tap counts only where id_q == id_p (material_out, prim, flags ...) */
  void* rgba32f_out;             /* DEVICE H x W x 4 f32 or NULL; may be the same pointer as `color` (any other overlap is undefined) */
  void* rgba8_out;               /* DEVICE H x W x 4 u8 or NULL; not both outputs NULL */
};
typedef struct RaycaDenoise RaycaDenoise;
int32_t rayca_hip_denoise_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaDenoise* d, RaycaStats* stats_out);

/* The camera a frame of the scene uses (camera_draw_infos[0]), in the form a reprojection needs it.  Host only: no GPU work, no
 * frame context.  A camera ray is origin + s * R * S * (xx, yy, -1) (scene.rs:125-141, trs.rs:275-284), with R and S the rotation
 * and the scale of the camera node's world transform; for a world point x with v = x - origin that gives
 *   xx = (right . v) / -(back . v),  yy = (up . v) / -(back . v)
 * without a quaternion inverse, for a non-uniform camera scale too.  `rotate` is the reference's (vec3.rs:148-159), evaluated on
 * the host; every division is per component.  After a rayca_hip_scene_update the call returns the new camera.
 * RAYCA_ERR_BAD_ARG: a NULL argument.  RAYCA_ERR_NO_CAMERA: the scene has none. */
struct RaycaCameraPose {
  float origin[3];  float angle;      /* the origin of the frame's camera rays: the translation of the camera node's world transform;
                                         tanf(yfov * 0.5f), the bits a frame uses */
  float right[3];   float reserved0;  /* rotate((1,0,0), rotation) / scale.x; reserved: 0 */
  float up[3];      float reserved1;  /* rotate((0,1,0), rotation) / scale.y */
  float back[3];    float reserved2;  /* rotate((0,0,1), rotation) / scale.z */
};
typedef struct RaycaCameraPose RaycaCameraPose;
int32_t rayca_hip_scene_camera(const RaycaScene* scene, RaycaCameraPose* out);

/* Temporal accumulation with reprojection: one pass, one kernel, on a frame, its G-buffer and a history, all in DEVICE memory.
 * `color` is what rayca_hip_render_device wrote to d_rgba32f_out (gamma 1); point, normal and id are what rayca_hip_surface_device
 * wrote for the frame's camera rays (of a one-sample frame: the reprojection assumes points on the rays through pixel centres);
 * the history is what an earlier call wrote to color_out / length_out / moments_out, with the G-buffer (prev_*) and the camera
 * (prev_camera) of the frame it belongs to.  No reference counterpart.  The scene handle gives the call its device and its frame
 * context; the scene is not read, and an empty scene is no error.
 * Everything is f32, every operation rounds once, in the association written here, so that a literal float32 restatement gives
 * the same bits; every comparison is written so that a NaN fails it.  For pixel p = (x, y), c = color[p], W = width, H = height:
 *   sample      finite iff c.k - c.k == 0 for all four channels
 *   luminance   lum = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b
 *   history, identity mode (prev_camera == NULL):
 *               h = hist_color[p], L = hist_length[p], m = hist_moments[p]; present iff a history was given and L > 0
 *   history, reprojection mode (prev_camera given):
 *               normal[p] == (0, 0, 0) is a miss (as rayca_hip_surface_device writes one): no history.  Otherwise
 *               v = point[p] - origin
 *               cx = (right.x v.x + right.y v.y) + right.z v.z, cy the same with up, cz the same with back
 *               present only if cz < 0;  nz = 0 - cz
 *               aspect = (float)W / (float)H
 *               fx = ((cx / nz) / (angle * aspect) + 1) * 0.5 * W - 0.5      (left to right: five roundings behind the quotient)
 *               fy = (1 - (cy / nz) / angle) * 0.5 * H - 0.5
 *               present only if fx >= -1 && fx < W && fy >= -1 && fy < H
 *               x0 = floor(fx), tx = fx - x0; y0 = floor(fy), ty = fy - y0
 *               the four taps go j = 0, 1 (outer), i = 0, 1 (inner), q = (y0 + j, x0 + i), b = (i ? tx : 1 - tx) * (j ? ty : 1 - ty)
 *               a tap counts iff q is inside the image, b > 0, hist_length[q] > 0, prev_id[q] == id[p] (where ids are given),
 *                 (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= normal_min with n_p = normal[p], n_q = prev_normal[q], and, where
 *                 prev_point is given, |pd| <= plane_max with e = prev_point[q] - point[p], pd = (n_p.x e.x + n_p.y e.y) + n_p.z e.z
 *               sums from 0: wsum += b, colour += b * hist_color[q] (four channels), length += b * hist_length[q],
 *                 moments += b * hist_moments[q]
 *               present iff wsum > 0; then h, L, m = the sums / wsum
 *   blend       history present, sample finite:      n = L + 1, with max_history > 0 n = min(n, (float)max_history); a = 1 / n
 *                                                    out = h + (c - h) * a (four channels), length_out = n
 *                                                    m1 = m.x + (lum - m.x) * a, m2 = m.y + (lum * lum - m.y) * a
 *               history present, sample not finite:  out = h, length_out = L, moments = m (a firefly NaN does not enter the film)
 *               no history, sample finite:           out = c, length_out = 1, moments = (lum, lum * lum)
 *               no history, sample not finite:       out = c, length_out = 0, moments = 0 (hist_length > 0 is the validity
 *                                                    channel: the next frame reads nothing from this pixel)
 *               variance_out = max(m2 - m1 * m1, 0)
 * max() and min() are maxNum and minNum (a NaN operand gives the other one).  Moments are formed only with moments_out; a
 * hist_moments without it is not read.  Without a history (first frame) prev_camera changes nothing: no pixel has one.
 * Aliasing.  In identity mode the pass is pixel-local: color_out may be hist_color or color, length_out may be hist_length,
 * moments_out may be hist_moments -- a film in place.  In reprojection mode taps read neighbours: an output equal to any hist_ or
 * prev_ input is RAYCA_ERR_BAD_ARG; color_out == color stays allowed.  Any other overlap is undefined.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event as
 * for rayca_hip_surface_device; every other field, tile included, must be zero (a tile's packed rows are not neighbours).
 * Ordered on its context like a frame; asynchronous unless stats_out is given: then the call waits and reports the time of its
 * one launch under RAYCA_KERNEL_OTHER.  No scratch image.  color, hist_color and color_out must be 16-byte aligned (read and
 * written 16 bytes a pixel), every other image as its elements (4 bytes).
 * RAYCA_ERR_BAD_ARG (before any GPU work, the message names the field): NULL scene / arguments, width or height 0, width x
 * height > 2^32 - 1, non-zero reserved, a required pointer missing or a forbidden one given as the struct lists them, normal_min
 * or plane_max not > 0 where it applies, a misaligned image, the aliasing rule, context > 7, a non-zero field of opts that does not
 * apply.  RAYCA_ERR_UNSUPPORTED: a frame whose 64 x 4 pixel tiles number 2^24 or more. */
struct RaycaAccumulate {
  uint32_t width, height;   /* the whole frame */
  uint32_t max_history;     /* 0: unbounded (a running mean); else the history length is capped here (an exponential tail) */
  uint32_t reserved;        /* must be zero */
  float normal_min;         /* reprojection: a tap counts only where n_p . n_q >= normal_min; must be > 0 */
  float plane_max;          /* reprojection with prev_point: a tap counts only where |n_p . (x_q - x_p)| <= plane_max; must be > 0 then */
  const RaycaCameraPose* prev_camera;   /* HOST, copied during the call; NULL: identity mapping (the camera did not move) */
  const void* color;        /* DEVICE H x W x 4 f32, required: this frame, gamma 1 */
  const void* point;        /* DEVICE H x W x 3 f32  } this frame's G-buffer; required with prev_camera, */
  const void* normal;       /* DEVICE H x W x 3 f32  } must be NULL without it */
  const void* id;           /* DEVICE H x W u32 or NULL; with prev_id or not at all */
  const void* hist_color;   /* DEVICE H x W x 4 f32 } the history: all three or none (none = first frame), */
  const void* hist_length;  /* DEVICE H x W f32     } hist_moments optional with the other two */
  const void* hist_moments; /* DEVICE H x W x 2 f32: mean luminance, mean squared luminance */
  const void* prev_normal;  /* DEVICE H x W x 3 f32: the G-buffer of the frame the history belongs to; required with prev_camera + history */
  const void* prev_point;   /* DEVICE H x W x 3 f32 or NULL */
  const void* prev_id;      /* DEVICE H x W u32 or NULL */
  void* color_out;          /* DEVICE H x W x 4 f32, required */
  void* length_out;         /* DEVICE H x W f32, required */
  void* moments_out;        /* DEVICE H x W x 2 f32 or NULL; requires hist_moments whenever there is a history */
  void* variance_out;       /* DEVICE H x W f32 or NULL; needs moments_out */
};
typedef struct RaycaAccumulate RaycaAccumulate;
int32_t rayca_hip_accumulate_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaAccumulate* a, RaycaStats* stats_out);

/* The variance-guided a-trous denoiser (after the filter stage of SVGF, Schied et al. 2017), on a frame, its luminance variance
 * and its G-buffer in DEVICE memory: the stage behind rayca_hip_accumulate_device.  `color` is a film's color_out (gamma 1),
 * `variance` its variance_out, `length` its length_out; the guides are rayca_hip_denoise_device's.  Where that filter steers its
 * colour term with one global sigma_color, this one scales the luminance term with a local variance estimate, filters the variance
 * along with the colour, and gives a pixel with a short history a spatial estimate: a converged film is left nearly alone, a fresh
 * one is filtered hard, and an edge that no guide shows survives where it stands out of the noise.  No reference counterpart.  The
 * scene handle gives the call its device and its frame context; the scene is not read, and an empty scene is no error.
 * Everything is f32, every operation rounds once, in the association written here (only +, -, x, / and max: no exp, no sqrt, no
 * pow inside the filter), so that a literal float32 restatement gives the same bits; max() is maxNum (a NaN operand gives the
 * other one), and every comparison is written so that a NaN fails it.
 * lum(c) = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b;  k = {0.375, 0.25, 0.0625}, the 5 x 5 B3 spline.
 *   demodulate   only with albedo: den = max(albedo, 1e-3f), c = color / den per r, g, b; alpha stays color's.  ld = lum(den)
 *   variance v0  v = max(variance[p], 0)                                                              (a NaN becomes 0)
 *                albedo:  v = v / (ld * ld)        (exact for a grey albedo, an approximation for any other: the luminance of
 *                                                   a quotient is not the quotient of the luminances)
 *                length:  L = length[p], v = v / max(L, 1)        (the variance of the film's mean, not of one sample: what
 *                                                                  makes the filter back off as the film converges)
 *                min_history > 0 and L < (float)min_history: v is replaced by a spatial estimate over the demodulated image,
 *                  for dy = -3..3 (outer), dx = -3..3 (inner), q = (y + dy, x + dx) inside the image, s1, s2, ws from 0:
 *                  w = 1, then the normal and the point term of an iteration below; l_q = lum(c_q)
 *                  the tap counts iff w > 0, id_q == id_p (with id) and l_q - l_q == 0
 *                  s1 += w * l_q, s2 += w * (l_q * l_q), ws += w
 *                  ws > 0: m1 = s1 / ws, m2 = s2 / ws, v = max(m2 - m1 * m1, 0); else v = 0
 *   iteration i  (i = 0 .. iterations - 1, step s = 2^i), from a colour image and a variance plane into the other two:
 *                g_p = (sum G v_q) / (sum G) over dy = -1..1 (outer), dx = -1..1 (inner), q = (y + dy, x + dx) inside the image,
 *                  both sums from 0, G = 0.25 at the centre, 0.125 at an edge, 0.0625 at a corner
 *                dnm = sl2 * g_p + variance_floor, sl2 = sigma_luminance * sigma_luminance (formed on the host); l_p = lum(c_p)
 *                for dy = -2..2 (outer), dx = -2..2 (inner), q = (y + dy s, x + dx s) inside the image, sum, vs, ws from 0:
 *                  w = k[|dx|] * k[|dy|];  d = l_p - lum(c_q), w = w / (1 + (d * d) / dnm)
 *                  normal:  dn = max((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0), squared normal_power_log2 times, w = w * dn
 *                  point:   e = x_q - x_p, pd = (n_p.x e.x + n_p.y e.y) + n_p.z e.z, w = w / (1 + (pd pd) * (1 / sigma_plane^2))
 *                  the tap counts iff w > 0 and id_q == id_p (with id)
 *                  sum += w * c_q (r, g, b), vs += (w * w) * v_q (v_q: this iteration's unfiltered input variance), ws += w
 *                ws > 0: c_p' = sum / ws, v_p' = vs / (ws * ws); else both pass through (a NaN colour, the zero normal of a miss)
 *   output       the colour as rayca_hip_denoise_device's output stage: remodulate c = c * den if demodulated, gamma, rgba32f_out,
 *                rgba8_out.  variance_out receives the last variance plane, in the units the filter ran in (demodulated with albedo).
 * No kernel reads an image it writes, and `variance` is read only for v0: rgba32f_out may be `color`, variance_out may be
 * `variance`.  Any other overlap is undefined.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event as
 * for rayca_hip_surface_device; every other field, tile included, must be zero.  Ordered on its context like a frame; asynchronous
 * unless stats_out is given: then the call waits and reports the time of its launches (iterations + 2, + 1 with albedo) under
 * RAYCA_KERNEL_OTHER.  The context keeps the denoiser's two scratch images and two variance planes of 4 bytes a pixel.  color,
 * albedo and rgba32f_out must be 16-byte aligned, every other image as its elements (4 bytes).
 * RAYCA_ERR_BAD_ARG (before any GPU work, the message names the field): NULL scene / arguments / color / variance, no output, width
 * or height 0, width x height > 2^32 - 1, iterations 0 or > 8, normal_power_log2 > 10, min_history > 0 without length, point
 * without normal, point with sigma_plane not > 0, sigma_luminance, variance_floor or gamma not > 0, non-zero reserved, a misaligned
 * image, context > 7, a non-zero field of opts that does not apply.  RAYCA_ERR_UNSUPPORTED: a frame whose 64 x 4 pixel tiles number
 * 2^24 or more. */
struct RaycaDenoiseVariance {
  uint32_t width, height;        /* the whole frame */
  uint32_t iterations;           /* 1..8; iteration i uses step 2^i */
  uint32_t normal_power_log2;    /* 0..10: the normal weight is max(0, n_p.n_q) squared this many times */
  uint32_t min_history;          /* a pixel whose length is below it takes the spatial estimate; 0: no spatial fallback */
  uint32_t reserved;             /* must be zero */
  float sigma_luminance;         /* > 0: the luminance difference is measured in units of sigma_luminance standard deviations */
  float sigma_plane;             /* world units; must be > 0 when `point` is given */
  float variance_floor;          /* > 0: added to the scaled variance, so that a zero variance divides by something */
  float gamma;                   /* > 0; applied to the colour outputs exactly as a render call applies RaycaConfig.gamma */
  const void* color;             /* DEVICE H x W x 4 f32, required: the film (color_out of rayca_hip_accumulate_device), gamma 1 */
  const void* variance;          /* DEVICE H x W f32, required: what variance_out of the accumulation holds */
  const void* length;            /* DEVICE H x W f32 or NULL (length_out); required when min_history > 0 */
  const void* albedo;            /* DEVICE H x W x 4 f32 or NULL: demodulate before, remodulate after */
  const void* normal;            /* DEVICE H x W x 3 f32 or NULL */
  const void* point;             /* DEVICE H x W x 3 f32 or NULL; needs `normal` */
  const void* id;                /* DEVICE H x W u32 or NULL: a tap counts only where id_q == id_p */
  void* rgba32f_out;             /* DEVICE H x W x 4 f32 or NULL; may be the same pointer as `color` */
  void* rgba8_out;               /* DEVICE H x W x 4 u8 or NULL; not both colour outputs NULL */
  void* variance_out;            /* DEVICE H x W f32 or NULL; may be the same pointer as `variance` */
};
typedef struct RaycaDenoiseVariance RaycaDenoiseVariance;
int32_t rayca_hip_denoise_variance_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaDenoiseVariance* d, RaycaStats* stats_out);

/* Guided upsampling: a low-resolution frame onto a full-size G-buffer (a joint bilateral upsample), one pass, one kernel, all in
 * DEVICE memory.  `color` is what rayca_hip_render_device wrote to d_rgba32f_out for the width / scale x height / scale view
 * (gamma 1), or that frame behind a denoiser or a film; the _low guides are what rayca_hip_surface_device wrote for that view's
 * camera rays, the full-size guides what it wrote for the width x height view of the same camera.  The G-buffers are those of
 * sample 0 of a one-sample config (points on the rays through pixel centres), as for the accumulation.  Textures, silhouettes
 * and normals come from the exact full-size surface data; only the demodulated colour -- the low-frequency irradiance -- is
 * interpolated.  No reference counterpart.  The scene handle gives the call its device and its frame context; the scene is not
 * read, and an empty scene is no error.
 * Everything is f32, every operation rounds once, in the association written here (only +, -, x, /, floor and max), so that a
 * literal float32 restatement gives the same bits; every comparison is written so that a NaN fails it; max() is maxNum (a NaN
 * operand gives the other one).  The low image is w = width / scale by h = height / scale, both divisions exact (so that both
 * views share an aspect ratio whose float quotient has the same bits).  For output pixel p = (x, y), s = (float)scale:
 *   footprint    fx = ((float)x + 0.5f) / s - 0.5f, fy = ((float)y + 0.5f) / s - 0.5f
 *                x0 = floor(fx), tx = fx - x0; y0 = floor(fy), ty = fy - y0
 *                the four taps go j = 0, 1 (outer), i = 0, 1 (inner), q = (y0 + j, x0 + i), b = (i ? tx : 1 - tx) * (j ? ty : 1 - ty)
 *                a tap exists iff q is inside the low image, b > 0 and color[q] is finite (c.k - c.k == 0 for all four channels)
 *   demodulate   with albedo: c_q.rgb = color[q].rgb / max(albedo_low[q].rgb, 1e-3f); alpha stays color's.  Else c_q = color[q]
 *   guided pass  over the taps that exist, sum (four channels) and wsum from 0:
 *                  w = b
 *                  normal, n_p == (0, 0, 0) (a miss, as rayca_hip_surface_device writes one): the tap counts only where
 *                    n_q == (0, 0, 0); the normal and the point term are skipped
 *                  normal, otherwise:
 *                    dn = max((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z, 0), squared normal_power_log2 times, w = w * dn
 *                    point:  e = x_q - x_p, pd = (n_p.x e.x + n_p.y e.y) + n_p.z e.z, w = w / (1 + (pd pd) * (1 / sigma_plane^2))
 *                            (the reciprocal is formed on the host, as the denoiser's)
 *                  id:      the tap counts only where id_q == id_p
 *                  the tap counts iff w > 0; then sum += w * c_q, wsum += w
 *                wsum > 0: o = sum / wsum
 *   fallback     wsum not > 0 (no tap agrees with the pixel's surface): the same loop with w = b alone, sumb and bsum from 0;
 *                bsum > 0: o = sumb / bsum.  Otherwise (no tap exists) o = the demodulated colour of the nearest low pixel,
 *                (min(y / scale, h - 1), min(x / scale, w - 1)) in integer arithmetic, whatever it holds: a NaN passes through,
 *                as in the other filters.
 *   weight_out   wsum of the guided pass: 0 where the fallback was used -- the caller's list of pixels that might deserve a
 *                traced sample
 *   output       with albedo: o.rgb = o.rgb * max(albedo[p].rgb, 1e-3f); then the output stage of rayca_hip_denoise_device exactly:
 *                gamma != 1: powf(c, 1 / gamma) on r, g, b as a frame's last kernel; rgba32f_out, and rgba8_out quantised and
 *                packed as a frame's.
 * (x_p, n_p, id_p are point, normal, id at p; x_q, n_q, id_q are point_low, normal_low, id_low at q.  At scale 1 every pixel has
 * the one tap b = 1: without guides the pass is the output stage alone, but for a -0.0, which the sum from 0 returns as +0.0.)
 * Aliasing: no output may overlap an input.  The images differ in size and the taps read neighbours, so an output pointer equal
 * to an input pointer is RAYCA_ERR_BAD_ARG; any other overlap is undefined.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event as
 * for rayca_hip_surface_device; every other field, tile included, must be zero (a tile's packed rows are not neighbours).
 * Ordered on its context like a frame; asynchronous unless stats_out is given: then the call waits and reports the time of its
 * one launch under RAYCA_KERNEL_OTHER.  No scratch image.  color, albedo_low, albedo and rgba32f_out must be 16-byte aligned (read
 * and written 16 bytes a pixel), every other image as its elements (4 bytes).
 * RAYCA_ERR_BAD_ARG (before any GPU work, the message names the field): NULL scene / arguments / color, scale 0 or > 8, width or
 * height not divisible by scale, width or height 0, width x height > 2^32 - 1, one half of a guide pair, point without normal,
 * point with sigma_plane not > 0, gamma not > 0, normal_power_log2 > 10, no colour output, non-zero reserved, a misaligned image,
 * the aliasing rule, context > 7, a non-zero field of opts that does not apply.  RAYCA_ERR_UNSUPPORTED: a frame whose 64 x 4
 * pixel tiles number 2^24 or more. */
struct RaycaUpsample {
  uint32_t width, height;        /* the output: the whole full-size frame, W x H */
  uint32_t scale;                /* 1..8; the low image is w = width / scale by h = height / scale, both exact */
  uint32_t normal_power_log2;    /* 0..10: the normal weight is max(0, n_p.n_q) squared this many times */
  float sigma_plane;             /* world units; must be > 0 when `point` is given */
  float gamma;                   /* > 0; applied to the colour outputs exactly as a render call applies RaycaConfig.gamma */
  uint32_t reserved;             /* must be zero */
  const void* color;             /* DEVICE h x w x 4 f32, required: the low-resolution frame, gamma 1 */
  const void* albedo_low;        /* DEVICE h x w x 4 f32 } each guide at both resolutions or at neither */
  const void* normal_low;        /* DEVICE h x w x 3 f32 } */
  const void* point_low;         /* DEVICE h x w x 3 f32 } */
  const void* id_low;            /* DEVICE h x w u32     } */
  const void* albedo;            /* DEVICE H x W x 4 f32 or NULL: demodulate the taps, remodulate the pixel (surface color_out / diffuse_out) */
  const void* normal;            /* DEVICE H x W x 3 f32 or NULL (surface normal_out) */
  const void* point;             /* DEVICE H x W x 3 f32 or NULL; needs `normal` (surface point_out) */
  const void* id;                /* DEVICE H x W u32 or NULL: a tap counts only where id_q == id_p (material_out, prim, ...) */
  void* rgba32f_out;             /* DEVICE H x W x 4 f32 or NULL */
  void* rgba8_out;               /* DEVICE H x W x 4 u8 or NULL; not both colour outputs NULL */
  void* weight_out;              /* DEVICE H x W f32 or NULL: the guided pass's wsum, 0 where the fallback was used */
};
typedef struct RaycaUpsample RaycaUpsample;
int32_t rayca_hip_upsample_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaUpsample* u, RaycaStats* stats_out);

/* Exposure metering: how bright a frame is, measured in DEVICE memory -- a luminance histogram of a linear frame and, from it, an
 * exposure record that rayca_hip_tonemap_device reads where it lies.  `color` is a frame with gamma 1 (render_device's float
 * output, a film, a denoised or upsampled frame).  No reference counterpart.  The scene handle gives the call its device and its
 * frame context; the scene is not read.
 * Only +, -, x, /, min, max and integer arithmetic, every f32 operation rounded once in the association written here; every
 * comparison is written so that a NaN fails it.  Everything behind Y is integer arithmetic, so the order in which the pixels
 * are counted changes no bit, and a literal restatement (tests/tonemap_literal.py) gives the same words.
 *   histogram  per pixel (r, g, b, a): Y = (0.2126f r + 0.7152f g) + 0.0722f b
 *              not finite: r, g, b or Y fails x - x == 0.  black: finite and Y <= 0 (a miss of the scene is black).  Any other
 *              pixel is counted, in bin clamp((int)(bits(Y) >> 20) - ((127 - 16) << 3), 0, 255): the float's own exponent and its
 *              top three mantissa bits -- 8 bins an octave over 2^-16 .. 2^16, linear inside an octave; below and above, the
 *              first and the last bin.
 *              hist_out[0..255] the bins, [256] counted, [257] black, [258] not finite, [259] 0.  The call overwrites all 260.
 *   exposure   (with exposure_out) from this call's histogram, in u64 with floor:
 *              N = counted, a = N * low_permille / 1000, b = N * high_permille / 1000
 *              over the bins in order, c0 / c1 the running count before / after bin i: k_i = max(0, min(c1, b) - max(c0, a))
 *              K = sum k_i, T = sum k_i * (2 i + 1), Q = (T << 12) / K          (T << 12 < 2^53)
 *              L = (1 + (float)(Q & 0xffff) / 65536) * 2^((Q >> 16) - 16)      -- both steps exact: the inverse of the bins'
 *                                                                                 piecewise-linear logarithm at the trimmed mean
 *              target = min(max(key / L, min_scale), max_scale)
 *              p = exposure_prev[0] is usable iff exposure_prev is given, p > 0 and p - p == 0
 *              K == 0 (nothing counted): L = 0, target = p if usable, else 1
 *              scale = p + (target - p) * rate if p is usable, else target
 *              exposure_out = {scale, target, L, 0}
 *              `rate` is the caller's adaptation factor (for instance 1 - exp(-dt * speed), formed by the caller); 1 jumps.
 * exposure_prev may be exposure_out (the record is read before it is written); hist_out must differ from every other pointer,
 * and exposure_out from color: equal pointers are RAYCA_ERR_BAD_ARG, any other overlap is undefined.
 * opts, ordering, stats_out: as for rayca_hip_upsample_device (every field but stream, context, wait_event and record_event
 * zero, tile included); launches: the clear, the histogram kernel and, with exposure_out, the one-wave exposure kernel.
 * RAYCA_ERR_BAD_ARG (before any GPU work, the message names the field): NULL scene / arguments / color / hist_out, width or
 * height 0, width x height > 2^32 - 1, not 0 <= low_permille < high_permille <= 1000, key not > 0, min_scale or max_scale not
 * finite or not 0 < min_scale <= max_scale, rate not in (0, 1], non-zero reserved, a misaligned pointer (color and exposure_out
 * 16 bytes, hist_out and exposure_prev 4), equal pointers as above, context > 7, a non-zero field of opts that does not apply.
 * RAYCA_ERR_UNSUPPORTED: a frame whose 64 x 4 pixel tiles number 2^24 or more (as the passes that would display it). */
struct RaycaMeter {
  uint32_t width, height;        /* the whole frame, W x H */
  uint32_t low_permille;         /* the trimmed mean leaves out this share of the counted pixels at the dark end ... */
  uint32_t high_permille;        /* ... and everything above this share: 0 <= low < high <= 1000 */
  float key;                     /* > 0: the luminance the metered one is mapped to (0.18: middle grey) */
  float min_scale, max_scale;    /* finite, 0 < min_scale <= max_scale: the target is clamped between them */
  float rate;                    /* in (0, 1]: how far the scale moves from exposure_prev's towards the target */
  uint32_t reserved;             /* must be zero */
  const void* color;             /* DEVICE H x W x 4 f32, required, gamma 1 */
  void* hist_out;                /* DEVICE 260 u32, required; overwritten (the caller never clears it) */
  void* exposure_out;            /* DEVICE 4 f32 or NULL: {scale, target, L, 0} */
  const void* exposure_prev;     /* DEVICE 4 f32 or NULL: the previous record; may be exposure_out */
};
typedef struct RaycaMeter RaycaMeter;
int32_t rayca_hip_meter_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaMeter* m, RaycaStats* stats_out);

/* Tone mapping: a linear frame through an exposure scale and a display operator into the output stage, one pixel-local pass in
 * DEVICE memory.  The scale is word 0 of `exposure` -- normally the record rayca_hip_meter_device wrote, so that nothing returns
 * to the host -- or, without it, the host's `scale`.  No reference counterpart; the scene is not read.
 * Arithmetic as above (+, -, x, / only, one rounding each, the association written here).  Per pixel c, s the scale,
 * x.k = c.k * s for k in r, g, b:
 *   RAYCA_TONEMAP_LINEAR    o = x
 *   RAYCA_TONEMAP_REINHARD  (extended, on luminance) Y = (0.2126f x.r + 0.7152f x.g) + 0.0722f x.b; where Y > 0:
 *                           m = (1 + Y * inv_white2) / (1 + Y), o.k = x.k * m; elsewhere o = x.  inv_white2 = 1 / (white * white),
 *                           formed on the host as the denoiser forms its reciprocals, 0 when white is 0 (no white point)
 *   RAYCA_TONEMAP_ACES      (the rational fit) per channel o.k = (x.k * (2.51f * x.k + 0.03f)) / (x.k * (2.43f * x.k + 0.59f) + 0.14f)
 *                           (the denominator has no real root)
 * Alpha passes through; a channel that is not finite comes out as the arithmetic has it.  Then the output stage of
 * rayca_hip_denoise_device exactly: gamma != 1: powf(o, 1 / gamma) on r, g, b; rgba32f_out, and rgba8_out quantised and packed as
 * a frame's.
 * rgba32f_out may be `color` (a lane reads its pixel before it writes it).  Every other pair of equal pointers among color,
 * exposure and the outputs is RAYCA_ERR_BAD_ARG; any other overlap is undefined.
 * opts, ordering, stats_out: as for rayca_hip_upsample_device; one launch.
 * RAYCA_ERR_BAD_ARG (before any GPU work, the message names the field): NULL scene / arguments / color, width or height 0,
 * width x height > 2^32 - 1, an unknown op, exposure NULL and scale not finite or not > 0, white negative or not finite, white
 * set with an op other than REINHARD, gamma not > 0, no output, non-zero reserved, a misaligned pointer (color and rgba32f_out 16
 * bytes, exposure and rgba8_out 4), equal pointers as above, context > 7, a non-zero field of opts that does not apply.
 * RAYCA_ERR_UNSUPPORTED: a frame whose 64 x 4 pixel tiles number 2^24 or more. */
enum { RAYCA_TONEMAP_LINEAR = 0, RAYCA_TONEMAP_REINHARD = 1, RAYCA_TONEMAP_ACES = 2 };
struct RaycaTonemap {
  uint32_t width, height;        /* the whole frame, W x H */
  uint32_t op;                   /* RAYCA_TONEMAP_ */
  float scale;                   /* used when `exposure` is NULL: finite and > 0 */
  float white;                   /* REINHARD's white point: 0 = none, else finite and > 0; must be 0 for the other operators */
  float gamma;                   /* > 0; applied to the colour outputs exactly as a render call applies RaycaConfig.gamma */
  uint32_t reserved;             /* must be zero */
  const void* color;             /* DEVICE H x W x 4 f32, required, gamma 1 */
  const void* exposure;          /* DEVICE 4 f32 or NULL: word 0 is the scale (rayca_hip_meter_device's exposure_out) */
  void* rgba32f_out;             /* DEVICE H x W x 4 f32 or NULL; may be the same pointer as `color` */
  void* rgba8_out;               /* DEVICE H x W x 4 u8 or NULL; not both outputs NULL */
};
typedef struct RaycaTonemap RaycaTonemap;
int32_t rayca_hip_tonemap_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaTonemap* t, RaycaStats* stats_out);

/* Adaptive sampling, the plan: a film's own error estimate decides where the next `budget` rays go, everything in DEVICE memory
 * and nothing read back.  `color`, `variance` and `length` are a film's color_out, variance_out and length_out
 * (rayca_hip_accumulate_device); the plan gives every pixel an integer weight, turns the weights into ray offsets by an exact
 * prefix sum and, with rays_out, writes the camera rays themselves in the layout rayca_hip_query_device and
 * rayca_hip_radiance_device read.  `budget` (B) is fixed on the host, so the radiance call behind the plan takes its count without
 * a round trip.  No reference counterpart.  The weights and offsets read no scene; the rays read its camera.
 * The weight is f32, every operation rounds once, in the association written here; every comparison is written so that a NaN
 * fails it; max() and min() are maxNum and minNum.  Everything behind the weight is integer arithmetic and no result depends on
 * an order of execution, so a literal restatement (tests/adaptive_literal.py) gives the same words.  For pixel p (raster order,
 * p = y * W + x), c = color[p]:
 *   weight     l = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b, d = max(l, lum_floor)
 *              v = max(variance[p], 0), L = length[p]
 *              e = (v / max(L, 1)) / (d * d)                      the relative variance of the pixel's mean
 *              r = e / (target * target)                          (the product is formed on the host, once)
 *              q = floor(min(r, 255)) where r >= 0, else 0
 *              w = min(base_weight + (uint)q, 255)
 *              where !(L >= (float)min_history): w = max(w, fresh_weight)   (one sample has variance 0 and must not look converged)
 *   offsets    S = sum of the weights, exactly; if S == 0 every weight counts as 1 (then S = W * H)
 *              P(p) = the sum of the weights of the pixels in front of p
 *              offset_out[p] = (uint32)((uint64)P(p) * B / S), offset_out[W * H] = B
 *              so pixel p receives n_p = offset_out[p + 1] - offset_out[p] rays, all n_p sum to B exactly, and
 *              |n_p - w_p B / S| < 1
 *   rays       ray j belongs to the pixel p with offset_out[p] <= j < offset_out[p + 1] and is its sample k = j - offset_out[p]
 *              stratum s = (first_stratum + k) mod n^2 of the n x n stratified sub-pixel positions, n = jitter:
 *              ix = s mod n, iy = s / n, step 1 / n, offset 0.5 / n -- a frame's own positions for samples_per_pixel n^2
 *              rays_out[j] = row p of rayca_hip_camera_rays_device(cfg with samples_per_pixel n^2, sample s), bit for bit
 *              pixel_out[j] = p
 * Rays and pixel indices are made only for the outputs that are given; rays_out needs a camera.  budget == 0 is RAYCA_OK: every
 * offset is 0 and there are no rays.  Outputs must not overlap inputs or each other: undefined.
 * opts (may be NULL): stream (NULL => the context's own stream, and the call waits for it), context, wait_event, record_event as
 * for rayca_hip_surface_device; every other field, tile included, must be zero.  Ordered on its context like a frame; asynchronous
 * unless stats_out is given: then the call waits and reports its launches under RAYCA_KERNEL_OTHER -- three (weights, the scan of
 * the segment sums, offsets) and a fourth for rays_out or pixel_out when budget > 0.  The context keeps a scratch word a pixel
 * (without weight_out) and one per 64 pixels of a row.
 * RAYCA_ERR_BAD_ARG (before any GPU work, the message names the field): NULL scene / arguments, non-zero reserved, width or
 * height 0, width x height > 2^32 - 1, budget > 2^31, jitter not in 1..8, base_weight or fresh_weight above 255, target or lum_floor
 * not > 0, NULL color / variance / length / offset_out, a misaligned image (color 16 bytes, every other 4), context > 7, a non-zero
 * field of opts that does not apply.  RAYCA_ERR_UNSUPPORTED: width x height x 256 > 2^32 (the sum of the weights must fit 32 bits
 * and its product with the budget 64).  RAYCA_ERR_NO_CAMERA: rays_out on a scene without a camera. */
struct RaycaSamplePlan {
  uint32_t width, height;   /* the whole frame, W x H */
  uint32_t budget;          /* B: the rays this pass traces, <= 2^31 */
  uint32_t jitter;          /* n, 1..8: the rays go through the n x n stratified sub-pixel positions */
  uint32_t first_stratum;   /* a pixel's first ray takes this stratum (mod n^2), the next ones those behind it */
  uint32_t base_weight;     /* 0..255: what every pixel weighs before its variance adds to it */
  uint32_t fresh_weight;    /* 0..255: the least weight of a pixel whose history is shorter than min_history */
  uint32_t min_history;
  float target;             /* > 0: the relative standard error of a pixel's mean that adds one step of weight */
  float lum_floor;          /* > 0: the luminance the error is measured against is at least this */
  uint32_t reserved;        /* must be zero */
  const void* color;        /* DEVICE H x W x 4 f32, required: the film, gamma 1 */
  const void* variance;     /* DEVICE H x W f32, required */
  const void* length;       /* DEVICE H x W f32, required */
  void* weight_out;         /* DEVICE H x W u32 or NULL */
  void* offset_out;         /* DEVICE (H x W + 1) u32, required */
  void* rays_out;           /* DEVICE B x 6 f32 or NULL: origin xyz, direction xyz */
  void* pixel_out;          /* DEVICE B u32 or NULL */
};
typedef struct RaycaSamplePlan RaycaSamplePlan;
int32_t rayca_hip_sample_plan_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaSamplePlan* plan, RaycaStats* stats_out);

/* Adaptive sampling, the fold: a ragged list of samples into a history, one pixel-local pass in DEVICE memory.  `samples` is
 * what rayca_hip_radiance_device wrote (gamma 1) for a plan's rays, `offset` that plan's offset_out; the history and the outputs
 * are rayca_hip_accumulate_device's.  The scene is not read.  Per pixel p, with the arithmetic, the finiteness test and the
 * luminance of rayca_hip_accumulate_device:
 *   state      h = hist_color[p], L = hist_length[p], m = hist_moments[p]; present iff L > 0, as identity mode takes a history
 *   samples    for j = offset[p] .. offset[p + 1] - 1, in this order: the blend rows of rayca_hip_accumulate_device with
 *              c = samples[j] (history present or not, sample finite or not), max_history as there; the step's outputs are the
 *              next step's history -- what offset[p + 1] - offset[p] calls of rayca_hip_accumulate_device in identity mode give
 *   no sample  color_out, length_out and moments_out are the history's, as they stand
 *   variance_out = max(m2 - m1 * m1, 0) of the moments written
 * The pass is pixel-local: color_out may be hist_color, length_out hist_length, moments_out hist_moments.  Any other overlap is
 * undefined.  opts, ordering, stats_out: as for rayca_hip_accumulate_device; one launch, no scratch.
 * RAYCA_ERR_BAD_ARG (before any GPU work, the message names the field): NULL scene / arguments, non-zero reserved, width or
 * height 0, width x height > 2^32 - 1, NULL samples / offset / color_out / length_out / hist_color / hist_length, moments_out
 * without hist_moments, variance_out without moments_out, a misaligned image (samples, hist_color and color_out 16 bytes, every
 * other 4), context > 7, a non-zero field of opts that does not apply.  RAYCA_ERR_UNSUPPORTED: a frame whose 64 x 4 pixel tiles
 * number 2^24 or more. */
struct RaycaFilmFold {
  uint32_t width, height;   /* the whole frame */
  uint32_t max_history;     /* as RaycaAccumulate.max_history */
  uint32_t reserved;        /* must be zero */
  const void* samples;      /* DEVICE B x 4 f32, required: B = offset[H x W] */
  const void* offset;       /* DEVICE (H x W + 1) u32, required: non-decreasing, offset[0] = 0 */
  const void* hist_color;   /* DEVICE H x W x 4 f32, required */
  const void* hist_length;  /* DEVICE H x W f32, required */
  const void* hist_moments; /* DEVICE H x W x 2 f32 or NULL; read only with moments_out */
  void* color_out;          /* DEVICE H x W x 4 f32, required */
  void* length_out;         /* DEVICE H x W f32, required */
  void* moments_out;        /* DEVICE H x W x 2 f32 or NULL; requires hist_moments */
  void* variance_out;       /* DEVICE H x W f32 or NULL; needs moments_out */
};
typedef struct RaycaFilmFold RaycaFilmFold;
int32_t rayca_hip_film_fold_device(RaycaScene* scene, const RaycaRenderOptions* opts, const RaycaFilmFold* fold, RaycaStats* stats_out);

/* Post-build BVH read-back for parity tests against the oracle's literal SAH build:
 * `prim_order[i]` = index (in flatten order) of the primitive stored at slot i.  Buffers may be
 * NULL to query sizes through rayca_hip_scene_info. */
int32_t rayca_hip_scene_primitive_order(const RaycaScene* scene, uint32_t* prim_order,
                                        uint32_t capacity);

/* Node read-back for tests (no reference counterpart): copies the scene's binary nodes to HOST memory.
 * which = 0: the 64-B nodes (12 f32: min xyz, max xyz of the left child's box, then of the right child's; two u32 child
 * references; 8 B padding).  which = 1: the 48-B centre / half-extent records the conservative kernels of a
 * RAYCA_BUILDER_SAH scene read instead (RaycaStats.node_format bit 12; 12 f32: centre xyz, half extent xyz per child;
 * the low 16 bits of the x / y half extents of a child hold the low / high half of its reference, an inner reference
 * being the child record's byte offset, 48 x its index) -- node i of one is node i of the other.  `bytes_out` receives the array's size; with out == NULL only that.  RAYCA_ERR_BAD_ARG if the
 * scene has no such array or `capacity_bytes` is too small. */
int32_t rayca_hip_scene_read_nodes(RaycaScene* scene, uint32_t which, void* out, uint64_t capacity_bytes, uint64_t* bytes_out);

/* Light read-back (no reference counterpart): copies the scene's light records, as the kernels read them, to HOST memory -- in
 * flatten order, the index rayca_hip_direct_device's light_first counts in; after a rayca_hip_scene_update the updated records.
 * What a caller needs to reproduce a direct-light sample without restating the scene flatten: position is the translation of the
 * light node's LOCAL transform (w = 1), as the reference's NEE reads it (nee.rs:133-134), not the node's world position; normal
 * is normalized(ab x ac) and area the reference's own (1 - cos(ab, ac)) |ab| |ac| (|ab| |ac| for a rectangle) of a quad light,
 * zeros otherwise; attenuation[3] is 0.  `count_out` receives the
 * number of lights; with out == NULL only that.  RAYCA_ERR_BAD_ARG: NULL scene; out and count_out both NULL; `capacity` (in
 * records) too small. */
struct RaycaLightRecord {
  uint32_t kind;         /* RAYCA_LIGHT_* */
  uint32_t material;     /* a quad light's material, or RAYCA_NONE */
  float intensity;
  float area;
  float color[4];
  float attenuation[4];  /* constant, linear, quadratic, 0 */
  float position[4];
  float ab[4];
  float ac[4];
  float normal[4];
};
typedef struct RaycaLightRecord RaycaLightRecord;
int32_t rayca_hip_scene_read_lights(RaycaScene* scene, RaycaLightRecord* out, uint32_t capacity, uint32_t* count_out);

#ifdef __cplusplus
}
#endif
#endif /* RAYCA_HIP_H */
