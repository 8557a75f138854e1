// refill.hpp -- host-side entry of the lane-refill camera-ray kernel (refill.hip), called from api.inc.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"
#include "flavour.hpp"

namespace rayca {

struct RefillFlavour {
  Trav trav;   // one of the six kTravFast* (k_flat_refill reads its WIDE, SPILL and HALF)
  bool sph, stats;
};
// host stub of the instantiation (for hipFuncGetAttributes) and its launch
const void* flat_refill_kernel(const RefillFlavour& f);
void launch_flat_refill(const RefillFlavour& f, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const FrameParams& fp, uint32_t* heads,
                        uint8_t* rgba8, float4* rgba32f, TraceCounters* counters, const TraceLaunch& tl);

// the same for the rays of a queue (closest hits of a bounce generation of the wavefront engine; 4-wide fp16 nodes).  slack: the
// queue holds a caller's rays (rayca_hip_radiance_device), not rays that start on the scene's surfaces
const void* queue_refill_kernel(bool sph, bool stats, bool slack);
void launch_queue_refill(bool sph, bool stats, bool slack, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const QueuedRay* in_rays,
                         const uint32_t* in_count, float4* hits, uint32_t* heads, TraceCounters* counters, const TraceLaunch& tl);

// the same for rays the caller keeps in device memory (rayca_hip_query_device): closest hit or occlusion, with a distance bound
const void* query_refill_kernel(bool occluded, bool sph, bool stats);
void launch_query_refill(bool occluded, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const QueryIo& q,
                         uint32_t* heads, TraceCounters* counters, const TraceLaunch& tl);

// the same for the hemisphere rays of rayca_hip_ambient_device: made in registers from points, normals and a direction table, one bit
// of the point's mask word per occluded ray.  rot: the call has a rotation array
const void* ambient_refill_kernel(bool rot, bool sph, bool stats);
void launch_ambient_refill(bool rot, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const AmbientIo& a,
                           uint32_t* heads, TraceCounters* counters, const TraceLaunch& tl);

// the same for the eight corner rays of rayca_hip_probe_lookup_device: made in registers from a point and its cell of the probe grid,
// one bit of the point's mask word per occluded ray
const void* probe_refill_kernel(bool sph, bool stats);
void launch_probe_refill(bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const ProbeIo& a, uint32_t* heads,
                         TraceCounters* counters, const TraceLaunch& tl);

// the same for the shadow rays of rayca_hip_direct_device: made in registers from a point, its optional normal and a light's record,
// one bit of the point's mask word per lit sample.  sphere: the call has no normals
const void* direct_refill_kernel(bool sphere, bool sph, bool stats);
void launch_direct_refill(bool sphere, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const DirectIo& a, uint32_t* heads,
                          TraceCounters* counters, const TraceLaunch& tl);

// and for the shadow-ray pass of a generation (k_wf_shadow's work)
struct ShadowRefillArgs {
  float4* sh_ray;
  float4* sh_x;
  uint32_t nls;
  float4* direct;
  uint32_t* state;
  uint32_t npix;
};
const void* shadow_refill_kernel(bool gen0, bool sph, bool stats);
void launch_shadow_refill(bool gen0, bool sph, bool stats, uint32_t grid, size_t lds_bytes, hipStream_t stream, const DevScene& sc, const FrameParams& fp,
                          const QueuedRay* in_rays, const uint32_t* in_count, const ShadowRefillArgs& a, uint32_t depth, uint32_t* heads,
                          TraceCounters* counters, const TraceLaunch& tl);

}  // namespace rayca
