// sample.inc -- surface sampling (rayca_hip_surface_cdf_device, rayca_hip_surface_sample_device): area-weighted points on the
// scene's triangles, in device memory.  Included from kernels.hip inside the no-packed-f32 region, behind surface.inc and
// nearest.inc: load_tri of trace_core.inc, store_records of surface.inc.  The header's comments on RaycaSurfaceCdf and
// RaycaSurfaceSample are the specification; slot_area and the sampler's tail are that text, operation by operation (no FMA: the
// unit is built with -ffp-contract=off).  Neither kernel traverses anything.  A literal restatement is tests/sample_literal.py.
//
// The table is adaptive.inc's pattern on the primitive records: an integer weight per slot, an exact prefix sum, a binary search
// per output.  Areas become integers by an exponent shift that depends on the largest area alone, and that maximum is the one
// atomic here: an integer maximum over the bits of non-negative floats, which order as the floats do, so no result depends on
// an order of execution.
//   k_cdf_amax      a slot per lane: its area, the wave's maximum, one atomicMax per wave
//   k_cdf_weights   a slot per lane: its area again (48 B re-read, no scratch array), the weight into cdf[i + 1]
//   k_cdf_scan      one block turns cdf[1 .. T] into its inclusive prefix sums in place, chunk by chunk with a carry
//                   (k_plan_scan's shape with 64-bit sums)
//   k_sample_surface  a sample per lane: two hash words into a target below the total, the binary search, the barycentrics

constexpr int kCdfScanBlock = 1024, kCdfScanItems = 4;
constexpr uint32_t kCdfScanChunk = kCdfScanBlock * kCdfScanItems;   // entries one trip of k_cdf_scan's loop covers

struct SurfaceCdfIo {
  const uint8_t* include;      // prim_count bytes, or nullptr: every slot
  uint32_t* amax;              // one word of the context's scratch, cleared in front of k_cdf_amax: the largest area's bits
  unsigned long long* cdf;     // prim_count + 1
};

// edges, normal and squared length of the normal of a slot's triangle, as the header writes them
struct SlotGeometry {
  float ax, ay, az, abx, aby, abz, acx, acy, acz;
  float nx, ny, nz, a2;
};
__device__ __forceinline__ SlotGeometry slot_geometry(const TriRecord& tr) {
  SlotGeometry g;
  g.ax = tr.v0.x; g.ay = tr.v0.y; g.az = tr.v0.z;
  g.abx = tr.v1.x - g.ax; g.aby = tr.v1.y - g.ay; g.abz = tr.v1.z - g.az;
  g.acx = tr.v2.x - g.ax; g.acy = tr.v2.y - g.ay; g.acz = tr.v2.z - g.az;
  g.nx = g.aby * g.acz - g.abz * g.acy;
  g.ny = g.abz * g.acx - g.abx * g.acz;
  g.nz = g.abx * g.acy - g.aby * g.acx;
  g.a2 = (g.nx * g.nx + g.ny * g.ny) + g.nz * g.nz;
  return g;
}
// The area a slot counts with: twice the triangle's, since the common factor does not change a share.  sqrtf is the build's
// correctly rounded square root (llvm.sqrt.f32 under the compiler's default of correctly rounded f32 division and square root;
// this toolchain's __fsqrt_rn is the approximate native one and is not used).  NaN and +inf fail the comparison: 0.
__device__ __forceinline__ float slot_area(const DevScene& sc, uint32_t i, const uint8_t* include) {
  if (include && include[i] == 0) return 0.0f;
  const float area = sqrtf(slot_geometry(load_tri(sc, i)).a2);
  return area <= FLT_MAX ? area : 0.0f;
}

__global__ __launch_bounds__(kBlock) void k_cdf_amax(DevScene sc, SurfaceCdfIo io) {
  const uint32_t i = rc_bid() * kBlock + rc_tid();   // (prim_count <= 2^25: no wrap)
  uint32_t bits = i < sc.prim_count ? __float_as_uint(slot_area(sc, i, io.include)) : 0u;
  for (int off = 32; off > 0; off >>= 1) bits = max(bits, (uint32_t)__shfl_down(bits, off));
  if (__lane_id() == 0 && bits != 0u) atomicMax(io.amax, bits);
}

// amax = m * 2^e with 0.5 <= m < 1, from its bits.  (An area that counts is the root of an a2 >= 2^-149: at least 2^-75, never a
// denormal.  So -127 < 32 - e <= 106, and the shift below is a product with a power of two that is an f32.)
__device__ __forceinline__ int area_exponent(uint32_t bits) { return (int)(bits >> 23) - 126; }

__global__ __launch_bounds__(kBlock) void k_cdf_weights(DevScene sc, SurfaceCdfIo io) {
  const uint32_t i = rc_bid() * kBlock + rc_tid();
  if (i >= sc.prim_count) return;
  const uint32_t amax = *io.amax;
  uint32_t w = 0u;
  if (amax != 0u) {
    // area < 2^e: the shifted area is below 2^32, and exact unless it underflows -- then it is below 1 and its floor is 0
    const float shifted = ldexpf(slot_area(sc, i, io.include), 32 - area_exponent(amax));
    w = (uint32_t)floorf(shifted);
  }
  io.cdf[i + 1u] = w;
  if (i == 0u) io.cdf[0] = 0ull;
}

__device__ __forceinline__ unsigned long long wave_inclusive_sum64(unsigned long long v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(v, d);
    if (lane >= (uint32_t)d) v += up;
  }
  return v;
}

// One block.  Thread i of a trip owns kCdfScanItems consecutive entries; a wave scans its lanes' totals, the block its waves'.
// Inclusive and in place: v[k] becomes v[0] + ... + v[k].
__global__ __launch_bounds__(kCdfScanBlock) void k_cdf_scan(unsigned long long* v, uint32_t n) {
  __shared__ unsigned long long wave_total[kCdfScanBlock / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long carry = 0ull;
  for (uint32_t base = 0u; base < n; base += kCdfScanChunk) {   // (n <= 2^25: no wrap)
    const uint32_t first = base + threadIdx.x * kCdfScanItems;
    unsigned long long e[kCdfScanItems], mine = 0ull;
#pragma unroll
    for (int k = 0; k < kCdfScanItems; ++k) {
      e[k] = first + k < n ? v[first + k] : 0ull;
      mine += e[k];
    }
    const unsigned long long incl = wave_inclusive_sum64(mine, lane);
    __syncthreads();   // the previous trip's reads of wave_total
    if (lane == 63u) wave_total[wave] = incl;
    __syncthreads();
    unsigned long long before = carry, chunk = 0ull;
#pragma unroll
    for (int u = 0; u < kCdfScanBlock / 64; ++u) {
      const unsigned long long tot = wave_total[u];
      if ((uint32_t)u < wave) before += tot;
      chunk += tot;
    }
    unsigned long long run = before + (incl - mine);
#pragma unroll
    for (int k = 0; k < kCdfScanItems; ++k) {
      run += e[k];
      if (first + k < n) v[first + k] = run;
    }
    carry += chunk;
  }
}

struct SurfaceSampleIo {
  const unsigned long long* cdf;   // prim_count + 1
  uint32_t count, seed, sample, first_index;
  uint32_t* prim_out;              // any of the four may be nullptr
  float* uv_out;                   // x 2
  float* point_out;                // x 3
  float* normal_out;               // x 3
};

// One sample per lane.  GEOM: point_out or normal_out is given -- the drawn slot's record is read; prim and uv need the table
// alone.  The search keeps cdf[lo] <= target < cdf[hi] from (0, T) on -- cdf[0] = 0 and cdf[T] = total > target -- so it ends at
// the one slot whose interval holds the target, and that interval is not empty: a slot of weight 0 is never drawn.  Its upper
// levels are the same entries for every lane and stay in the caches; a coarse table in LDS in front of it was not built.
template <bool GEOM>
__global__ __launch_bounds__(kBlock) void k_sample_surface(DevScene sc, SurfaceSampleIo io) {
  __shared__ float stage[kBlock * 3];
  const uint64_t first = (uint64_t)rc_bid() * kBlock;
  const uint64_t j = first + rc_tid();   // (count may be 2^32 - 1: the last block's lanes behind it must not wrap into range)
  const bool in_range = j < (uint64_t)io.count;
  uint32_t prim = RAYCA_NONE;
  float s = 0.0f, t = 0.0f, u = 0.0f;
  float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
  if (in_range) {
    const uint32_t slots = sc.prim_count;
    const unsigned long long total = io.cdf[slots];
    if (total != 0ull) {
      const uint32_t key = rng_root(io.seed, io.first_index + (uint32_t)j, io.sample);
      const unsigned long long r = (unsigned long long)rng_word(key, 0u) << 32 | rng_word(key, 1u);
      const unsigned long long target = __umul64hi(r, total);   // floor(r * total / 2^64) < total
      uint32_t lo = 0u, hi = slots;
      while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (io.cdf[mid] <= target) lo = mid;
        else hi = mid;
      }
      prim = lo;
      const float s0 = rng_f32(key, 2u), t0 = rng_f32(key, 3u);
      const bool fold = s0 + t0 > 1.0f;
      s = fold ? 1.0f - s0 : s0;
      t = fold ? 1.0f - t0 : t0;
      u = (1.0f - s) - t;
      if (GEOM) {
        const SlotGeometry g = slot_geometry(load_tri(sc, prim));
        p[0] = (g.ax + g.abx * s) + g.acx * t;
        p[1] = (g.ay + g.aby * s) + g.acy * t;
        p[2] = (g.az + g.abz * s) + g.acz * t;
        const float len = sqrtf(g.a2);
        n[0] = g.nx / len; n[1] = g.ny / len; n[2] = g.nz / len;
      }
    }
  }
  if (io.prim_out && in_range) io.prim_out[j] = prim;
  if (io.uv_out) {   // (weight of vertex 0, weight of vertex 1): what shade_hit reads of a hit record
    const float v[2] = {u, s};
    store_records<2>(io.uv_out, first, io.count, v, stage);
  }
  if (GEOM && io.point_out) store_records<3>(io.point_out, first, io.count, p, stage);
  if (GEOM && io.normal_out) store_records<3>(io.normal_out, first, io.count, n, stage);
}
