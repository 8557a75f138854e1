// adaptive.inc -- the kernels behind rayca_hip_sample_plan_device and rayca_hip_film_fold_device (included from kernels.hip
// behind temporal.inc, inside its namespace): a film's variance decides where the next rays go (DESIGN 4.18).  The plan turns
// colour, variance and history length into one integer weight a pixel, the weights into ray offsets by an exact prefix sum, and
// the offsets into camera rays; the fold puts the ragged list of samples traced along them back into the film with k_accumulate's
// blend (temporal.inc film_blend).  The weight is f32 built from +, x, /, floor, min and max, one rounding per operation in the
// association the header writes; everything behind it is integer arithmetic, and no result depends on an order of execution: no
// atomics anywhere.  A literal restatement is tests/adaptive_literal.py.
//
// The prefix sum runs over the pixels in raster order.  Its first level is the wave: under the 64 x 4 tile prologue a wave is 64
// consecutive pixels of one row, a SEGMENT, and segment s = y * tiles_x + tx is the s-th of them in raster order.
//   k_plan_weights   a weight per pixel, a sum per segment
//   k_plan_scan      one block turns the segment sums into their exclusive prefix sums in place, chunk by chunk with a carry, and
//                    leaves the total behind them
//   k_plan_offsets   a wave rescans its segment, adds the segment's prefix, multiplies and divides
//   k_plan_rays      one ray per lane: a binary search over the offsets, then camera_ray() with the ray's own sub-pixel terms

constexpr int kPlanScanBlock = 1024, kPlanScanItems = 4;
constexpr uint32_t kPlanScanChunk = kPlanScanBlock * kPlanScanItems;   // segment sums one trip of k_plan_scan's loop covers

struct PlanIo {
  const float4* color;       // H x W
  const float* variance;     // H x W
  const float* length;       // H x W
  uint32_t* weight;          // H x W: weight_out, or the context's scratch
  uint32_t* sums;            // segments + 1: the segment sums, then (k_plan_scan) their exclusive prefix sums and the total
  uint32_t* offset;          // H x W + 1
  uint32_t width, height, tiles_x;
  uint32_t count;            // width * height
  uint32_t budget;
  uint32_t base_weight, fresh_weight;
  float min_history;         // (float)min_history
  float target2;             // target * target
  float lum_floor;
};

// inclusive sum over the wave's lanes below and at this one
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(v, d);
    if (lane >= (uint32_t)d) v += up;
  }
  return v;
}

// (segment = blockIdx.x's tile row and column with the wave's row: the lanes of a wave share it)
__device__ __forceinline__ uint32_t plan_segment(const PlanIo& io, const TilePixel& t) { return (uint32_t)t.y64 * io.tiles_x + (uint32_t)(t.x64 / kDenoiseTileW); }

__global__ __launch_bounds__(kBlock) void k_plan_weights(PlanIo io) {
  TilePixel t;
  const bool inside = tile_pixel(io.tiles_x, io.width, io.height, t);
  uint32_t w = 0u;
  if (inside) {
    const float4 c = io.color[t.p];
    const float d = fmaxf(luminance(c.x, c.y, c.z), io.lum_floor);
    const float v = fmaxf(io.variance[t.p], 0.0f);
    const float len = io.length[t.p];
    const float e = (v / fmaxf(len, 1.0f)) / (d * d);
    const float r = e / io.target2;
    const float steps = r >= 0.0f ? floorf(fminf(r, 255.0f)) : 0.0f;
    w = min(io.base_weight + (uint32_t)steps, 255u);
    if (!(len >= io.min_history)) w = max(w, io.fresh_weight);
    io.weight[t.p] = w;
  }
  // the wave's row lies in the image iff its first lane's pixel does (x of lane 0 is a tile's first column: inside)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t sum = wave_inclusive_sum(w, lane);
  if (lane == 63u && t.y64 < io.height) io.sums[plan_segment(io, t)] = sum;
}

// One block.  Thread i of a trip owns kPlanScanItems consecutive sums; a wave scans its lanes' totals, the block its waves'.
__global__ __launch_bounds__(kPlanScanBlock) void k_plan_scan(uint32_t* sums, uint32_t n) {
  __shared__ uint32_t wave_total[kPlanScanBlock / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0u;
  for (uint32_t base = 0u; base < n; base += kPlanScanChunk) {   // (n <= 2^24: no wrap)
    const uint32_t first = base + threadIdx.x * kPlanScanItems;
    uint32_t e[kPlanScanItems], mine = 0u;
#pragma unroll
    for (int k = 0; k < kPlanScanItems; ++k) {
      e[k] = first + k < n ? sums[first + k] : 0u;
      mine += e[k];
    }
    const uint32_t incl = wave_inclusive_sum(mine, lane);
    __syncthreads();   // the previous trip's reads of wave_total
    if (lane == 63u) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = carry, chunk = 0u;
#pragma unroll
    for (int v = 0; v < kPlanScanBlock / 64; ++v) {
      const uint32_t tot = wave_total[v];
      if ((uint32_t)v < wave) before += tot;
      chunk += tot;
    }
    uint32_t run = before + (incl - mine);
#pragma unroll
    for (int k = 0; k < kPlanScanItems; ++k) {
      if (first + k < n) sums[first + k] = run;
      run += e[k];
    }
    carry += chunk;
  }
  if (threadIdx.x == 0) sums[n] = carry;
}

__global__ __launch_bounds__(kBlock) void k_plan_offsets(PlanIo io, uint32_t segments) {
  TilePixel t;
  const bool inside = tile_pixel(io.tiles_x, io.width, io.height, t);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = inside ? io.weight[t.p] : 0u;
  const uint32_t incl = wave_inclusive_sum(w, lane);
  if (!inside) return;
  uint32_t total = io.sums[segments];
  uint32_t before = io.sums[plan_segment(io, t)] + (incl - w);
  if (total == 0u) {   // every weight counts as 1
    total = io.count;
    before = t.p;
  }
  // (before <= total <= 2^32 - 1, budget <= 2^31: the product fits 64 bits and the quotient is at most the budget)
  io.offset[t.p] = (uint32_t)((uint64_t)before * io.budget / total);
  if (t.p == io.count - 1u) io.offset[io.count] = io.budget;
}

struct PlanRaysIo {
  const uint32_t* offset;    // count + 1
  float* rays;               // budget x 6, or nullptr
  uint32_t* pixel;           // budget, or nullptr
  uint32_t count, budget;
  uint32_t jitter, strata;   // n, n * n
  uint32_t first_stratum;    // below strata
  float step;                // 1 / n as camera_sample_params forms it; fp.sub_offset is 0.5 / n
};

// Ray j belongs to the pixel p with offset[p] <= j < offset[p + 1]: one past it is the first entry above j (offset[0] = 0 <= j
// and offset[count] = budget > j, so that entry exists and is not the first).
__global__ __launch_bounds__(kBlock) void k_plan_rays(FrameParams fp, PlanRaysIo io) {
  __shared__ float stage[kBlock * kStageFloats];
  const uint64_t first = (uint64_t)rc_bid() * kBlock;
  const uint32_t j = (uint32_t)first + rc_tid();   // (first < budget <= 2^31)
  const bool in_range = first + rc_tid() < (uint64_t)io.budget;
  float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (in_range) {
    uint32_t lo = 0u, hi = io.count;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);   // (< count: inside the table)
      if (io.offset[mid] > j) hi = mid;
      else lo = mid + 1u;
    }
    const uint32_t p = lo ? lo - 1u : 0u;
    if (io.pixel) io.pixel[j] = p;
    if (io.rays) {
      const uint32_t s = (io.first_stratum + (j - io.offset[p])) % io.strata;
      const uint32_t iy = s / io.jitter, ix = s - iy * io.jitter;
      FrameParams mine = fp;
      mine.sub_step_x = (float)ix * io.step;
      mine.sub_step_y = (float)iy * io.step;
      const uint32_t y = p / fp.width, x = p - y * fp.width;
      const DRay ray = camera_ray(mine, x, y);
      v[0] = ray.o.x; v[1] = ray.o.y; v[2] = ray.o.z;
      v[3] = ray.d.x; v[4] = ray.d.y; v[5] = ray.d.z;
    }
  }
  if (io.rays) store_records<6>(io.rays, first, io.budget, v, stage);   // (uniform: every lane of the block takes it)
}

// ---- the fold: a ragged list of samples into a history -------------------------------------------------------------------------
struct FoldIo {
  const float4* samples;       // budget x 4
  const uint32_t* offset;      // H x W + 1
  const float4* hist_color;    // H x W
  const float* hist_length;    // H x W
  const float* hist_moments;   // H x W x 2 (MOMENTS)
  float4* color_out;
  float* length_out;
  float* moments_out;          // H x W x 2 (MOMENTS)
  float* variance_out;         // (MOMENTS) or nullptr
  uint32_t width, height, tiles_x;
  float cap;                   // (float)max_history, 0: unbounded
};

// One pixel per lane.  p's history is read before anything of p is written, so an output may be the history it continues.  A
// pixel's samples are consecutive 16-B records; neighbouring lanes read neighbouring runs.
template <bool MOMENTS>
__global__ __launch_bounds__(kBlock) void k_film_fold(FoldIo io) {
  TilePixel t;
  if (!tile_pixel(io.tiles_x, io.width, io.height, t)) return;
  const uint32_t p = t.p;
  const uint32_t begin = io.offset[p], end = io.offset[p + 1u];
  float4 o = io.hist_color[p];
  float n_out = io.hist_length[p], m1 = 0.0f, m2 = 0.0f;
  if (MOMENTS) {
    const float* m = io.hist_moments + 2ull * p;
    m1 = m[0]; m2 = m[1];
  }
  for (uint32_t j = begin; j < end; ++j) {
    // the state identity-mode k_accumulate takes from a history: present iff its length is > 0, else nothing of it counts
    const bool present = n_out > 0.0f;
    const float4 h = present ? o : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float len = present ? n_out : 0.0f, mx = present ? m1 : 0.0f, my = present ? m2 : 0.0f;
    const float4 c = io.samples[j];
    film_blend(present, h, len, mx, my, c, finite4(c), luminance(c.x, c.y, c.z), io.cap, o, n_out, m1, m2);
  }
  io.color_out[p] = o;
  io.length_out[p] = n_out;
  if (MOMENTS) {
    float* m = io.moments_out + 2ull * p;
    m[0] = m1; m[1] = m2;
    if (io.variance_out) io.variance_out[p] = fmaxf(m2 - m1 * m1, 0.0f);
  }
}
