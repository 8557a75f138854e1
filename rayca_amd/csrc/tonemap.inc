// tonemap.inc -- the kernels behind rayca_hip_meter_device and rayca_hip_tonemap_device (included from kernels.hip, inside its
// namespace): a luminance histogram of a linear frame, the exposure record made from it, and the display transform that reads
// that record (DESIGN 4.13).  Image space only: nothing of a scene is read.  Every f32 value is built from IEEE +, -, x and /,
// one rounding per operation in the association the header writes, and everything behind a pixel's luminance is integer
// arithmetic, so that a literal restatement gives the same words (tests/tonemap_literal.py).  Every comparison is written so
// that a NaN fails it.  No float atomic anywhere: the only atomics add integers, which commute.

constexpr uint32_t kMeterBins = 256;       // 8 an octave over 2^-16 .. 2^16
constexpr uint32_t kMeterCounted = 256, kMeterBlack = 257, kMeterNotFinite = 258;
constexpr uint32_t kMeterWords = 260;      // hist_out: the bins, counted, black, not finite, 0
constexpr uint32_t kMeterLive = 259;       // the words the kernels add to (the last one stays the clear's zero)
constexpr int kMeterBlock = 1024;          // lanes a block: few, large blocks -- every block ends in up to 259 global atomics (DESIGN 4.13)
constexpr uint32_t kMeterMaxGrid = 256;    // blocks: one per CU, 16 waves each; a larger frame strides (the cap was swept: DESIGN 4.13)
constexpr int kMeterBinBias = (127 - 16) << 3;

struct MeterIo {
  const float4* color;   // H x W, gamma 1
  uint32_t* hist;        // kMeterWords, cleared in front of the launch
  uint32_t count;        // width * height (<= 2^32 - 1)
};

// The histogram.  A grid-stride loop under a capped grid, one 16-byte load per pixel.  The bins of a block live in LDS, one copy
// per wave, which keeps the waves of a block off each other's words (one copy per block was measured slower, DESIGN 4.13), and
// take one integer LDS atomic per counted pixel; the three totals are counted in registers.  Behind the loop every word that is
// not zero goes to the global histogram with one integer atomic: at most 259 per block, whatever the frame's size.  Those atomics
// meet on the nine lines of hist_out and set the kernel's time once there are many blocks, hence few blocks of 1024 lanes.
__global__ __launch_bounds__(kMeterBlock) void k_meter_hist(MeterIo io) {
  constexpr uint32_t kCopies = kMeterBlock / 64;
  __shared__ uint32_t bins[kCopies][kMeterWords];
  for (uint32_t w = threadIdx.x; w < kCopies * kMeterWords; w += kMeterBlock) (&bins[0][0])[w] = 0u;
  __syncthreads();
  uint32_t* const mine = bins[threadIdx.x / 64];
  uint32_t counted = 0, black = 0, not_finite = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kMeterBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kMeterBlock + threadIdx.x; i < io.count; i += stride) {   // (i < 2^32 inside the loop)
    const float4 c = io.color[i];
    // Alpha is not looked at, and without a use of it the compiler narrows the load to 12 bytes (global_load_dwordx3).  The empty
    // statement names c.w and keeps it one aligned global_load_dwordx4 a lane.  Checked in the ISA of this kernel (hipcc -S
    // --cuda-device-only, the loads of k_meter_hist): one global_load_dwordx4, no dwordx3; look again after a compiler change.
    asm volatile("" ::"v"(c.w));
    const float y = luminance(c.x, c.y, c.z);
    if (!((c.x - c.x == 0.0f) && (c.y - c.y == 0.0f) && (c.z - c.z == 0.0f) && (y - y == 0.0f))) {
      ++not_finite;
    } else if (y <= 0.0f) {
      ++black;
    } else {
      const int bin = (int)(__float_as_uint(y) >> 20) - kMeterBinBias;   // (y > 0: the sign bit is clear)
      atomicAdd(&mine[min(max(bin, 0), (int)kMeterBins - 1)], 1u);
      ++counted;
    }
  }
  if (counted) atomicAdd(&mine[kMeterCounted], counted);
  if (black) atomicAdd(&mine[kMeterBlack], black);
  if (not_finite) atomicAdd(&mine[kMeterNotFinite], not_finite);
  __syncthreads();
  for (uint32_t w = threadIdx.x; w < kMeterLive; w += kMeterBlock) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCopies; ++k) v += bins[k][w];
    if (v) atomicAdd(&io.hist[w], v);
  }
}

struct ExposureIo {
  const uint32_t* hist;    // the finished histogram (a launch of its own: behind every block of k_meter_hist)
  float* out;              // {scale, target, L, 0}
  const float* prev;       // or nullptr; may be `out`
  uint32_t low_permille, high_permille;
  float key, min_scale, max_scale, rate;
};

// The exposure record: one wave, four bins a lane.  The running counts are a wave prefix sum, the two sums a wave reduction,
// all in integers; lane 0 alone forms the few f32 values and writes the record (having read `prev`, which may be `out`).
__global__ __launch_bounds__(64) void k_exposure(ExposureIo io) {
  const uint32_t lane = threadIdx.x;
  const uint32_t* const h = io.hist + 4u * lane;   // bins 4 lane .. 4 lane + 3 (hist_out is aligned as its words: four loads)
  const uint32_t hv[4] = {h[0], h[1], h[2], h[3]};
  const uint32_t own = (hv[0] + hv[1]) + (hv[2] + hv[3]);   // (no carry: the bins sum to counted < 2^32)
  uint32_t incl = own;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off);
    if (lane >= (uint32_t)off) incl += up;
  }
  const uint64_t n = io.hist[kMeterCounted];
  const uint64_t a = n * io.low_permille / 1000u, b = n * io.high_permille / 1000u;
  uint64_t c0 = incl - own, k_sum = 0, t_sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint64_t c1 = c0 + hv[j];
    const uint64_t hi = c1 < b ? c1 : b, lo = c0 > a ? c0 : a;
    const uint64_t k = hi > lo ? hi - lo : 0u;
    k_sum += k;
    t_sum += k * (2u * (4u * lane + j) + 1u);
    c0 = c1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    k_sum += __shfl_down(k_sum, off);
    t_sum += __shfl_down(t_sum, off);
  }
  if (lane != 0) return;
  float p = 0.0f;
  bool usable = false;
  if (io.prev) {
    p = io.prev[0];
    usable = p > 0.0f && p - p == 0.0f;
  }
  float lum = 0.0f, target = usable ? p : 1.0f;
  if (k_sum != 0) {
    const uint64_t q = (t_sum << 12) / k_sum;   // (t_sum <= 511 k_sum < 2^41; q < 2^21)
    lum = (1.0f + (float)(uint32_t)(q & 0xffffu) / 65536.0f) * __uint_as_float(((uint32_t)(q >> 16) + (127u - 16u)) << 23);
    target = fminf(fmaxf(io.key / lum, io.min_scale), io.max_scale);
  }
  const float scale = usable ? p + (target - p) * io.rate : target;
  *reinterpret_cast<float4*>(io.out) = make_float4(scale, target, lum, 0.0f);
}

enum : int { kTonemapLinear = 0, kTonemapReinhard = 1, kTonemapAces = 2 };

struct TonemapIo {
  const float4* color;       // H x W, gamma 1
  const float* exposure;     // word 0 is the scale, or nullptr: `scale`
  float4* rgba32f;           // H x W, or nullptr; may be `color`
  uint8_t* rgba8;            // H x W x 4, or nullptr
  uint32_t width, height;
  uint32_t tiles_x;          // blocks per tile row
  float scale;
  float inv_white2;          // 1 / white^2, or 0
  float inv_gamma;
};

__device__ __forceinline__ float tonemap_aces(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

// One pixel per lane, the denoiser's 64 x 4 tile per block.  A lane reads its own pixel before it writes it, so rgba32f may be
// color.  The operator and the outputs are template flags: an absent output costs nothing.
template <int OP, bool F32, bool U8>
__global__ __launch_bounds__(kBlock) void k_tonemap(TonemapIo io) {
  TilePixel t;
  if (!tile_pixel(io.tiles_x, io.width, io.height, t)) return;
  const uint32_t p = t.p;
  const float s = io.exposure ? io.exposure[0] : io.scale;
  const float4 c = io.color[p];
  float4 o = make_float4(c.x * s, c.y * s, c.z * s, c.w);
  if (OP == kTonemapReinhard) {
    const float y = luminance(o.x, o.y, o.z);
    if (y > 0.0f) {
      const float m = (1.0f + y * io.inv_white2) / (1.0f + y);
      o.x = o.x * m;
      o.y = o.y * m;
      o.z = o.z * m;
    }
  } else if (OP == kTonemapAces) {
    o.x = tonemap_aces(o.x);
    o.y = tonemap_aces(o.y);
    o.z = tonemap_aces(o.z);
  }
  write_display_pixel(o, io.inv_gamma, p, U8 ? io.rgba8 : nullptr, F32 ? io.rgba32f : nullptr);
}
