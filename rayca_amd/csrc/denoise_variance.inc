// denoise_variance.inc -- the kernels behind rayca_hip_denoise_variance_device (included from kernels.hip behind denoise.inc,
// inside its namespace): the variance-guided a-trous filter on a frame, its luminance variance and its G-buffer in device memory
// (DESIGN 4.11).  The luminance edge-stopping weight scales with a local variance estimate, the variance is filtered along with
// the colour, and a pixel with a short history takes a spatial estimate instead of its temporal one.  Image space only: nothing
// of a scene is read.  As in denoise.inc every value is built from IEEE +, -, x, / and max (no exp, no sqrt, no pow), one
// rounding per operation in the association the header writes, so that a literal float32 restatement gives the same bits
// (tests/denoise_variance_literal.py).  Every comparison is written so that a NaN fails it; max is maxNum.  The demodulation and
// the output stage are denoise.inc's own kernels, launched as they are.

// What the initial-variance launch reads and writes; every pointer is DEVICE memory.
struct VarianceInitIo {
  const float4* color;     // H x W: the image the iterations start from (demodulated where there is an albedo)
  const float4* albedo;    // H x W, or nullptr
  const float* variance;   // H x W: the luminance variance of the accumulation
  const float* length;     // H x W (LENGTH)
  const float* normal;     // } the guides of the spatial estimate (SPATIAL), each as its flag says
  const float* point;      // }
  const uint32_t* id;      // }
  float* var_out;          // H x W: the first variance plane (never `variance`: a scratch plane of the context)
  uint32_t width, height;  // (width * height <= 2^32 - 1)
  uint32_t tiles_x;
  uint32_t normal_squarings;
  float kp;                // 1 / sigma_plane^2
  float min_history;       // (float)min_history (SPATIAL: > 0)
};

// v0: the temporal variance brought into the filter's units (over lum(den)^2 where demodulated, over the history length: the
// variance of the film's mean), or, in a lane whose history is shorter than min_history, the weighted variance of the luminance
// over the 7 x 7 neighbourhood.  The 49 taps are a per-lane branch: a wave of a converged film skips them.  k_atrous's layout.
template <bool LENGTH, bool SPATIAL, bool NORMAL, bool POINT, bool ID>
__global__ __launch_bounds__(kBlock) void k_variance_init(VarianceInitIo io) {
  static_assert(LENGTH || !SPATIAL, "the spatial estimate is chosen by the history length");
  TilePixel t;
  if (!tile_pixel(io.tiles_x, io.width, io.height, t)) return;
  const uint32_t p = t.p;
  float v = fmaxf(io.variance[p], 0.0f);   // (a NaN becomes 0)
  if (io.albedo) {
    const float4 den = denoise_den(io.albedo[p]);
    const float ld = luminance(den.x, den.y, den.z);
    v = v / (ld * ld);
  }
  float len = 0.0f;
  if (LENGTH) {
    len = io.length[p];
    v = v / fmaxf(len, 1.0f);
  }
  if (SPATIAL && len < io.min_history) {   // (false for a NaN length)
    const int64_t x = (int64_t)t.x64, y = (int64_t)t.y64;
    const GuideCentre g = guide_centre<NORMAL, POINT, ID>(io.normal, io.point, io.id, p);
    float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
#pragma unroll 1
    for (int dy = -3; dy <= 3; ++dy) {
      const int64_t qy = y + dy;
      if (qy < 0 || qy >= (int64_t)io.height) continue;
#pragma unroll
      for (int dx = -3; dx <= 3; ++dx) {
        const int64_t qx = x + dx;
        if (qx < 0 || qx >= (int64_t)io.width) continue;
        const uint32_t q = (uint32_t)((uint64_t)qy * io.width + (uint64_t)qx);
        const float4 cq = io.color[q];
        const float w = guide_weight<NORMAL, POINT>(1.0f, g, io.normal, io.point, q, io.normal_squarings, io.kp);
        const float lq = luminance(cq.x, cq.y, cq.z);
        bool take = w > 0.0f && lq - lq == 0.0f;   // (false for zero and NaN weights, and for a luminance that is not finite)
        if (ID) take = take && io.id[q] == g.idp;
        if (take) {
          s1 = s1 + w * lq;
          s2 = s2 + w * (lq * lq);
          ws = ws + w;
        }
      }
    }
    v = 0.0f;
    if (ws > 0.0f) {
      const float m1 = s1 / ws, m2 = s2 / ws;
      v = fmaxf(m2 - m1 * m1, 0.0f);
    }
  }
  io.var_out[p] = v;
}

// What one variance-guided iteration reads and writes; every pointer is DEVICE memory.  No input is an output.
struct AtrousVarIo {
  const float4* in;        // H x W colour of this iteration, alpha carried in .w
  float4* out;
  const float* var_in;     // H x W variance of this iteration
  float* var_out;
  const float* normal;     // H x W x 3, or nullptr
  const float* point;      // H x W x 3, or nullptr
  const uint32_t* id;      // H x W, or nullptr
  uint32_t width, height;  // (width * height <= 2^32 - 1: a pixel's index fits 32 bits, its float offsets are formed in 64)
  uint32_t tiles_x;        // blocks per tile row
  uint32_t step;           // 2^i
  uint32_t normal_squarings;
  float sl2;               // sigma_luminance^2
  float variance_floor;
  float kp;                // 1 / sigma_plane^2
};

// k_atrous's layout and tap order with the variance-guided luminance term in the colour term's place: the 3 x 3 prefilter of
// the variance at step 1 gives the term's denominator, and the variance goes through the taps with the squared weights (the
// variance of a weighted mean of independent values).  A tap moves 48 B where k_atrous moves 44, the prefilter 9 loads of 4 B.
template <bool NORMAL, bool POINT, bool ID>
__global__ __launch_bounds__(kBlock) void k_atrous_var(AtrousVarIo io) {
  TilePixel t;
  if (!tile_pixel(io.tiles_x, io.width, io.height, t)) return;
  const int64_t x = (int64_t)t.x64, y = (int64_t)t.y64, s = (int64_t)io.step;
  const uint32_t p = t.p;
  const float4 cp = io.in[p];
  const float vp = io.var_in[p];
  const GuideCentre g = guide_centre<NORMAL, POINT, ID>(io.normal, io.point, io.id, p);
  // the prefiltered variance: a 3 x 3 Gaussian at step 1 over the taps inside the image
  float gs = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const int64_t qy = y + dy;
    if (qy < 0 || qy >= (int64_t)io.height) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int64_t qx = x + dx;
      if (qx < 0 || qx >= (int64_t)io.width) continue;
      const float gk = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);   // (0.25, 0.125, 0.0625: exact constants)
      gs = gs + gk * io.var_in[(uint32_t)((uint64_t)qy * io.width + (uint64_t)qx)];
      gw = gw + gk;
    }
  }
  const float dnm = io.sl2 * (gs / gw) + io.variance_floor;
  const float lp = luminance(cp.x, cp.y, cp.z);
  constexpr float k[3] = {0.375f, 0.25f, 0.0625f};
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, vs = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = y + dy * s;
    if (qy < 0 || qy >= (int64_t)io.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = x + dx * s;
      if (qx < 0 || qx >= (int64_t)io.width) continue;
      const uint32_t q = (uint32_t)((uint64_t)qy * io.width + (uint64_t)qx);
      const float4 cq = io.in[q];
      float w = k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
      const float d = lp - luminance(cq.x, cq.y, cq.z);
      w = w / (1.0f + (d * d) / dnm);
      w = guide_weight<NORMAL, POINT>(w, g, io.normal, io.point, q, io.normal_squarings, io.kp);
      bool take = w > 0.0f;   // (false for zero and for NaN)
      if (ID) take = take && io.id[q] == g.idp;
      if (take) {
        sr = sr + w * cq.x;
        sg = sg + w * cq.y;
        sb = sb + w * cq.z;
        vs = vs + (w * w) * io.var_in[q];
        wsum = wsum + w;
      }
    }
  }
  float4 o = cp;   // no tap counted (a NaN colour, a zero normal at a miss): colour and variance pass through
  float vo = vp;
  if (wsum > 0.0f) {
    o.x = sr / wsum;
    o.y = sg / wsum;
    o.z = sb / wsum;
    vo = vs / (wsum * wsum);
  }
  io.out[p] = o;
  io.var_out[p] = vo;
}
