// upsample.inc -- the kernel behind rayca_hip_upsample_device (included from kernels.hip, inside its namespace): a joint
// bilateral upsample of a low-resolution frame onto a full-size G-buffer (DESIGN 4.12).  Image space only: nothing of a scene
// is read.  Every value is built from IEEE +, -, x, /, floor and max, one rounding per operation in the association the header
// writes, so that a literal float32 restatement gives the same bits (tests/upsample_literal.py).  Every comparison is written
// so that a NaN fails it; max is maxNum.

// What the pass reads and writes; every pointer is DEVICE memory.  No output is one of the inputs.
struct UpsampleIo {
  const float4* color;         // h x w, gamma 1
  const float4* albedo_low;    // h x w (ALBEDO)
  const float* normal_low;     // h x w x 3 (NORMAL)
  const float* point_low;      // h x w x 3 (POINT)
  const uint32_t* id_low;      // h x w (ID)
  const float4* albedo;        // H x W (ALBEDO)
  const float* normal;         // H x W x 3 (NORMAL)
  const float* point;          // H x W x 3 (POINT)
  const uint32_t* id;          // H x W (ID)
  float4* rgba32f;             // H x W, or nullptr
  uint8_t* rgba8;              // H x W x 4, or nullptr
  float* weight;               // H x W, or nullptr
  uint32_t width, height;      // H x W (width * height <= 2^32 - 1: a pixel's index fits 32 bits, its float offsets are formed in 64)
  uint32_t low_width, low_height;   // width / scale, height / scale, both exact
  uint32_t tiles_x;            // blocks per tile row
  uint32_t scale;              // 1..8
  uint32_t normal_squarings;
  float s;                     // (float)scale
  float kp;                    // 1 / sigma_plane^2
  float inv_gamma;
};

// One output pixel per lane, the denoiser's 64 x 4 tile per block: a wave is 64 consecutive pixels of an output row, which
// lie over at most 64 / scale + 2 low pixels of two rows -- the scale x scale pixels under one low pixel share their four
// taps, so the low image comes out of L1 and what crosses the memory bus is the full-size guides and the output.  The
// guided sums and the unguided ones of the fallback run side by side in the one loop over the four taps (they share every
// load; the unguided five accumulators exist only where a guide can reject a tap).  A template flag per optional guide: an
// absent one costs nothing.
template <bool ALBEDO, bool NORMAL, bool POINT, bool ID>
__global__ __launch_bounds__(kBlock) void k_upsample(UpsampleIo io) {
  constexpr bool GUIDED = NORMAL || ID;   // (POINT needs NORMAL; the albedo rejects no tap)
  TilePixel t;
  if (!tile_pixel(io.tiles_x, io.width, io.height, t)) return;
  const uint32_t x = (uint32_t)t.x64, y = (uint32_t)t.y64;
  const uint32_t p = t.p;
  const float fx = ((float)x + 0.5f) / io.s - 0.5f, fy = ((float)y + 0.5f) / io.s - 0.5f;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float tx = fx - x0f, ty = fy - y0f;
  const int64_t x0 = (int64_t)x0f, y0 = (int64_t)y0f;   // (in [-1, 2^32]: exact)

  const GuideCentre g = guide_centre<NORMAL, POINT, ID>(io.normal, io.point, io.id, p);
  const bool miss = NORMAL && g.npx == 0.0f && g.npy == 0.0f && g.npz == 0.0f;

  float wsum = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f;   // the guided pass
  float bsum = 0.0f, br = 0.0f, bg = 0.0f, bb = 0.0f, ba = 0.0f;   // the fallback: w = b alone
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t qy = y0 + j;
    if (qy < 0 || qy >= (int64_t)io.low_height) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t qx = x0 + i;
      if (qx < 0 || qx >= (int64_t)io.low_width) continue;
      const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
      if (!(b > 0.0f)) continue;
      const uint32_t q = (uint32_t)((uint64_t)qy * io.low_width + (uint64_t)qx);   // (inside the low image: < w * h <= width * height)
      float4 c = io.color[q];
      if (!finite4(c)) continue;
      if (ALBEDO) c = demodulate(c, io.albedo_low[q]);
      if (GUIDED) {
        bsum = bsum + b;
        br = br + b * c.x;
        bg = bg + b * c.y;
        bb = bb + b * c.z;
        ba = ba + b * c.w;
      }
      float w = b;
      bool take = true;
      if (NORMAL) {
        // guide_weight's two terms, written out: the tap's normal is loaded once, in front of the miss rule
        const float* n = io.normal_low + 3ull * q;
        const float nqx = n[0], nqy = n[1], nqz = n[2];
        if (miss) {
          take = nqx == 0.0f && nqy == 0.0f && nqz == 0.0f;   // a miss takes misses only, by b alone
        } else {
          float dn = fmaxf((g.npx * nqx + g.npy * nqy) + g.npz * nqz, 0.0f);
          for (uint32_t k = 0; k < io.normal_squarings; ++k) dn = dn * dn;
          w = w * dn;
          if (POINT) {
            const float* xq = io.point_low + 3ull * q;
            const float ex = xq[0] - g.ppx, ey = xq[1] - g.ppy, ez = xq[2] - g.ppz;
            const float pd = (g.npx * ex + g.npy * ey) + g.npz * ez;
            w = w / (1.0f + (pd * pd) * io.kp);
          }
        }
      }
      if (ID) take = take && io.id_low[q] == g.idp;
      if (take && w > 0.0f) {   // (false for zero and for NaN)
        wsum = wsum + w;
        sr = sr + w * c.x;
        sg = sg + w * c.y;
        sb = sb + w * c.z;
        sa = sa + w * c.w;
      }
    }
  }

  float4 o;
  if (wsum > 0.0f) {
    o = make_float4(sr / wsum, sg / wsum, sb / wsum, sa / wsum);
  } else if (GUIDED && bsum > 0.0f) {   // no tap agrees with the pixel's surface: plain bilinear over the taps that exist
    o = make_float4(br / bsum, bg / bsum, bb / bsum, ba / bsum);
  } else {   // no tap exists (NaN neighbourhoods): the nearest low pixel, whatever it holds
    const uint32_t ny = min(y / io.scale, io.low_height - 1u), nx = min(x / io.scale, io.low_width - 1u);
    const uint32_t q = (uint32_t)((uint64_t)ny * io.low_width + nx);
    o = io.color[q];
    if (ALBEDO) o = demodulate(o, io.albedo_low[q]);
  }
  if (io.weight) io.weight[p] = wsum;
  if (ALBEDO) o = remodulate(o, io.albedo[p]);
  write_display_pixel(o, io.inv_gamma, p, io.rgba8, io.rgba32f);
}
