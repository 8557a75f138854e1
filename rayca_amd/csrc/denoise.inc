// denoise.inc -- the kernels behind rayca_hip_denoise_device (included from kernels.hip, inside its namespace): the
// edge-avoiding a-trous wavelet filter on a frame and its G-buffer in device memory (DESIGN 4.9).  Image space only: nothing
// of a scene is read.  Every weight is built from IEEE +, -, x, / and max (no exp, no pow inside the filter), one rounding
// per operation in the association written here, so that a literal float32 restatement gives the same bits
// (tests/denoise_literal.py).  max is maxNum: a NaN operand gives the other one.

// What one a-trous iteration reads and writes; every pointer is DEVICE memory.  `in` and `out` are never the same image.
struct AtrousIo {
  const float4* in;        // H x W colour of this iteration (demodulated where there is an albedo), alpha carried in .w
  float4* out;
  const float* normal;     // H x W x 3, or nullptr
  const float* point;      // H x W x 3, or nullptr
  const uint32_t* id;      // H x W, or nullptr
  uint32_t width, height;  // (width * height <= 2^32 - 1: a pixel's index fits 32 bits, its float offsets are formed in 64)
  uint32_t tiles_x;        // blocks per tile row
  uint32_t step;           // 2^i
  uint32_t normal_squarings;
  float kc, kp;            // 1 / sigma_color^2, 1 / sigma_plane^2
};

// One pixel per lane, a 64 x 4 tile per block: the 64 lanes of a wave read one 1-KiB run of float4 colour per tap, and a
// dilated tap is the same run shifted by dx * step pixels.  The 25 taps go dy = -2..2 (outer), dx = -2..2 (inner) into one
// running sum; p's own colour and guides stay in registers.  A template flag per term: an absent guide costs nothing.
template <bool COLOR, bool NORMAL, bool POINT, bool ID>
__global__ __launch_bounds__(kBlock) void k_atrous(AtrousIo io) {
  // tile_pixel's lines, written out: through the helper the two bounds tests become one branch and this kernel's SGPR count moves
  const uint32_t ty = blockIdx.x / io.tiles_x, tx = blockIdx.x - ty * io.tiles_x;
  const uint64_t x64 = (uint64_t)tx * kDenoiseTileW + (threadIdx.x & (kDenoiseTileW - 1));
  const uint64_t y64 = (uint64_t)ty * kDenoiseTileH + (threadIdx.x / kDenoiseTileW);
  if (x64 >= io.width || y64 >= io.height) return;
  const int64_t x = (int64_t)x64, y = (int64_t)y64, s = (int64_t)io.step;
  const uint32_t p = (uint32_t)(y64 * io.width + x64);   // (< width * height)
  const float4 cp = io.in[p];
  const GuideCentre g = guide_centre<NORMAL, POINT, ID>(io.normal, io.point, io.id, p);
  constexpr float k[3] = {0.375f, 0.25f, 0.0625f};
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
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
      if (COLOR) {
        const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
        const float dc = (dr * dr + dg * dg) + db * db;
        w = w / (1.0f + dc * io.kc);
      }
      w = guide_weight<NORMAL, POINT>(w, g, io.normal, io.point, q, io.normal_squarings, io.kp);
      bool take = w > 0.0f;   // (false for zero and for NaN)
      if (ID) take = take && io.id[q] == g.idp;
      if (take) {
        sr = sr + w * cq.x;
        sg = sg + w * cq.y;
        sb = sb + w * cq.z;
        wsum = wsum + w;
      }
    }
  }
  float4 o = cp;   // no tap counted (a NaN colour, a zero normal at a miss): the pixel passes through
  if (wsum > 0.0f) {
    o.x = sr / wsum;
    o.y = sg / wsum;
    o.z = sb / wsum;
  }
  io.out[p] = o;
}

// colour / den -> out, alpha as it is (pixel-local)
__global__ __launch_bounds__(kBlock) void k_denoise_demod(const float4* color, const float4* albedo, float4* out, uint32_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (uint64_t)count) return;
  out[i] = demodulate(color[i], albedo[i]);
}

// The output stage (pixel-local): remodulate where `albedo` is given, then gamma and RGBA8 as a render call's last kernel
// does them (write_display_pixel).  `in` is never one of the outputs.
__global__ __launch_bounds__(kBlock) void k_denoise_finish(const float4* in, const float4* albedo, float inv_gamma, uint8_t* rgba8, float4* rgba32f, uint32_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (uint64_t)count) return;
  float4 c = in[i];
  if (albedo) c = remodulate(c, albedo[i]);
  write_display_pixel(c, inv_gamma, (uint32_t)i, rgba8, rgba32f);
}
