// image_pass.inc -- what the image-space post passes share on the device (included from kernels.hip in front of denoise.inc,
// inside its namespace): the 64 x 4 tile a block covers, a pixel's guides and the guide terms of a tap, and the small colour
// helpers.  Every helper is __forceinline__ and holds the operations of the kernels it was written out in, in their
// association, one rounding each (-ffp-contract=off), every comparison written so that a NaN fails it: the bit-exactness
// contract of the files behind it (DESIGN 4.9-4.13, the literals under tests/) holds through each of them.

constexpr int kDenoiseTileW = 64, kDenoiseTileH = kBlock / kDenoiseTileW;   // a wave = 64 consecutive pixels of one row

// The pixel of this lane: one pixel per lane, a 64 x 4 tile per block, the blocks row by row over `tiles_x` tiles a row.
struct TilePixel {
  uint64_t x64, y64;
  uint32_t p;   // y * width + x (< width * height <= 2^32 - 1; a pixel's float offsets are formed in 64 bits)
};
// false: the lane lies past the image's right or lower edge and has nothing to do
__device__ __forceinline__ bool tile_pixel(uint32_t tiles_x, uint32_t width, uint32_t height, TilePixel& t) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  // (tx * 64 <= width - 1 and ty * 4 <= height - 1, so neither sum passes 2^32 + 63: formed in 64 bits)
  t.x64 = (uint64_t)tx * kDenoiseTileW + (threadIdx.x & (kDenoiseTileW - 1));
  t.y64 = (uint64_t)ty * kDenoiseTileH + (threadIdx.x / kDenoiseTileW);
  if (t.x64 >= width || t.y64 >= height) return false;
  t.p = (uint32_t)(t.y64 * width + t.x64);
  return true;
}

// Rec.709 luminance
__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// all four channels finite (x - x is NaN for an infinity and for a NaN)
__device__ __forceinline__ bool finite4(float4 c) { return (c.x - c.x == 0.0f) && (c.y - c.y == 0.0f) && (c.z - c.z == 0.0f) && (c.w - c.w == 0.0f); }

// den = max(albedo, 1e-3) per channel: what a colour is divided by in front of a filter and multiplied with behind it; alpha
// goes through as it is
__device__ __forceinline__ float4 denoise_den(float4 a) { return make_float4(fmaxf(a.x, 1e-3f), fmaxf(a.y, 1e-3f), fmaxf(a.z, 1e-3f), 1.0f); }
__device__ __forceinline__ float4 demodulate(float4 c, float4 albedo) {
  const float4 den = denoise_den(albedo);
  return make_float4(c.x / den.x, c.y / den.y, c.z / den.z, c.w);
}
__device__ __forceinline__ float4 remodulate(float4 c, float4 albedo) {
  const float4 den = denoise_den(albedo);
  return make_float4(c.x * den.x, c.y * den.y, c.z * den.z, c.w);
}

// The output stage: gamma and RGBA8 as a render call's last kernel does them -- finalize_pixel with one sample per pixel
// (x / 1.0f is x).  Either output may be nullptr.
__device__ __forceinline__ void write_display_pixel(float4 c, float inv_gamma, uint32_t p, uint8_t* rgba8, float4* rgba32f) {
  FrameParams fp{};
  fp.spp = 1u;
  fp.inv_gamma = inv_gamma;
  finalize_pixel(fp, as_color(c), p, rgba8, rgba32f);
}

// p's own guides, kept in registers over the taps
struct GuideCentre {
  float npx, npy, npz, ppx, ppy, ppz;
  uint32_t idp;
};

template <bool NORMAL, bool POINT, bool ID>
__device__ __forceinline__ GuideCentre guide_centre(const float* normal, const float* point, const uint32_t* id, uint32_t p) {
  GuideCentre g{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
  if (NORMAL) {
    const float* n = normal + 3ull * p;
    g.npx = n[0]; g.npy = n[1]; g.npz = n[2];
  }
  if (POINT) {
    const float* q = point + 3ull * p;
    g.ppx = q[0]; g.ppy = q[1]; g.ppz = q[2];
  }
  if (ID) g.idp = id[p];
  return g;
}

// The normal and the point term of a tap at q, in this order: w * dn with dn = max(n_p . n_q, 0) squared `squarings` times,
// then w / (1 + pd^2 kp) with pd the tap's distance from p's tangent plane.
template <bool NORMAL, bool POINT>
__device__ __forceinline__ float guide_weight(float w, const GuideCentre& g, const float* normal, const float* point, uint32_t q, uint32_t squarings, float kp) {
  if (NORMAL) {
    const float* n = normal + 3ull * q;
    float dn = fmaxf((g.npx * n[0] + g.npy * n[1]) + g.npz * n[2], 0.0f);
    for (uint32_t j = 0; j < squarings; ++j) dn = dn * dn;
    w = w * dn;
  }
  if (POINT) {
    const float* xq = point + 3ull * q;
    const float ex = xq[0] - g.ppx, ey = xq[1] - g.ppy, ez = xq[2] - g.ppz;
    const float pd = (g.npx * ex + g.npy * ey) + g.npz * ez;
    w = w / (1.0f + (pd * pd) * kp);
  }
  return w;
}
