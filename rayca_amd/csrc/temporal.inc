// temporal.inc -- the kernel behind rayca_hip_accumulate_device (included from kernels.hip, inside its namespace): temporal
// accumulation of a frame into a history in device memory, with reprojection through the previous camera (DESIGN 4.10).  Image
// space only: nothing of a scene is read.  Every value is built from IEEE +, -, x, /, floor, min and max, one rounding per
// operation in the association the header writes, so that a literal float32 restatement gives the same bits
// (tests/temporal_literal.py).  Every comparison is written so that a NaN fails it; min / max are minNum / maxNum.

// What the pass reads and writes; every pointer is DEVICE memory, the previous camera travels by value.
struct AccumulateIo {
  const float4* color;         // H x W, this frame
  const float* point;          // H x W x 3 } this frame's G-buffer (REPROJECT)
  const float* normal;         // H x W x 3 }
  const uint32_t* id;          // H x W (ID)
  const float4* hist_color;    // H x W, or nullptr: no history at all (identity mode only; REPROJECT implies a history)
  const float* hist_length;    // H x W
  const float* hist_moments;   // H x W x 2 (MOMENTS, with a history); by element: 4-byte aligned like the other guides
  const float* prev_normal;    // H x W x 3 (REPROJECT)
  const float* prev_point;     // H x W x 3 (PLANE)
  const uint32_t* prev_id;     // H x W (ID)
  float4* color_out;
  float* length_out;
  float* moments_out;          // H x W x 2 (MOMENTS)
  float* variance_out;         // (MOMENTS) or nullptr
  uint32_t width, height;      // (width * height <= 2^32 - 1: a pixel's index fits 32 bits, its float offsets are formed in 64)
  uint32_t tiles_x;            // blocks per tile row
  float cap;                   // (float)max_history, 0: unbounded
  float normal_min, plane_max;
  float fw, fh;                // (float)width, (float)height
  float angle, angle_aspect;   // prev_camera.angle, and angle * ((float)width / (float)height)
  float ox, oy, oz;            // prev_camera.origin
  float rx, ry, rz, ux, uy, uz, bx, by, bz;   // right, up, back
};

// The blend: one sample c (finite or not, luminance lum) into a pixel's state -- whether it has a history, and that history's
// colour h, length len and moments (mx, my) -- by the four rows of the header's table.  `cap` is (float)max_history, 0: unbounded.
// k_accumulate applies it once a pixel, k_film_fold (adaptive.inc) once per sample of a pixel's list.
__device__ __forceinline__ void film_blend(bool present, float4 h, float len, float mx, float my, float4 c, bool finite, float lum, float cap,
                                           float4& o, float& n_out, float& m1, float& m2) {
  if (present) {
    if (finite) {
      float n = len + 1.0f;
      if (cap > 0.0f) n = fminf(n, cap);
      const float a = 1.0f / n;
      o = make_float4(h.x + (c.x - h.x) * a, h.y + (c.y - h.y) * a, h.z + (c.z - h.z) * a, h.w + (c.w - h.w) * a);
      n_out = n;
      m1 = mx + (lum - mx) * a;
      m2 = my + (lum * lum - my) * a;
    } else {
      o = h; n_out = len; m1 = mx; m2 = my;
    }
  } else {
    o = c;
    n_out = finite ? 1.0f : 0.0f;
    m1 = finite ? lum : 0.0f;
    m2 = finite ? lum * lum : 0.0f;
  }
}

// One pixel per lane, the denoiser's 64 x 4 tile per block: a wave is 64 consecutive pixels of a row, so that under a small
// camera motion the taps of neighbouring lanes are neighbouring addresses -- a colour tap is a 1-KiB run of 16-B loads.  In
// identity mode the pass is pixel-local: p's history is read before anything of p is written, which is what lets an output be
// the history (or the frame) itself.  A template flag per optional input: an absent one costs nothing.
template <bool REPROJECT, bool ID, bool PLANE, bool MOMENTS>
__global__ __launch_bounds__(kBlock) void k_accumulate(AccumulateIo io) {
  // tile_pixel's lines, written out: through the helper the two bounds tests become one branch and this kernel's SGPR count moves
  const uint32_t tby = blockIdx.x / io.tiles_x, tbx = blockIdx.x - tby * io.tiles_x;
  const uint64_t x64 = (uint64_t)tbx * kDenoiseTileW + (threadIdx.x & (kDenoiseTileW - 1));
  const uint64_t y64 = (uint64_t)tby * kDenoiseTileH + (threadIdx.x / kDenoiseTileW);
  if (x64 >= io.width || y64 >= io.height) return;
  const uint32_t p = (uint32_t)(y64 * io.width + x64);   // (< width * height)
  const float4 c = io.color[p];
  const bool finite = finite4(c);
  const float lum = luminance(c.x, c.y, c.z);

  bool present = false;
  float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float len = 0.0f, mx = 0.0f, my = 0.0f;
  if (!REPROJECT) {
    if (io.hist_color) {
      len = io.hist_length[p];
      if (len > 0.0f) {
        present = true;
        h = io.hist_color[p];
        if (MOMENTS) {
          const float* m = io.hist_moments + 2ull * p;
          mx = m[0]; my = m[1];
        }
      }
    }
  } else {
    const float* n = io.normal + 3ull * p;
    const float npx = n[0], npy = n[1], npz = n[2];
    if (!(npx == 0.0f && npy == 0.0f && npz == 0.0f)) {   // (a miss has a zero normal and no history)
      const float* xp = io.point + 3ull * p;
      const float ppx = xp[0], ppy = xp[1], ppz = xp[2];
      const float vx = ppx - io.ox, vy = ppy - io.oy, vz = ppz - io.oz;
      const float cx = (io.rx * vx + io.ry * vy) + io.rz * vz;
      const float cy = (io.ux * vx + io.uy * vy) + io.uz * vz;
      const float cz = (io.bx * vx + io.by * vy) + io.bz * vz;
      if (cz < 0.0f) {
        const float nz = 0.0f - cz;
        const float fx = ((cx / nz) / io.angle_aspect + 1.0f) * 0.5f * io.fw - 0.5f;
        const float fy = (1.0f - (cy / nz) / io.angle) * 0.5f * io.fh - 0.5f;
        if (fx >= -1.0f && fx < io.fw && fy >= -1.0f && fy < io.fh) {
          const float x0f = floorf(fx), y0f = floorf(fy);
          const float tx = fx - x0f, ty = fy - y0f;
          const int64_t x0 = (int64_t)x0f, y0 = (int64_t)y0f;   // (in [-1, 2^32]: exact)
          uint32_t idp = 0u;
          if (ID) idp = io.id[p];
          float wsum = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sl = 0.0f, smx = 0.0f, smy = 0.0f;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int64_t qy = y0 + j;
            if (qy < 0 || qy >= (int64_t)io.height) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const int64_t qx = x0 + i;
              if (qx < 0 || qx >= (int64_t)io.width) continue;
              const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
              if (!(b > 0.0f)) continue;
              const uint32_t q = (uint32_t)((uint64_t)qy * io.width + (uint64_t)qx);   // (inside the image: < width * height)
              const float lq = io.hist_length[q];
              if (!(lq > 0.0f)) continue;
              if (ID) {
                if (io.prev_id[q] != idp) continue;
              }
              const float* nq = io.prev_normal + 3ull * q;
              if (!((npx * nq[0] + npy * nq[1]) + npz * nq[2] >= io.normal_min)) continue;
              if (PLANE) {
                const float* xq = io.prev_point + 3ull * q;
                const float ex = xq[0] - ppx, ey = xq[1] - ppy, ez = xq[2] - ppz;
                const float pd = (npx * ex + npy * ey) + npz * ez;
                if (!(fabsf(pd) <= io.plane_max)) continue;
              }
              const float4 hq = io.hist_color[q];
              wsum = wsum + b;
              sr = sr + b * hq.x;
              sg = sg + b * hq.y;
              sb = sb + b * hq.z;
              sa = sa + b * hq.w;
              sl = sl + b * lq;
              if (MOMENTS) {
                const float* mq = io.hist_moments + 2ull * q;
                smx = smx + b * mq[0];
                smy = smy + b * mq[1];
              }
            }
          }
          if (wsum > 0.0f) {
            present = true;
            h = make_float4(sr / wsum, sg / wsum, sb / wsum, sa / wsum);
            len = sl / wsum;
            if (MOMENTS) {
              mx = smx / wsum;
              my = smy / wsum;
            }
          }
        }
      }
    }
  }

  float4 o;
  float n_out, m1, m2;
  film_blend(present, h, len, mx, my, c, finite, lum, io.cap, o, n_out, m1, m2);
  io.color_out[p] = o;
  io.length_out[p] = n_out;
  if (MOMENTS) {
    float* m = io.moments_out + 2ull * p;
    m[0] = m1; m[1] = m2;
    if (io.variance_out) io.variance_out[p] = fmaxf(m2 - m1 * m1, 0.0f);
  }
}
