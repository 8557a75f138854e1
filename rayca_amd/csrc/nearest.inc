// nearest.inc -- nearest-point queries (rayca_hip_nearest_device): for points in device memory the nearest surface point of
// the scene's triangles within a radius, or whether there is one.  Included from kernels.hip inside the no-packed-f32 region,
// behind trace_core.inc, whose NodeStack, load_tri and LaneCounters it uses.  The header's comment on RaycaNearest is the
// specification; nearest_on_triangle is that text, operation by operation (no FMA: the unit is built with -ffp-contract=off).
//
// The traversal is its own, not trace()'s: the binary f32 nodes (DevScene::nodes, there under both builders from scene_create
// on), children ordered by point-to-box distance and culled by the best squared distance so far.
//
// The cull and why it never costs a result (DESIGN 4.15 has the derivation).  M = the largest coordinate magnitude of the root
// box and of p, u = 2^-24.
//   * nearest_on_triangle's s and t satisfy 0 <= s, 0 <= t, s + t <= 1 + u in every branch, so its q is a convex combination
//     of the vertices up to rounding: per axis q lies within 13 u M of the triangle's extent, hence of every box that holds
//     the triangle.
//   * Per axis the box gap e = max(lo - p, p - hi, 0) as computed exceeds the computed |p - q| by at most 17 u M.  e' =
//     max(e - 2^-18 M, 0) (64 u M) therefore is at most the computed |p - q| on that axis.
//   * lb' = (e'x e'x + e'y e'y) + e'z e'z and dist2 = (dx dx + dy dy) + dz dz are the same expression, and every operation
//     in it is monotone under round-to-nearest for operands >= 0: lb' <= dist2 of every triangle in the box.  No relative
//     margin is needed on top.
// A child is skipped iff lb' > best, so no skipped triangle has dist2 <= best: neither a nearer one nor a tie on a lower slot.

// the points, their radii and the results, all in DEVICE memory
struct NearestIo {
  const float* points;    // count x 3
  const float* radius;    // count, or nullptr: radius_all for every point
  float radius_all;
  uint32_t count;
  float* dist2_out;       // CLOSEST: any of the four may be nullptr
  uint32_t* prim_out;
  float* point_out;
  float* uv_out;
  uint8_t* within_out;    // WITHIN
};

struct NearestPoint {
  float s, t;             // q = (a + ab*s) + ac*t; in the vertex regions q is the vertex itself
  float qx, qy, qz;
  float dist2;
};

__device__ __forceinline__ float nr_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// Ericson, Real-Time Collision Detection 5.1.5, in the header's order of tests.  A quotient 0 / 0 (a degenerate triangle) or a
// NaN from overflowing products -- it fails every comparison it enters and falls through to the interior branch -- leaves
// dist2 NaN: no candidate.
__device__ __forceinline__ NearestPoint nearest_on_triangle(const TriRecord& tr, float px, float py, float pz) {
  const float ax = tr.v0.x, ay = tr.v0.y, az = tr.v0.z;
  const float abx = tr.v1.x - ax, aby = tr.v1.y - ay, abz = tr.v1.z - az;
  const float acx = tr.v2.x - ax, acy = tr.v2.y - ay, acz = tr.v2.z - az;
  const float apx = px - ax, apy = py - ay, apz = pz - az;
  const float d1 = nr_dot(abx, aby, abz, apx, apy, apz), d2 = nr_dot(acx, acy, acz, apx, apy, apz);
  const float bpx = px - tr.v1.x, bpy = py - tr.v1.y, bpz = pz - tr.v1.z;
  const float d3 = nr_dot(abx, aby, abz, bpx, bpy, bpz), d4 = nr_dot(acx, acy, acz, bpx, bpy, bpz);
  const float cpx = px - tr.v2.x, cpy = py - tr.v2.y, cpz = pz - tr.v2.z;
  const float d5 = nr_dot(abx, aby, abz, cpx, cpy, cpz), d6 = nr_dot(acx, acy, acz, cpx, cpy, cpz);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float d43 = d4 - d3, d56 = d5 - d6;
  NearestPoint n;
  int vertex = -1;
  if (d1 <= 0.0f && d2 <= 0.0f) {                            // vertex a
    n.s = 0.0f; n.t = 0.0f; vertex = 0;
  } else if (d3 >= 0.0f && d4 <= d3) {                       // vertex b
    n.s = 1.0f; n.t = 0.0f; vertex = 1;
  } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {       // edge ab
    n.s = d1 / (d1 - d3); n.t = 0.0f;
  } else if (d6 >= 0.0f && d5 <= d6) {                       // vertex c
    n.s = 0.0f; n.t = 1.0f; vertex = 2;
  } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {       // edge ac
    n.s = 0.0f; n.t = d2 / (d2 - d6);
  } else if (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) {     // edge bc
    n.t = d43 / (d43 + d56); n.s = 1.0f - n.t;
  } else {                                                   // interior; the selects keep (s, t) in the triangle when rounding has
    const float den = (va + vb) + vc;                        // left va, vb, vc with mixed signs (a far point, a needle)
    float s = vb / den, t = vc / den;
    s = s < 0.0f ? 0.0f : s;
    s = s > 1.0f ? 1.0f : s;
    const float room = 1.0f - s;
    t = t < 0.0f ? 0.0f : t;
    t = t > room ? room : t;
    n.s = s; n.t = t;
  }
  n.qx = (ax + abx * n.s) + acx * n.t;
  n.qy = (ay + aby * n.s) + acy * n.t;
  n.qz = (az + abz * n.s) + acz * n.t;
  // (selects of scalars: a select between the three vertices as objects puts the record into scratch)
  n.qx = vertex == 0 ? ax : (vertex == 1 ? tr.v1.x : (vertex == 2 ? tr.v2.x : n.qx));
  n.qy = vertex == 0 ? ay : (vertex == 1 ? tr.v1.y : (vertex == 2 ? tr.v2.y : n.qy));
  n.qz = vertex == 0 ? az : (vertex == 1 ? tr.v1.z : (vertex == 2 ? tr.v2.z : n.qz));
  const float dx = px - n.qx, dy = py - n.qy, dz = pz - n.qz;
  n.dist2 = nr_dot(dx, dy, dz, dx, dy, dz);
  return n;
}

// the cull's lower bound of dist2 over a box: see the head of the file
__device__ __forceinline__ float nearest_box_bound(float lox, float loy, float loz, float hix, float hiy, float hiz, float px, float py, float pz, float slack) {
  const float ex = fmaxf(fmaxf(fmaxf(lox - px, px - hix), 0.0f) - slack, 0.0f);
  const float ey = fmaxf(fmaxf(fmaxf(loy - py, py - hiy), 0.0f) - slack, 0.0f);
  const float ez = fmaxf(fmaxf(fmaxf(loz - pz, pz - hiz), 0.0f) - slack, 0.0f);
  return (ex * ex + ey * ey) + ez * ez;
}

// One point per lane.  WITHIN: one byte, the search ends at the first candidate that counts.  CULL: ordered and culled; without
// it every node and every triangle is visited (RAYCA_TRAVERSAL_EXHAUSTIVE), children left first.  The result does not depend on
// the order of visits: among the candidates with dist2 < r2 the smallest dist2 wins, the lowest slot on equal dist2.
template <bool WITHIN, bool CULL, bool SPILL, bool STATS>
__global__ __launch_bounds__(kBlock) void k_nearest(DevScene sc, NearestIo q, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  NodeStack<SPILL> stack = make_stack<SPILL>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t i = rc_bid() * rc_bdim() + rc_tid();
  LaneCounters cnt{};
  if (i < q.count) {
    const float* pp = q.points + 3ull * i;
    const float px = pp[0], py = pp[1], pz = pp[2];
    const float radius = q.radius ? q.radius[i] : q.radius_all;
    const float r2 = radius * radius;
    const float pmax = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
    const bool dead = !(radius > 0.0f) || !(pmax <= FLT_MAX);   // NaN or <= 0 radius, a non-finite coordinate: a miss
    float best = r2;
    uint32_t best_prim = RAYCA_NONE;
    float bs = 0.0f, bt = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    if (!dead) {
      float m = pmax;
      for (int k = 0; k < 3; ++k) m = fmaxf(m, fmaxf(fabsf(sc.root_min[k]), fabsf(sc.root_max[k])));
      const float slack = m * 3.814697265625e-06f;   // 2^-18 M
      uint32_t cur = sc.root_ref;   // (may be a leaf)
      if (CULL) {
        if (STATS) cnt.boxes++;
        if (!(nearest_box_bound(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], px, py, pz, slack) <= best)) cur = kTerminated;
      }
      while (cur != kTerminated) {
        while (!(cur & kLeafFlag) && cur != kTerminated) {
          const float4* np = sc.nodes + 4ull * cur;
          const float4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
          const uint32_t lref = __float_as_uint(q3.x), rref = __float_as_uint(q3.y);
          if (STATS) cnt.boxes += 2;
          // (a model without primitives leaves kNoChild behind a box far away: never entered, whatever the radius)
          bool hl = lref != kNoChild, hr = rref != kNoChild, left_first = true;
          if (CULL) {
            const float ll = nearest_box_bound(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, px, py, pz, slack);
            const float lr = nearest_box_bound(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, px, py, pz, slack);
            hl = hl && ll <= best;
            hr = hr && lr <= best;
            left_first = ll <= lr;
          }
          if (hl && hr) {
            stack.push(left_first ? rref : lref);
            cur = left_first ? lref : rref;
          } else if (hl) {
            cur = lref;
          } else if (hr) {
            cur = rref;
          } else {
            cur = stack.pop();
          }
        }
        if (cur != kTerminated) {   // a leaf
          const uint32_t first = cur & kLeafFirstMask;
          const uint32_t count = ((cur >> 25) & 63u) + 1u;
          for (uint32_t j = first; j < first + count; ++j) {
            const TriRecord tr = load_tri(sc, j);
            if (STATS) cnt.tris++;
            const NearestPoint n = nearest_on_triangle(tr, px, py, pz);
            if (n.dist2 < best || (n.dist2 == best && best_prim != RAYCA_NONE && j < best_prim)) {
              best = n.dist2;
              best_prim = j;
              if (!WITHIN) {
                bs = n.s; bt = n.t; bx = n.qx; by = n.qy; bz = n.qz;
              }
            }
          }
          cur = (WITHIN && best_prim != RAYCA_NONE) ? kTerminated : stack.pop();
        }
      }
    }
    const bool found = best_prim != RAYCA_NONE;
    if (WITHIN) {
      q.within_out[i] = found ? 1 : 0;
    } else {
      if (q.dist2_out) q.dist2_out[i] = found ? best : FLT_MAX;
      if (q.prim_out) q.prim_out[i] = best_prim;
      if (q.point_out) {
        float* o = q.point_out + 3ull * i;
        o[0] = found ? bx : 0.0f; o[1] = found ? by : 0.0f; o[2] = found ? bz : 0.0f;
      }
      if (q.uv_out) {   // (weight of vertex 0, weight of vertex 1): what shade_hit reads of a hit record
        q.uv_out[2ull * i] = found ? (1.0f - bs) - bt : 0.0f;
        q.uv_out[2ull * i + 1ull] = found ? bs : 0.0f;
      }
    }
  }
  if (STATS) {
    unsigned long long b = cnt.boxes, t = cnt.tris;
    for (int off = 32; off > 0; off >>= 1) {
      b += __shfl_down(b, off);
      t += __shfl_down(t, off);
    }
    if (__lane_id() == 0) {
      atomicAdd(&counters->boxes, b);
      atomicAdd(&counters->tris, t);
    }
  }
}
