// signed.inc -- signed distance and occupancy (rayca_hip_signed_device): for points in device memory, or the points of a regular
// grid made in registers, the nearest surface point (k_nearest's search) and a vote of a few crossing-count rays on which side of
// the surface the point lies (k_hits' count_all search with both faces).  Included from kernels.hip inside the no-packed-f32
// region, behind nearest.inc and hits.inc, whose nearest_on_triangle, nearest_box_bound and hits_test it calls unchanged, as it
// does trace_core.inc's node_step, NodeStack, reference_candidate and load_tri.  The header's comment on RaycaSigned is the
// specification.
//
// One point per lane on the binary f32 nodes with the spill path.  Two phases on one node stack, which is empty between them
// (a search ends when pop() hands out kTerminated):
//   A  the nearest search: k_nearest's loop skeleton and cull, operation by operation -- the same candidates in the same
//      comparison, so the same bits whatever the order of visits (nearest.inc has the argument).  Compiled out without a distance
//      output (NEAR).
//   B  the rays: the loop over the directions runs outermost and the directions are kernel arguments, so at any time the whole
//      wave traces ONE direction from neighbouring origins.  Each ray is made in registers, tested against the root box and
//      walked with k_hits' skeleton and leaf rule; two counters stand where k_hits keeps its list.  The bound is +inf: there is
//      no distance cull, CULL only orders the children (and the counts do not depend on the order).  The slack form is the one
//      caller-supplied rays take: a grid's or a caller's points are anywhere.

// the points (or the grid that makes them), their radii, the directions and the results; every pointer is DEVICE memory
struct SignedIo {
  const float* points;    // count x 3; not read with GRID
  const float* radius;    // count, or nullptr: radius_all for every point
  float radius_all;
  uint32_t count;
  float grid_origin[3], grid_step[3];
  uint32_t grid_dims[3];
  uint32_t rule, n_dirs;  // RAYCA_SIGNED_PARITY / _WINDING; 1, 3 or 5
  float dirs[5][3];
  float* dist2_out;       // any of the seven may be nullptr
  uint32_t* prim_out;
  float* point_out;
  float* uv_out;
  uint8_t* inside_out;
  uint8_t* votes_out;
  uint32_t* cross_out;    // count x n_dirs x 2: (front, back)
};

template <bool NEAR, bool CULL, bool GRID, bool FAST, bool STATS>
__global__ __launch_bounds__(kBlock, RAYCA_TRACE_MIN_WAVES) void k_signed(DevScene sc, SignedIo q, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  constexpr bool SLACK = FAST && RAYCA_RAY_SLACK;   // trace()'s kSlackAlways, as k_hits
  NodeStack<true> stack = make_stack<true>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  const uint32_t i = rc_bid() * rc_bdim() + rc_tid();
  LaneCounters cnt{};
  if (i < q.count) {
    float px, py, pz;
    if (GRID) {   // x runs fastest: a wave holds neighbouring points.  Convert, multiply, add, each rounded on its own
      const uint32_t nx = q.grid_dims[0], ny = q.grid_dims[1];
      const uint32_t row = i / nx, ix = i - row * nx, iz = row / ny, iy = row - iz * ny;
      px = q.grid_origin[0] + (float)ix * q.grid_step[0];
      py = q.grid_origin[1] + (float)iy * q.grid_step[1];
      pz = q.grid_origin[2] + (float)iz * q.grid_step[2];
    } else {
      const float* pp = q.points + 3ull * i;
      px = pp[0]; py = pp[1]; pz = pp[2];
    }
    const float pmax = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
    const bool finite = pmax <= FLT_MAX;   // (a NaN fails the comparison)

    // ---- phase A: RAYCA_NEAREST_CLOSEST for (p, radius) ----
    if (NEAR) {
      const float radius = q.radius ? q.radius[i] : q.radius_all;
      const float r2 = radius * radius;
      const bool dead = !(radius > 0.0f) || !finite;
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
                bs = n.s; bt = n.t; bx = n.qx; by = n.qy; bz = n.qz;
              }
            }
            cur = stack.pop();
          }
        }
      }
      const bool found = best_prim != RAYCA_NONE;
      if (q.dist2_out) q.dist2_out[i] = found ? best : FLT_MAX;
      if (q.prim_out) q.prim_out[i] = best_prim;
      if (q.point_out) {
        float* o = q.point_out + 3ull * i;
        o[0] = found ? bx : 0.0f; o[1] = found ? by : 0.0f; o[2] = found ? bz : 0.0f;
      }
      if (q.uv_out) {
        q.uv_out[2ull * i] = found ? (1.0f - bs) - bt : 0.0f;
        q.uv_out[2ull * i + 1ull] = found ? bs : 0.0f;
      }
    }

    // ---- phase B: one crossing-count ray per direction, and the vote ----
    uint32_t votes = 0u;
    for (uint32_t j = 0; j < q.n_dirs; ++j) {
      uint32_t front = 0u, back = 0u;
      if (finite) {
        const DRay ray = make_ray(point3(px, py, pz), vec3(q.dirs[j][0], q.dirs[j][1], q.dirs[j][2]));
        const FastRay fr = make_fast(sc, ray, false);
        float tmin;
        if (STATS) cnt.boxes++;
        uint32_t cur = FAST && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref;   // (may be a leaf)
        if (!slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin)) cur = kTerminated;
        while (cur != kTerminated) {
          while (!(cur & kLeafFlag) && cur != kTerminated) {
            cur = node_step<CULL, FAST, false, true, STATS, false, SLACK>(sc, ray, fr, INFINITY, cur, stack, cnt);
          }
          if (cur != kTerminated) {   // a leaf
            const uint32_t first = cur & kLeafFirstMask;
            const uint32_t count = ((cur >> 25) & 63u) + 1u;
            for (uint32_t s = first; s < first + count; ++s) {
              const TriRecord tr = load_tri(sc, s);
              if (STATS) cnt.tris++;
              float t, u, v;
              uint32_t face;
              if (!hits_test<false, true>(sc, tr, ray, t, u, v, face) || !(t < INFINITY)) continue;
              if (!reference_candidate(sc, tr, ray)) continue;
              front += face ^ 1u;
              back += face;
            }
            cur = stack.pop();
          }
        }
      }
      const bool vote = q.rule == RAYCA_SIGNED_WINDING ? back > front : ((front + back) & 1u) != 0u;
      votes |= (vote ? 1u : 0u) << j;
      if (q.cross_out) {
        uint32_t* o = q.cross_out + ((size_t)i * q.n_dirs + j) * 2u;
        o[0] = front;
        o[1] = back;
      }
    }
    if (q.votes_out) q.votes_out[i] = (uint8_t)votes;
    if (q.inside_out) q.inside_out[i] = 2u * (uint32_t)__popc(votes) > q.n_dirs ? 1 : 0;
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
