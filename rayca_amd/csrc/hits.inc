// hits.inc -- multi-hit ray queries (rayca_hip_hits_device): for rays in device memory the first k hits along each ray, in
// order, or the number of all of them.  Included from kernels.hip inside the no-packed-f32 region, behind trace_core.inc, whose
// node_step, NodeStack, tri_test / sphere_test, reference_candidate and cull_limit it uses unchanged.  The header's comment on
// RaycaHits is the specification; hits_test is its "hit of a slot", operation by operation.
//
// One ray per lane on the binary f32 nodes with the spill path, as k_query_rays; the leaf rule is new.  A lane keeps the k best
// hits found so far as keys (t, slot), sorted by (t, tie rank), in LDS behind the node stack's rows -- a per-lane array indexed at
// run time would live in scratch -- entry-major like the stack: row r of thread x at list[r * kBlock + x], rows [0, k) the t,
// rows [k, 2k) the slots, so the 64 lanes of a wave hit 64 banks whatever their fill.  (u, v, face) are not kept: when the search
// has ended the same test runs once more on the winners -- the same code on the same operands gives the same bits -- which
// halves the LDS and the words an insertion moves.
//
// The cull (ORDERED) and why it never costs a result (DESIGN 4.17).  b = min(tmax, t of entry k - 1 once the list is full),
// with COUNT_ALL tmax alone; limit = cull_limit(b); a child is entered iff its entry distance is <= limit.
//   * cull_limit's slack is what DESIGN 4.6 proves for closest hits: a slot whose t is <= b has every box above it entered at a
//     distance <= cull_limit(b).  The bound b only falls while a search runs, so a box skipped under an earlier, larger limit
//     stays skipped under every later one.
//   * A hit that belongs into the final list has t <= the final t of entry k - 1 <= every b the search ever used (and t < tmax):
//     none of its boxes is skipped.  That includes a hit that TIES with entry k - 1 on a lower rank -- the test is <=, not < --
//     so the list does not depend on the order of visits.

// the rays, their bounds and the results, all in DEVICE memory
struct HitsIo {
  const float* rays;      // count x 6
  const float* tmax;      // count, or nullptr: tmax_all for every ray
  float tmax_all;
  uint32_t count, k;
  float* t_out;           // count x k; any of the four record outputs may be nullptr
  uint32_t* prim_out;     // count x k
  float* uv_out;          // count x k x 2
  uint8_t* face_out;      // count x k
  uint32_t* n_out;        // count, or nullptr
};

// The hit of one slot, if the ray has one: tri_test as it stands (face 0); BOTH: a triangle that tri_test rejects by its
// back-face line is tested as (v0, v2, v1), whose (u', v') are the weights of v0 and v2 -- reported as (u', (1 - u') - v'),
// the weights of vertex 0 and vertex 1 as every hit record carries them (face 1).  A sphere slot is sphere_test's one hit.
template <bool SPH, bool BOTH>
__device__ __forceinline__ bool hits_test(const DevScene& sc, const TriRecord& tr, const DRay& r, float& t, float& u, float& v, uint32_t& face) {
  face = 0u;
  if (SPH && tr.v0.x != tr.v0.x) {  // sphere slot
    u = v = 0.0f;
    return sphere_test(sc.spheres[__float_as_uint(tr.v0.y)], r, t);
  }
  if (tri_test(tr.v0, tr.v1, tr.v2, r, t, u, v)) return true;
  if (BOTH) {
    const F4 n = cross(tr.v1 - tr.v0, tr.v2 - tr.v0);
    if (dot(r.d, n) > 0.0f) {   // tri_test's first line
      float us, vs;
      if (tri_test(tr.v0, tr.v2, tr.v1, r, t, us, vs)) {
        u = us;
        v = (1.0f - us) - vs;
        face = 1u;
        return true;
      }
    }
  }
  return false;
}

// (t, rank) before the holder of list entry (te, slot e)?  The holder's rank comes from its record, on an exact tie only
__device__ __forceinline__ bool hits_before(const DevScene& sc, float t, uint32_t rank, float te, uint32_t slot_e) {
  return t < te || (t == te && tie_before(sc, rank, slot_e));
}

template <bool ORDERED, bool FAST, bool SPH, bool STATS, bool BOTH, bool COUNT_ALL>
__global__ __launch_bounds__(kBlock, RAYCA_TRACE_MIN_WAVES) void k_hits(DevScene sc, HitsIo q, TraceCounters* counters, TraceLaunch tl) {
  extern __shared__ uint32_t lds_stack[];
  typedef __attribute__((address_space(3))) uint32_t LdsWord;
  typedef __attribute__((address_space(3))) float LdsFloat;
  constexpr bool SLACK = FAST && RAYCA_RAY_SLACK;   // trace()'s kSlackAlways: a caller's origins are anywhere
  NodeStack<true> stack = make_stack<true>(lds_stack, tl, rc_bid() * kBlock + rc_tid());
  uint32_t* const list = lds_stack + tl.lds_entries * kBlock + rc_tid();
  LdsFloat* const lt = (LdsFloat*)list;                   // row e: t of entry e
  LdsWord* const ls = (LdsWord*)list + q.k * kBlock;      // row e: its slot
  const uint32_t i = rc_bid() * rc_bdim() + rc_tid();
  const uint32_t k = q.k;
  LaneCounters cnt{};
  if (i < q.count) {
    const float* rp = q.rays + 6ull * i;
    const DRay ray = make_ray(point3(rp[0], rp[1], rp[2]), vec3(rp[3], rp[4], rp[5]));
    const float tm = q.tmax ? q.tmax[i] : q.tmax_all;
    const float bound = tm < FLT_MAX ? tm : INFINITY;   // a hit counts iff t < bound: false for a NaN and for t = +inf
    const bool finite = fabsf(rp[0]) <= FLT_MAX && fabsf(rp[1]) <= FLT_MAX && fabsf(rp[2]) <= FLT_MAX && fabsf(rp[3]) <= FLT_MAX && fabsf(rp[4]) <= FLT_MAX &&
                        fabsf(rp[5]) <= FLT_MAX;   // (a NaN fails its comparison)
    const bool dead = !(tm > 0.0f) || !finite;   // NaN or <= 0 tmax, a component that is not finite: no hits
    uint32_t n = 0u, total = 0u;                 // entries in the list; counting hits (COUNT_ALL)
    float kth = INFINITY;                        // t of entry k - 1 once the list is full
    if (!dead) {
      const FastRay fr = make_fast(sc, ray, false);
      float limit = INFINITY;
      if (ORDERED && bound < INFINITY) limit = cull_limit<SLACK>(sc, fr, bound);
      float tmin;
      if (STATS) cnt.boxes++;
      uint32_t cur = FAST && RAYCA_NODE_CH ? sc.root_ref_ch : sc.root_ref;   // (may be a leaf)
      if (!slab(sc.root_min[0], sc.root_min[1], sc.root_min[2], sc.root_max[0], sc.root_max[1], sc.root_max[2], ray, tmin)) cur = kTerminated;
      while (cur != kTerminated) {
        while (!(cur & kLeafFlag) && cur != kTerminated) {
          cur = node_step<ORDERED, FAST, false, true, STATS, false, SLACK>(sc, ray, fr, limit, cur, stack, cnt);
        }
        if (cur != kTerminated) {   // a leaf
          const uint32_t first = cur & kLeafFirstMask;
          const uint32_t count = ((cur >> 25) & 63u) + 1u;
          for (uint32_t j = first; j < first + count; ++j) {
            const TriRecord tr = load_tri(sc, j);
            if (STATS) {
              cnt.tris++;
              if (cnt.books()) cnt.slot_tris += 64ull;
            }
            float t, u, v;
            uint32_t face;
            if (!hits_test<SPH, BOTH>(sc, tr, ray, t, u, v, face) || !(t < bound)) continue;
            // a full list takes the hit only in front of its last entry (with k == 0 nothing is kept)
            const bool full = n == k;
            const bool keep = k != 0u && (!full || t < kth || (t == kth && tie_before(sc, tr.rank, ls[(k - 1u) * kBlock])));
            if (!COUNT_ALL && !keep) continue;
            if (!reference_candidate(sc, tr, ray)) continue;
            if (COUNT_ALL) total++;
            if (!keep) continue;
            uint32_t p = full ? k - 1u : n;   // the free entry, or the last one, which drops out
            while (p > 0u) {
              const float te = lt[(p - 1u) * kBlock];
              const uint32_t se = ls[(p - 1u) * kBlock];
              if (!hits_before(sc, t, tr.rank, te, se)) break;
              lt[p * kBlock] = te;
              ls[p * kBlock] = se;
              --p;
            }
            lt[p * kBlock] = t;
            ls[p * kBlock] = j;
            if (!full) ++n;
            if (n == k) {
              kth = lt[(k - 1u) * kBlock];
              if (ORDERED && !COUNT_ALL) {
                const float b = fminf(kth, bound);
                limit = b < INFINITY ? cull_limit<SLACK>(sc, fr, b) : INFINITY;
              }
            }
          }
          cur = stack.pop();
        }
      }
    }
    if (q.n_out) q.n_out[i] = COUNT_ALL ? total : n;
    // the records: the test once more on the winners, the miss record behind them
    for (uint32_t e = 0; e < k; ++e) {
      float t = FLT_MAX, u = 0.0f, v = 0.0f;
      uint32_t slot = RAYCA_NONE, face = 0u;
      if (e < n) {
        slot = ls[e * kBlock];
        const TriRecord tr = load_tri(sc, slot);
        hits_test<SPH, BOTH>(sc, tr, ray, t, u, v, face);
      }
      const size_t at = (size_t)i * k + e;
      if (q.t_out) q.t_out[at] = t;
      if (q.prim_out) q.prim_out[at] = slot;
      if (q.uv_out) {
        q.uv_out[2ull * at] = u;
        q.uv_out[2ull * at + 1ull] = v;
      }
      if (q.face_out) q.face_out[at] = (uint8_t)face;
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
