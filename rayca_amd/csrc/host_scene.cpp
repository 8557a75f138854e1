// host_scene.cpp -- scene-graph flattening and the reference-equivalent BVH build.
//
// What the reference does at the top of every draw (rayca-soft/src/scene.rs:90-99):
//   SceneDrawInfo::new      scene.rs:190-282        world transforms + draw-info lists
//   BvhScene::from_scene    bvh/primitive.rs:194-395 one BvhModel (primitive list) per model
//   Tlas::new               bvh/tlas.rs:248-269     one BLAS per model (SAH, bvh/blas.rs:229-316)
//                                                   + median-split TLAS (bvh/tlas.rs:74-134)
// The tree produced here has exactly the reference's topology and primitive order (so depth ties
// resolve identically); only the evaluation strategy differs: the 63 x 3 SAH candidates of
// find_best_split_plane (blas.rs:93-123) are priced from one binned sweep per axis instead of 189
// passes over the primitives, and disjoint subtrees are built on separate host threads.
#include "host_scene.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <cmath>
#include <thread>

#include <sched.h>
#include <sys/mman.h>
#include <unordered_map>

namespace rayca {

// ---- the pool behind DefaultInitAllocator (host_scene.hpp) ------------------------------------------------------------------
namespace {
struct BigBlockPool {
  std::mutex mu;
  std::unordered_map<void*, size_t> capacity;            // every live block of the pool, handed out or cached
  std::vector<std::pair<size_t, void*>> cached;          // (capacity, block) not handed out
  size_t cached_bytes = 0;
  size_t limit = [] {
    const char* e = getenv("RAYCA_HOST_POOL_MB");
    return (size_t)(e ? std::max(atoi(e), 0) : 1024) << 20;
  }();
  ~BigBlockPool() {
    for (auto& c : cached) std::free(c.second);
  }
};
BigBlockPool& big_pool() {
  static BigBlockPool* p = new BigBlockPool();   // (never destroyed: vectors of static lifetime may give blocks back at exit)
  return *p;
}
}  // namespace
void* big_block_take(size_t bytes) {
  BigBlockPool& bp = big_pool();
  constexpr size_t kAlign = size_t(2) << 20;
  const size_t want = (bytes + kAlign - 1) / kAlign * kAlign;
  {
    std::lock_guard<std::mutex> lock(bp.mu);
    size_t best = bp.cached.size();
    for (size_t i = 0; i < bp.cached.size(); ++i)   // the smallest cached block that fits and is not wastefully large
      if (bp.cached[i].first >= want && bp.cached[i].first <= 2 * want + (size_t(8) << 20) && (best == bp.cached.size() || bp.cached[i].first < bp.cached[best].first)) best = i;
    if (best != bp.cached.size()) {
      void* p = bp.cached[best].second;
      bp.cached_bytes -= bp.cached[best].first;
      bp.cached.erase(bp.cached.begin() + (long)best);
      return p;
    }
  }
  void* p = std::aligned_alloc(kAlign, want);
  if (!p) throw std::bad_alloc();
  (void)madvise(p, want, MADV_HUGEPAGE);   // (where the system allows it: 512 times fewer faults on first touch)
  std::lock_guard<std::mutex> lock(bp.mu);
  bp.capacity[p] = want;
  return p;
}
void big_block_give(void* p) noexcept {
  if (!p) return;
  BigBlockPool& bp = big_pool();
  bool release = false;
  {
    std::lock_guard<std::mutex> lock(bp.mu);
    auto it = bp.capacity.find(p);
    if (it == bp.capacity.end()) return;   // (not ours: cannot happen)
    if (bp.cached_bytes + it->second <= bp.limit && bp.cached.size() < 64) {
      bp.cached.emplace_back(it->second, p);
      bp.cached_bytes += it->second;
    } else {
      bp.capacity.erase(it);
      release = true;
    }
  }
  if (release) std::free(p);
}

unsigned host_threads() {
  static const unsigned n = [] {
    if (const char* e = getenv("RAYCA_HOST_THREADS")) return std::max(1u, (unsigned)atoi(e));
    unsigned avail = std::thread::hardware_concurrency();
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) avail = (unsigned)CPU_COUNT(&set);
    return std::max(1u, std::min(avail, 16u));
  }();
  return n;
}

namespace {

// worker(t) for t in [0, threads): threads - 1 of them on threads started here, worker(0) on the caller; all joined
template <class Fn>
void run_on_host_threads(unsigned threads, Fn worker) {
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; ++t) pool.emplace_back([&worker, t] { worker(t); });
  worker(0u);
  for (std::thread& th : pool) th.join();
}

// fn(begin, end) over [0, n) on all host threads
template <class Fn>
void parallel_chunks(size_t n, Fn fn) {
  const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(host_threads(), n / 4096 + 1));
  const size_t per = (n + nt - 1) / nt;
  run_on_host_threads(nt, [&](unsigned t) { fn(std::min(n, t * per), std::min(n, (t + 1) * per)); });
}

inline Box empty_box() { return Box{point3(FLT_MAX, FLT_MAX, FLT_MAX), point3(-FLT_MAX, -FLT_MAX, -FLT_MAX)}; }
inline Box origin_box() { return Box{point3(0, 0, 0), point3(0, 0, 0)}; }  // AABB::default()  aabb.rs:9-13
inline void grow(Box& bx, F4 p) {
  bx.a = vmin(bx.a, p);
  bx.b = vmax(bx.b, p);
}
inline float area(const Box& bx) {  // aabb.rs:20-23
  const F4 e = as_vec(bx.b - bx.a);
  return e.x * e.y + e.y * e.z + e.z * e.x;
}
inline float axis_of(F4 v, int axis) { return axis == 0 ? v.x : (axis == 1 ? v.y : v.z); }

inline Trs trs_from_abi(const RaycaTrs& t) {
  return Trs{vec3(t.translation[0], t.translation[1], t.translation[2]), f4(t.rotation[0], t.rotation[1], t.rotation[2], t.rotation[3]),
             vec3(t.scale[0], t.scale[1], t.scale[2])};
}

float sphere_world_radius(const HostPrim& p, const Trs& t) {  // sphere.rs:90-92
  return p.radius * fmaxf(fmaxf(t.scale.x, t.scale.y), fmaxf(t.scale.z, t.scale.w));
}

// grow a box by a primitive the way AABB::grow_primitive does (aabb.rs:62-72)
void grow_primitive(Box& bx, const HostPrim& p, const Trs& t) {
  if (p.kind == RAYCA_GEOMETRY_TRIANGLE_MESH) {
    grow(bx, p.wp[0]);
    grow(bx, p.wp[1]);
    grow(bx, p.wp[2]);
  } else {
    const float r = sphere_world_radius(p, t);
    const F4 c = trs_apply_point(t, p.center);
    grow(bx, c + vec3(-r, 0, 0));
    grow(bx, c + vec3(r, 0, 0));
    grow(bx, c + vec3(0, -r, 0));
    grow(bx, c + vec3(0, r, 0));
    grow(bx, c + vec3(0, 0, -r));
    grow(bx, c + vec3(0, 0, r));
  }
}

void cache_world(HostPrim& p, const Trs& t) {
  if (p.kind == RAYCA_GEOMETRY_TRIANGLE_MESH) {
    for (int i = 0; i < 3; ++i) p.wp[i] = trs_apply_point(t, p.p[i]);  // Triangle::get_vertex  triangle.rs:67-69
    p.wcentroid = to_point(trs_apply_vec(t, p.centroid));              // primitive.rs:71-77 -> triangle.rs:161-163
    F4 mn = point3(FLT_MAX, FLT_MAX, FLT_MAX), mx = point3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
    for (int i = 0; i < 3; ++i) {
      mn = vmin(mn, p.wp[i]);
      mx = vmax(mx, p.wp[i]);
    }
    p.wmin = mn;
    p.wmax = mx;
  } else {
    const float r = sphere_world_radius(p, t);
    const F4 c = trs_apply_point(t, p.center);
    p.wcentroid = c;
    p.wmin = c - vec3(r, r, r);  // sphere.rs:170-178
    p.wmax = c + vec3(r, r, r);
    p.wp[0] = p.wp[1] = p.wp[2] = point3(0, 0, 0);
  }
}

// ---- BLAS build --------------------------------------------------------------------------------
thread_local BlasBuildFn g_device_builder = nullptr;  // per thread: scenes may be created concurrently on different devices
thread_local uint32_t g_device_ordinal = 0;
// below this many primitives the host builder is faster than a level-by-level sequence of launches
constexpr uint32_t kDeviceBuildMin = 4096;

struct BlasBuilder {
  const HostScene* scene;
  std::vector<uint32_t>* order;  // indices into scene->prims, partitioned in place
  uint32_t max_depth;
  unsigned parallel_levels;
  bool seed_origin;  // true: the reference's AABB::default() seed (blas.rs:66-67); false: empty boxes

  const HostPrim& prim(uint32_t slot) const { return scene->prims[(*order)[slot]]; }

  Box range_bounds(uint32_t offset, uint32_t count) const {  // BvhNode::new  blas.rs:27-36
    Box bx = empty_box();
    for (uint32_t i = offset; i < offset + count; ++i) {
      bx.a = vmin(bx.a, prim(i).wmin);
      bx.b = vmax(bx.b, prim(i).wmax);
    }
    return bx;
  }

  // find_best_split_plane (blas.rs:93-123) + evaluate_sah (blas.rs:64-89), exact binned form.
  // A primitive is left of plane i iff centroid < pos_i; pos_i is non-decreasing in i, so it is left
  // of exactly the planes i > k with k = #{i : pos_i <= centroid}.  Unions of min/max are exact, so
  // each of the 63 (count, box) pairs -- and therefore each cost -- equals the literal evaluation.
  void best_split(const BuildNode& node, int& best_axis, float& split_pos, float& best_cost) const {
    best_cost = FLT_MAX;
    best_axis = 0;
    split_pos = 0.0f;
    for (int axis = 0; axis < 3; ++axis) {
      const float bmin = axis_of(node.bounds.a, axis), bmax = axis_of(node.bounds.b, axis);
      if (bmin == bmax) continue;
      const float scale = (bmax - bmin) / 64.0f;
      float pos[64];
      pos[0] = -FLT_MAX;
      for (int i = 1; i < 64; ++i) pos[i] = bmin + (float)i * scale;
      Box bins[64];
      uint32_t cnt[64];
      for (int b = 0; b < 64; ++b) {
        bins[b] = empty_box();
        cnt[b] = 0;
      }
      for (uint32_t s = node.offset; s < node.offset + node.count; ++s) {
        const HostPrim& p = prim(s);
        const float c = axis_of(p.wcentroid, axis);
        int k;
        if (c != c) {
          k = 63;  // NaN: never `<` any plane
        } else {
          // k = number of planes j in 1..63 with pos[j] <= c  (upper bound in a monotone array)
          int lo = 1, hi = 64;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pos[mid] <= c) lo = mid + 1;
            else hi = mid;
          }
          k = lo - 1;
        }
        cnt[k]++;
        grow_primitive(bins[k], p, scene->world_trs[p.node]);
      }
      Box lbox[65], rbox[65];
      uint32_t lcnt[65], rcnt[65];
      lbox[0] = seed_origin ? origin_box() : empty_box();
      lcnt[0] = 0;
      for (int b = 0; b < 64; ++b) {
        lbox[b + 1] = lbox[b];
        lcnt[b + 1] = lcnt[b] + cnt[b];
        if (cnt[b]) {
          lbox[b + 1].a = vmin(lbox[b + 1].a, bins[b].a);
          lbox[b + 1].b = vmax(lbox[b + 1].b, bins[b].b);
        }
      }
      rbox[64] = seed_origin ? origin_box() : empty_box();
      rcnt[64] = 0;
      for (int b = 63; b >= 0; --b) {
        rbox[b] = rbox[b + 1];
        rcnt[b] = rcnt[b + 1] + cnt[b];
        if (cnt[b]) {
          rbox[b].a = vmin(rbox[b].a, bins[b].a);
          rbox[b].b = vmax(rbox[b].b, bins[b].b);
        }
      }
      for (int i = 1; i < 64; ++i) {
        float cost;
        if (seed_origin) {
          cost = (float)lcnt[i] * area(lbox[i]) + (float)rcnt[i] * area(rbox[i]);
        } else {
          if (lcnt[i] == 0 || rcnt[i] == 0) continue;  // not a split
          cost = (float)lcnt[i] * area(lbox[i]) + (float)rcnt[i] * area(rbox[i]);
        }
        if (!(cost > 0.0f)) cost = FLT_MAX;
        if (cost < best_cost) {
          best_cost = cost;
          best_axis = axis;
          split_pos = pos[i];
        }
      }
    }
  }

  // Blas::set_primitives_recursive  blas.rs:261-316.  Builds the subtree below arena[idx]; new
  // nodes go to `arena` (thread-local when running as a task).
  void split(std::vector<BuildNode>& arena, int32_t idx, uint32_t level) const {
    if (level >= max_depth) return;
    BuildNode node = arena[idx];
    int axis;
    float pos, cost;
    best_split(node, axis, pos, cost);
    const float no_split_cost = (float)node.count * area(node.bounds);
    if (cost > no_split_cost) return;
    uint32_t i = node.offset, j = node.offset + node.count;
    std::vector<uint32_t>& ord = *order;
    while (i < j) {  // partition-in-place, exactly the reference's swap sequence (blas.rs:279-289)
      if (axis_of(scene->prims[ord[i]].wcentroid, axis) < pos) {
        ++i;
      } else {
        std::swap(ord[i], ord[j - 1]);
        --j;
      }
    }
    const uint32_t left_count = i - node.offset, right_count = node.count - left_count;
    if (left_count == 0 || right_count == 0) return;
    BuildNode l, r;
    l.offset = node.offset;
    l.count = left_count;
    l.bounds = range_bounds(l.offset, l.count);
    r.offset = node.offset + left_count;
    r.count = right_count;
    r.bounds = range_bounds(r.offset, r.count);
    if (level < parallel_levels && node.count > 8192) {
      // children in private arenas, spliced afterwards; ranges are disjoint so partitioning is safe
      std::vector<BuildNode> la{l}, ra{r};
      auto fut = std::async(std::launch::async, [&] { split(la, 0, level + 1); });
      split(ra, 0, level + 1);
      fut.get();
      const int32_t lbase = (int32_t)arena.size();
      for (auto n : la) {
        if (n.left >= 0) {
          n.left += lbase;
          n.right += lbase;
        }
        arena.push_back(n);
      }
      const int32_t rbase = (int32_t)arena.size();
      for (auto n : ra) {
        if (n.left >= 0) {
          n.left += rbase;
          n.right += rbase;
        }
        arena.push_back(n);
      }
      arena[idx].left = lbase;
      arena[idx].right = rbase;
    } else {
      const int32_t li = (int32_t)arena.size();
      arena.push_back(l);
      const int32_t ri = (int32_t)arena.size();
      arena.push_back(r);
      arena[idx].left = li;
      arena[idx].right = ri;
      split(arena, li, level + 1);
      split(arena, ri, level + 1);
    }
    arena[idx].count = 0;  // inner
  }
};

// ---- TLAS build  bvh/tlas.rs:74-134 --------------------------------------------------------------
struct TNode {
  Box bounds;
  int32_t left = -1, right = -1;
  uint32_t offset = 0, count = 0;
};

void tlas_split(std::vector<TNode>& tn, int32_t self, std::vector<uint32_t>& blas_order, const std::vector<Box>& blas_root,
                uint32_t offset, uint32_t count) {
  TNode n;
  n.offset = offset;
  n.count = count;
  n.bounds = empty_box();
  for (uint32_t i = offset; i < offset + count; ++i) {
    n.bounds.a = vmin(n.bounds.a, blas_root[blas_order[i]].a);
    n.bounds.b = vmax(n.bounds.b, blas_root[blas_order[i]].b);
  }
  const F4 extent = as_vec(n.bounds.b - n.bounds.a);
  int axis = 0;
  if (extent.y > extent.x) axis = 1;
  if (extent.z > axis_of(extent, axis)) axis = 2;
  const float split_pos = axis_of(n.bounds.a, axis) + axis_of(extent, axis) * 0.5f;
  uint32_t i = offset, j = offset + count;
  while (i < j) {
    const Box& rb = blas_root[blas_order[i]];
    const F4 centroid = to_point(as_vec(rb.b - rb.a) / 2.0f);  // AABB::get_centroid: the half-extent (aabb.rs:95-97)
    if (axis_of(centroid, axis) < split_pos) {
      ++i;
    } else {
      std::swap(blas_order[i], blas_order[j - 1]);
      --j;
    }
  }
  const uint32_t left_count = i - offset, right_count = count - left_count;
  tn[self] = n;
  if (left_count > 0 && right_count > 0) {
    const int32_t l = (int32_t)tn.size();
    tn.emplace_back();
    tlas_split(tn, l, blas_order, blas_root, offset, left_count);
    const int32_t r = (int32_t)tn.size();
    tn.emplace_back();
    tlas_split(tn, r, blas_order, blas_root, offset + left_count, right_count);
    tn[self].left = l;
    tn[self].right = r;
    tn[self].count = 0;
  }
}

// double -> IEEE half, rounded toward -inf (up == false) or +inf (up == true); NaN for NaN.  The arithmetic statement of
// the rounding; the encoder uses the bit form below, the self-test holds the two against each other.
uint16_t to_half_directed_ref(double v, bool up) {
  if (v != v) return 0x7E00u;
  const bool neg = std::signbit(v);
  double a = std::fabs(v);
  const bool mag_up = neg ? !up : up;  // direction on the magnitude
  const uint16_t sign = neg ? 0x8000u : 0u;
  if (a == 0.0) return sign;
  if (a > 65504.0) return (uint16_t)(sign | (mag_up ? 0x7C00u : 0x7BFFu));
  int e;
  (void)std::frexp(a, &e);  // a = m * 2^e, m in [0.5, 1)
  e -= 1;                    // a = m' * 2^e, m' in [1, 2)
  if (e < -14) {             // subnormal halves: multiples of 2^-24
    const double q = a * 16777216.0;
    double r = mag_up ? std::ceil(q) : std::floor(q);
    if (r >= 1024.0) return (uint16_t)(sign | 0x0400u);
    return (uint16_t)(sign | (uint16_t)r);
  }
  const double unit = std::ldexp(1.0, e - 10);
  double q = a / unit;  // in [1024, 2048)
  double r = mag_up ? std::ceil(q) : std::floor(q);
  if (r >= 2048.0) {
    r = 1024.0;
    e += 1;
    if (e > 15) return (uint16_t)(sign | 0x7C00u);
  }
  return (uint16_t)(sign | ((uint16_t)(e + 15) << 10) | ((uint16_t)r - 1024u));
}

// The same on the bits of the double: a value in the normal range of a half keeps its top ten mantissa bits, and moves one
// unit away from zero when anything was cut off and the direction asks for it (the carry runs into the exponent, and out
// of the largest one into infinity, as it should).  Everything else -- zero, subnormal halves, overflow, inf, NaN -- takes
// the arithmetic form.  (A scene build converts twelve of these per node, twice over.)
inline uint16_t to_half_directed(double v, bool up) {
  uint64_t bits;
  std::memcpy(&bits, &v, sizeof bits);
  const uint64_t mag = bits & 0x7FFFFFFFFFFFFFFFull;
  const int e = (int)(mag >> 52) - 1023;
  if (e < -14 || e > 15) return to_half_directed_ref(v, up);
  const bool neg = (bits >> 63) != 0;
  const uint64_t man = mag & 0x000FFFFFFFFFFFFFull;
  uint32_t h = ((uint32_t)(e + 15) << 10) | (uint32_t)(man >> 42);
  if ((neg ? !up : up) && (man & 0x3FFFFFFFFFFull)) ++h;
  return (uint16_t)((neg ? 0x8000u : 0u) | h);
}

// ---- device layout -------------------------------------------------------------------------------

struct DevBuilder {
  HostScene& s;
  std::vector<uint32_t> blas_base;  // first global primitive slot of each BLAS (TLAS order)
  float pad_rel = 0.0f, pad_abs = 0.0f;  // RAYCA_BUILDER_SAH: conservative boxes (see build_host_scene)
  // subtrees laid out as one leaf (host_scene.hpp kLeafNodeCost): the same decisions, by the same arithmetic, as the
  // device layout makes for a tree it holds (bvh_build.hip k_layout_sizes)
  float node_cost = 0.0f;
  uint32_t leaf_max = kLeafCollapseMax;
  std::vector<uint32_t> plan_prims;   // per arena node of the BLAS being laid out: primitives below it
  std::vector<uint8_t> plan_leafed;   // 1: the subtree is one leaf, 2: inside such a subtree
  // false: a child that is not behind its parent in the arena (both builders append them that way; every pass relies on it)
  bool plan_leaves(const HostBlas& bl) {
    const std::vector<BuildNode>& a = bl.nodes;
    const size_t n = a.size();
    plan_prims.assign(n, 0u);
    plan_leafed.assign(n, 0);
    std::vector<float> cost(n, 0.0f);
    for (size_t i = n; i-- > 0;) {  // children sit behind their parents
      const BuildNode& bn = a[i];
      if (bn.left < 0) {
        plan_prims[i] = bn.count;
        cost[i] = (float)bn.count * area(bn.bounds);
        continue;
      }
      if ((size_t)bn.left <= i || (size_t)bn.right <= i || (size_t)bn.left >= n || (size_t)bn.right >= n) return false;
      const uint32_t pl = plan_prims[bn.left], pr = plan_prims[bn.right];
      const float ar = area(bn.bounds), as_leaf = (float)(pl + pr) * ar, as_split = node_cost * ar + cost[bn.left] + cost[bn.right];
      const bool one_leaf = node_cost > 0.0f && pl + pr <= leaf_max && as_leaf <= as_split;
      plan_leafed[i] = one_leaf ? 1 : 0;
      cost[i] = one_leaf ? as_leaf : as_split;
      plan_prims[i] = pl + pr;
    }
    for (size_t i = 0; i < n; ++i) {  // everything below a one-leaf subtree is not laid out at all
      const BuildNode& bn = a[i];
      if (bn.left < 0 || plan_leafed[i] == 0) continue;
      plan_leafed[bn.left] = plan_leafed[bn.right] = 2;
    }
    return true;
  }

  void put_box(DevNode& n, int side, const Box& b0) {
    Box b = b0;
    if (!(b0.a.x <= b0.b.x)) {  // the inverted box of an empty BLAS: make it unhittable
      b.a = point3(kNowhere, kNowhere, kNowhere);
      b.b = b.a;
    }
    if (pad_rel > 0.0f && b0.a.x <= b0.b.x) {  // (the nowhere box stays a point: padding would make it enterable)
      const float* lo[3] = {&b0.a.x, &b0.a.y, &b0.a.z};
      const float* hi[3] = {&b0.b.x, &b0.b.y, &b0.b.z};
      float* plo[3] = {&b.a.x, &b.a.y, &b.a.z};
      float* phi[3] = {&b.b.x, &b.b.y, &b.b.z};
      for (int k = 0; k < 3; ++k) {
        const float m = fmaxf(fmaxf(fabsf(*lo[k]), fabsf(*hi[k])), *hi[k] - *lo[k]);
        const float pad = m * pad_rel + pad_abs;
        *plo[k] = *lo[k] - pad;
        *phi[k] = *hi[k] + pad;
      }
    }
    put_box_raw(n, side, b);
  }
  static void put_box_raw(DevNode& n, int side, const Box& b) {
    if (side == 0) {
      n.q[0] = b.a.x; n.q[1] = b.a.y; n.q[2] = b.a.z; n.q[3] = b.b.x; n.q[4] = b.b.y; n.q[5] = b.b.z;
    } else {
      n.q[6] = b.a.x; n.q[7] = b.a.y; n.q[8] = b.a.z; n.q[9] = b.b.x; n.q[10] = b.b.y; n.q[11] = b.b.z;
    }
  }
  static uint32_t leaf_ref(uint32_t first, uint32_t count) { return kLeafFlag | ((count - 1u) << 25) | first; }

  uint32_t new_node() {
    s.dev_nodes.emplace_back();
    std::memset(&s.dev_nodes.back(), 0, sizeof(DevNode));
    return (uint32_t)s.dev_nodes.size() - 1;
  }
  // Every emit_* returns the packed child reference and reports, through `need`, how many stack entries a traversal of that
  // subtree can have pending at once: an inner node pushes one child and descends into the other, so need = 1 +
  // max(need(left), need(right)) -- except for the chain nodes below, whose two boxes are identical so the left (leaf) child
  // is always taken first and the pushed entry is popped before the rest of the chain is entered.
  std::string error;  // set by emit_blas for a tree it cannot lay out (an internal error: the caller hands it on)
  // A leaf range of more than 64 primitives: ceil(count / 64) - 1 consecutive nodes from `cur` on that re-test the same box,
  // 64 primitives to the left of each (a loop: chains can be thousands of nodes long with the reference's coarse leaves)
  void write_leaf_chain(uint32_t cur, uint32_t first, uint32_t count, const Box& box) {
    for (;; ++cur) {
      DevNode& d = s.dev_nodes[cur];
      std::memset(&d, 0, sizeof d);
      put_box(d, 0, box);
      put_box(d, 1, box);
      d.left = leaf_ref(first, kLeafMaxPrims);
      first += kLeafMaxPrims;
      count -= kLeafMaxPrims;
      if (count <= kLeafMaxPrims) {
        d.right = leaf_ref(first, count);
        return;
      }
      d.right = cur + 1u;
    }
  }
  // A host-held BLAS below its root, without recursion.  Children sit behind their parents in the arena (plan_leaves has
  // checked it), so one backward pass gives every subtree's device-node count and stack need, one forward pass gives every
  // node its index -- pre-order: a node, its left subtree, its right subtree -- and then every node is written independently,
  // by all host threads.  (A recursive walk over an arena in level order was 36 ms of cache misses for the atrium's 543 k nodes.)
  uint32_t emit_blas_flat(const HostBlas& bl, uint32_t base, uint32_t& need) {
    const std::vector<BuildNode>& a = bl.nodes;
    const size_t n = a.size();
    std::vector<uint32_t> size(n), stack_need(n);
    for (size_t i = n; i-- > 0;) {
      const BuildNode& bn = a[i];
      if (bn.left < 0) {  // leaf: nothing (its parent holds a packed reference), or a chain of ceil(count / 64) - 1 nodes
        const uint32_t chain = bn.count > kLeafMaxPrims ? (bn.count + kLeafMaxPrims - 1) / kLeafMaxPrims - 1 : 0u;
        size[i] = chain;
        stack_need[i] = chain ? 1u : 0u;
      } else {
        const bool one_leaf = plan_leafed[i] != 0;   // (its parent holds a leaf reference, it takes no nodes)
        size[i] = one_leaf ? 0u : 1u + size[bn.left] + size[bn.right];
        stack_need[i] = one_leaf ? 0u : 1u + std::max(stack_need[bn.left], stack_need[bn.right]);
      }
    }
    const uint32_t first = (uint32_t)s.dev_nodes.size();
    std::vector<uint32_t> index(n);  // device index of an inner node / of the head of a leaf's chain
    index[0] = first;
    for (size_t i = 0; i < n; ++i) {
      const BuildNode& bn = a[i];
      if (bn.left < 0) continue;
      index[bn.left] = index[i] + 1u;
      index[bn.right] = index[i] + 1u + size[bn.left];
    }
    s.dev_nodes.resize((size_t)first + size[0]);
    auto ref_of = [&](size_t i) -> uint32_t {  // what the parent stores for child i
      const BuildNode& bn = a[i];
      if (bn.left >= 0) return plan_leafed[i] == 1 ? leaf_ref(base + bn.offset, plan_prims[i]) : index[i];
      if (bn.count == 0) return kNoChild;  // a model without primitives: nothing to visit
      return bn.count <= kLeafMaxPrims ? leaf_ref(base + bn.offset, bn.count) : index[i];
    };
    parallel_chunks(n, [&](size_t b, size_t e) {
      for (size_t i = b; i < e; ++i) {
        const BuildNode& bn = a[i];
        if (plan_leafed[i] != 0) continue;  // the root of, or inside, a subtree that is one leaf
        if (bn.left >= 0) {
          DevNode& d = s.dev_nodes[index[i]];
          std::memset(&d, 0, sizeof d);
          put_box(d, 0, a[bn.left].bounds);
          put_box(d, 1, a[bn.right].bounds);
          d.left = ref_of((size_t)bn.left);
          d.right = ref_of((size_t)bn.right);
        } else if (bn.count > kLeafMaxPrims) {
          write_leaf_chain(index[i], base + bn.offset, bn.count, bn.bounds);
        }
      }
    });
    need = stack_need[0];
    return ref_of(0);
  }
  // One BLAS of the scene, its primitives from global slot `base` on
  uint32_t emit_blas(const HostBlas& bl, uint32_t base, uint32_t& need) {
    if (bl.dev_tree) {  // built and kept on the device: a run of node indices is set aside, the device fills it
      const uint32_t first = (uint32_t)s.dev_nodes.size();
      s.dev_nodes.resize((size_t)first + bl.dev_node_count);
      s.dev_segments.push_back(DeviceSegment{first, bl.dev_node_count, base, bl.dev_tree});
      need = bl.dev_need;
      return first;   // (more than 64 primitives: the root is an inner node or the head of a chain, node 0 of the run)
    }
    if (!plan_leaves(bl)) {
      error = "internal error: a BLAS arena holds a child that is not behind its parent";
      need = 0;
      return kNoChild;
    }
    return emit_blas_flat(bl, base, need);
  }
  // TLAS leaf holding blas [offset, offset+count): BLAS roots tested one after the other
  uint32_t emit_blas_chain(uint32_t offset, uint32_t count, const Box& leaf_box, uint32_t& need) {
    if (count == 1) return emit_blas(s.blas[offset], blas_base[offset], need);
    const uint32_t n = new_node();
    put_box(s.dev_nodes[n], 0, s.blas[offset].nodes[0].bounds);
    put_box(s.dev_nodes[n], 1, leaf_box);
    uint32_t nl = 0, nr = 0;
    const uint32_t lr = emit_blas(s.blas[offset], blas_base[offset], nl);
    s.dev_nodes[n].left = lr;
    const uint32_t rr = emit_blas_chain(offset + 1, count - 1, leaf_box, nr);
    s.dev_nodes[n].right = rr;
    need = 1 + std::max(nl, nr);
    return n;
  }
  uint32_t emit_tlas(const std::vector<TNode>& tn, int32_t idx, uint32_t& need) {
    const TNode& t = tn[idx];
    if (t.left < 0) return emit_blas_chain(t.offset, t.count, t.bounds, need);
    const uint32_t n = new_node();
    put_box(s.dev_nodes[n], 0, tn[t.left].bounds);
    put_box(s.dev_nodes[n], 1, tn[t.right].bounds);
    uint32_t nl = 0, nr = 0;
    const uint32_t lr = emit_tlas(tn, t.left, nl);
    s.dev_nodes[n].left = lr;
    const uint32_t rr = emit_tlas(tn, t.right, nr);
    s.dev_nodes[n].right = rr;
    need = 1 + std::max(nl, nr);
    return n;
  }
};

// ---- 4-wide collapse ---------------------------------------------------------------------------
// Each wide node adopts the grandchildren of a binary node (largest box first) until it has four
// children.  Skipping a binary node skips its box test, which cannot change what the traversal finds:
// a child's box is contained in its parent's and the slab arithmetic is monotone in the box corners,
// so whenever a child box passes the test every box above it passes too.
struct WideBuilder {
  HostScene& s;
  struct Kid {
    uint32_t ref;
    float b[6];  // min xyz, max xyz
  };
  static float kid_area(const Kid& k) {
    const float ex = k.b[3] - k.b[0], ey = k.b[4] - k.b[1], ez = k.b[5] - k.b[2];
    return ex * ey + ey * ez + ez * ex;
  }
  void kids_of(uint32_t bin, Kid out[2]) const {
    const DevNode& n = s.dev_nodes[bin];
    out[0].ref = n.left;
    out[1].ref = n.right;
    for (int i = 0; i < 6; ++i) {
      out[0].b[i] = n.q[i];
      out[1].b[i] = n.q[6 + i];
    }
  }
  // the up-to-four children a wide node gets for binary node `bin_ref`
  int expand(uint32_t bin_ref, Kid kids[4]) const {
    int k = 2;
    kids_of(bin_ref, kids);
    while (k < 4) {
      int best = -1;
      float best_area = -1.0f;
      for (int i = 0; i < k; ++i) {
        if ((kids[i].ref & kLeafFlag) || kids[i].ref == kNoChild) continue;
        const float a = kid_area(kids[i]);
        if (best < 0 || a > best_area) {
          best = i;
          best_area = a;
        }
      }
      if (best < 0) break;
      Kid two[2];
      kids_of(kids[best].ref, two);
      // keep the left-to-right order of the binary tree (exhaustive mode visits children in index order)
      for (int i = k; i > best + 1; --i) kids[i] = kids[i - 1];
      kids[best] = two[0];
      kids[best + 1] = two[1];
      ++k;
    }
    return k;
  }

  // Subtrees a few levels down are collapsed by all host threads into arrays of their own (numbered from 0, pre-order)
  // and spliced in when the top of the tree -- built by this thread, in the same pre-order -- reaches them: the result is
  // the array the purely sequential recursion produces, node for node.
  struct Task {
    uint32_t bin_root = 0, need = 0;
    std::vector<DevNode4> nodes;
  };
  std::vector<Task> tasks;
  std::vector<std::pair<uint32_t, uint32_t>> task_of;  // (binary ref, task), sorted by ref
  bool allow_parallel = true;  // (the self-test switches it off to compare against the sequential recursion)

  void collect(uint32_t bin_ref, int depth) {
    if ((bin_ref & kLeafFlag) || bin_ref == kNoChild) return;
    if (depth == 0) {
      tasks.emplace_back();
      tasks.back().bin_root = bin_ref;
      return;
    }
    Kid kids[4];
    const int k = expand(bin_ref, kids);
    for (int i = 0; i < k; ++i) collect(kids[i].ref, depth - 1);
  }

  uint32_t build(uint32_t bin_ref, uint32_t& need) {
    tasks.clear();
    task_of.clear();
    if (allow_parallel && s.dev_nodes.size() >= 65536 && host_threads() > 1) {
      collect(bin_ref, 3);
      std::atomic<size_t> next{0};
      run_on_host_threads((unsigned)std::min<size_t>(host_threads(), tasks.size()), [&](unsigned) {
        for (size_t t; (t = next.fetch_add(1)) < tasks.size();) build_into(tasks[t].nodes, tasks[t].bin_root, tasks[t].need, false);
      });
      for (size_t t = 0; t < tasks.size(); ++t) task_of.push_back({tasks[t].bin_root, (uint32_t)t});
      std::sort(task_of.begin(), task_of.end());
    }
    return build_into(s.dev_nodes4, bin_ref, need, true);
  }

  uint32_t build_into(std::vector<DevNode4>& out, uint32_t bin_ref, uint32_t& need, bool top) {
    if ((bin_ref & kLeafFlag) || bin_ref == kNoChild) {
      need = 0;
      return bin_ref;
    }
    if (top && !task_of.empty()) {
      const auto it = std::lower_bound(task_of.begin(), task_of.end(), std::make_pair(bin_ref, 0u));
      if (it != task_of.end() && it->first == bin_ref) {  // splice the finished subtree: local indices + base
        Task& t = tasks[it->second];
        const uint32_t base = (uint32_t)out.size();
        out.insert(out.end(), t.nodes.begin(), t.nodes.end());
        for (size_t i = base; i < out.size(); ++i)
          for (int c = 0; c < 4; ++c)
            if (!(out[i].child[c] & kLeafFlag) && out[i].child[c] != kNoChild) out[i].child[c] += base;
        std::vector<DevNode4>().swap(t.nodes);
        need = t.need;
        return base;  // a task's root is its node 0
      }
    }
    // iterative over an explicit work list would be needed for pathological depth only; the binary
    // chains for big leaves are collapsed 3 links at a time here
    Kid kids[4];
    const int k = expand(bin_ref, kids);
    const uint32_t idx = (uint32_t)out.size();
    out.emplace_back();
    uint32_t child_refs[4], child_need[4] = {0, 0, 0, 0};
    uint32_t worst = 0;
    for (int i = 0; i < k; ++i) {
      uint32_t nd = 0;
      child_refs[i] = build_into(out, kids[i].ref, nd, top);
      child_need[i] = nd;
      worst = std::max(worst, nd);
    }
    DevNode4& w = out[idx];
    for (int i = 0; i < 4; ++i) {
      if (i < k) {
        for (int a = 0; a < 3; ++a) {
          w.lo[a][i] = kids[i].b[a];
          w.hi[a][i] = kids[i].b[3 + a];
        }
        w.child[i] = child_refs[i];
      } else {
        // Unused slot: a zero-size box far away.  (An inverted +-FLT_MAX box does NOT work: (MAX - o) * rd
        // overflows to +-inf for |rd| > 1 and the slab test then passes.)  A point box passes only if the
        // three axis distances are equal, and any overflow makes them unordered, so it is never entered.
        for (int a = 0; a < 3; ++a) {
          w.lo[a][i] = kNowhere;
          w.hi[a][i] = kNowhere;
        }
        w.child[i] = kNoChild;
      }
      w.pad[i] = 0;
    }
    // pending entries: the nearest child is entered with k-1 siblings on the stack.  If all boxes are
    // identical (the chains that split big leaves) the children are taken in index order, so child i
    // is entered with k-1-i siblings pending.
    bool same = true;
    for (int i = 1; i < k && same; ++i) same = std::memcmp(kids[i].b, kids[0].b, sizeof kids[0].b) == 0;
    if (same) {
      need = 0;
      for (int i = 0; i < k; ++i) need = std::max(need, (uint32_t)(k - 1 - i) + child_need[i]);
    } else {
      need = (uint32_t)(k - 1) + worst;
    }
    return idx;
  }
};

bool fetch_index(const RaycaSceneDesc& d, const RaycaPrimitive& p, uint32_t i, uint32_t& out) {
  const uint64_t off = p.index_byte_offset;
  switch (p.index_type) {
    case RAYCA_INDEX_U8:
      if (off + i >= d.index_byte_count) return false;
      out = d.index_bytes[off + i];
      return true;
    case RAYCA_INDEX_U16: {
      if (off + 2ull * i + 2 > d.index_byte_count) return false;
      uint16_t v;
      std::memcpy(&v, d.index_bytes + off + 2ull * i, 2);
      out = v;
      return true;
    }
    case RAYCA_INDEX_U32: {
      if (off + 4ull * i + 4 > d.index_byte_count) return false;
      std::memcpy(&out, d.index_bytes + off + 4ull * i, 4);
      return true;
    }
    default:
      return false;  // panic!("Index type not supported")  primitive.rs:258
  }
}

void set_ext(PrimExt& e, int k, Color c, F4 n, F4 t, F4 b, F2 uv) {
  e.color[k][0] = c.r; e.color[k][1] = c.g; e.color[k][2] = c.b; e.color[k][3] = c.a;
  e.normal[k][0] = n.x; e.normal[k][1] = n.y; e.normal[k][2] = n.z;
  e.tangent[k][0] = t.x; e.tangent[k][1] = t.y; e.tangent[k][2] = t.z;
  e.bitangent[k][0] = b.x; e.bitangent[k][1] = b.y; e.bitangent[k][2] = b.z;
  e.uv[k][0] = uv.x; e.uv[k][1] = uv.y;
}

}  // namespace

// Self-check of the two layout passes against their recursive forms on a random tree (uneven depths, mostly small leaves
// and some of 65..264 primitives so that the 64-primitive chains occur): the arrays must be identical, byte for byte.
int32_t selftest_device_layouts(std::string& err) {
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&rng]() {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return rng;
  };
  auto rnd = [&](float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) & 0xFFFFFF) / 16777216.0f; };
  HostBlas bl;
  const uint32_t prims = 1u << 20;
  bl.prims.resize(prims);
  for (uint32_t i = 0; i < prims; ++i) bl.prims[i] = i;
  bl.nodes.emplace_back();
  bl.nodes[0].offset = 0;
  bl.nodes[0].count = prims;
  bl.nodes[0].bounds = Box{point3(-1, -1, -1), point3(1, 1, 1)};
  for (size_t i = 0; i < bl.nodes.size(); ++i) {  // breadth-first: children behind their parent, like the builders
    const BuildNode n = bl.nodes[i];
    const uint32_t leaf_max = (next() % 16u == 0u) ? 65u + (uint32_t)(next() % 200u) : 1u + (uint32_t)(next() % 8u);
    if (n.count <= leaf_max) continue;
    const uint32_t cut = 1u + (uint32_t)(next() % (n.count - 1u));
    BuildNode l, r;
    l.offset = n.offset; l.count = cut;
    r.offset = n.offset + cut; r.count = n.count - cut;
    for (BuildNode* c : {&l, &r}) {
      const float x0 = rnd(-1, 1), y0 = rnd(-1, 1), z0 = rnd(-1, 1);
      c->bounds = Box{point3(x0, y0, z0), point3(x0 + rnd(0, 0.5f), y0 + rnd(0, 0.5f), z0 + rnd(0, 0.5f))};
    }
    bl.nodes[i].left = (int32_t)bl.nodes.size();
    bl.nodes.push_back(l);
    bl.nodes[i].right = (int32_t)bl.nodes.size();
    bl.nodes.push_back(r);
    bl.nodes[i].count = 0;
  }
  // The literal statement of the binary layout, which the flat pass (DevBuilder::emit_blas) is held against: a node, then
  // its left subtree, then its right one; a subtree the plan folds is one leaf reference; a leaf of more than 64 primitives
  // is a chain of nodes that re-test its box, 64 primitives to the left of each.
  struct Literal {
    DevBuilder& db;
    const HostBlas& bl;
    uint32_t leaf(uint32_t first, uint32_t count, const Box& box, uint32_t& need) {
      need = count > kLeafMaxPrims ? 1 : 0;   // (a chain's pushed right child is popped before the rest of the chain is entered)
      if (count <= kLeafMaxPrims) return count ? DevBuilder::leaf_ref(first, count) : kNoChild;
      const uint32_t n = db.new_node();
      db.put_box(db.s.dev_nodes[n], 0, box);
      db.put_box(db.s.dev_nodes[n], 1, box);
      db.s.dev_nodes[n].left = DevBuilder::leaf_ref(first, kLeafMaxPrims);
      uint32_t rest_need = 0;
      const uint32_t rest = leaf(first + kLeafMaxPrims, count - kLeafMaxPrims, box, rest_need);
      db.s.dev_nodes[n].right = rest;
      return n;
    }
    uint32_t node(uint32_t idx, uint32_t& need) {
      const BuildNode& bn = bl.nodes[idx];
      if (bn.left < 0) return leaf(bn.offset, bn.count, bn.bounds, need);
      if (db.plan_leafed[idx] == 1) {
        need = 0;
        return DevBuilder::leaf_ref(bn.offset, db.plan_prims[idx]);
      }
      const uint32_t n = db.new_node();
      db.put_box(db.s.dev_nodes[n], 0, bl.nodes[bn.left].bounds);
      db.put_box(db.s.dev_nodes[n], 1, bl.nodes[bn.right].bounds);
      uint32_t nl = 0, nr = 0;
      const uint32_t lr = node((uint32_t)bn.left, nl);
      db.s.dev_nodes[n].left = lr;
      const uint32_t rr = node((uint32_t)bn.right, nr);
      db.s.dev_nodes[n].right = rr;
      need = 1 + std::max(nl, nr);
      return n;
    }
  };
  for (const float node_cost : {0.0f, kLeafNodeCost}) {   // the tree as built, and with subtrees laid out as single leaves
    HostScene a, b;
    uint32_t ref[2], need[2], ref4[2], need4[2];
    HostScene* scenes[2] = {&a, &b};
    for (int pass = 0; pass < 2; ++pass) {
      HostScene& s = *scenes[pass];
      s.blas.push_back(bl);
      DevBuilder db{s, {0u}};
      db.node_cost = node_cost;
      db.pad_rel = 1.52587890625e-05f;
      db.pad_abs = 1e-6f;
      if (pass == 1) {
        ref[pass] = db.emit_blas(s.blas[0], 0, need[pass]);
      } else {
        if (!db.plan_leaves(s.blas[0])) { err = "layout self-test: the random tree has a child in front of its parent"; return RAYCA_ERR_BAD_ARG; }
        ref[pass] = Literal{db, s.blas[0]}.node(0, need[pass]);
      }
      if (!db.error.empty()) { err = "layout self-test: " + db.error; return RAYCA_ERR_BAD_ARG; }
      WideBuilder wb{s};
      wb.allow_parallel = pass == 1;
      ref4[pass] = wb.build(ref[pass], need4[pass]);
    }
    if (node_cost == 0.0f && a.dev_nodes.size() < 65536) { err = "layout self-test: the random tree came out too small to exercise the parallel passes"; return RAYCA_ERR_BAD_ARG; }
    auto same = [](const auto& x, const auto& y) { return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(*x.data())) == 0; };
    const char* differs = nullptr;
    if (ref[0] != ref[1] || need[0] != need[1] || !same(a.dev_nodes, b.dev_nodes)) differs = "layout self-test: the flat binary-node pass differs from the recursive one";
    else if (ref4[0] != ref4[1] || need4[0] != need4[1] || !same(a.dev_nodes4, b.dev_nodes4)) differs = "layout self-test: the parallel 4-wide collapse differs from the sequential one";
    if (differs) { err = differs; return RAYCA_ERR_BAD_ARG; }
  }
  return RAYCA_OK;
}

// Self-check of the outward fp16 rounding the steering boxes rely on: every finite half maps to itself in both
// directions, and for values between two neighbouring halves `down` and `up` return exactly those neighbours.
int32_t selftest_half_rounding(std::string& err) {
  auto decode = [](uint16_t h) -> double {
    const int e = (h >> 10) & 31, m = h & 1023;
    const double v = e == 0 ? std::ldexp((double)m, -24) : std::ldexp(1024.0 + m, e - 25);
    return (h & 0x8000u) ? -v : v;
  };
  auto fail = [&](const char* what, double v) {
    char buf[128];
    snprintf(buf, sizeof buf, "half rounding: %s at %.17g", what, v);
    err = buf;
    return (int32_t)RAYCA_ERR_BAD_ARG;
  };
  for (uint32_t h = 0; h < 65536u; ++h) {
    if (((h >> 10) & 31u) == 31u) continue;  // inf / NaN
    const double v = decode((uint16_t)h);
    if (decode(to_half_directed(v, false)) != v || decode(to_half_directed(v, true)) != v) return fail("exact value moved", v);
    // the next half above (same sign ordering on the real line)
    const uint16_t up_bits = (h & 0x8000u) ? (uint16_t)((h & 0x7FFFu) == 0 ? 0x0001u : h - 1u) : (uint16_t)(h + 1u);
    if (((up_bits >> 10) & 31u) == 31u) continue;
    const double w = decode(up_bits);
    if (!(w > v)) continue;  // -0 / +0
    for (const double f : {0.25, 0.5, 0.999}) {
      const double x = v + (w - v) * f;
      const double lo = decode(to_half_directed(x, false)), hi = decode(to_half_directed(x, true));
      if (lo != v || hi != w) return fail("bracket is not the two neighbours", x);
    }
  }
  // the bit form against the arithmetic form: every binade a half can hold and the ones either side, both signs, values
  // on, just above and just below a half's grid
  uint64_t lcg = 0x9E3779B97F4A7C15ull;
  for (int e = -30; e <= 20; ++e)
    for (int i = 0; i < 4096; ++i) {
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      uint64_t man = lcg >> 12;
      if (i % 4 == 1) man &= ~0x3FFFFFFFFFFull;                   // exactly representable
      if (i % 4 == 2) man = (man & ~0x3FFFFFFFFFFull) | 1ull;      // one ulp of the double above
      if (i % 4 == 3) man |= 0x3FFFFFFFFFFull;                     // just below the next
      const uint64_t bits = ((uint64_t)((i >> 2) & 1) << 63) | ((uint64_t)(e + 1023) << 52) | man;
      double x;
      std::memcpy(&x, &bits, sizeof x);
      for (const bool up : {false, true})
        if (to_half_directed(x, up) != to_half_directed_ref(x, up)) return fail("bit form differs from the arithmetic form", x);
    }
  if (to_half_directed(1e6, true) != 0x7C00u || to_half_directed(1e6, false) != 0x7BFFu) return fail("overflow", 1e6);
  if (to_half_directed(-1e6, false) != 0xFC00u || to_half_directed(-1e6, true) != 0xFBFFu) return fail("overflow", -1e6);
  if (to_half_directed(1e-9, true) != 0x0001u || to_half_directed(1e-9, false) != 0x0000u) return fail("underflow", 1e-9);
  return RAYCA_OK;
}

void set_device_blas_builder(BlasBuildFn fn, uint32_t device) {
  g_device_builder = fn;
  g_device_ordinal = device;
}

// The three node formats next to the binary f32 one (RAYCA_BUILDER_SAH scenes): the same tree collapsed to 4-wide nodes, and
// both with fp16 steering boxes.  Reads `s.dev_nodes`, writes `dev_nodes4`, `dev_nodes_h`, `dev_nodes4_h` and their scalars; the
// library runs it on a thread of its own while the first frames are already traversing the binary nodes.
void finish_node_formats(HostScene& s, const std::atomic<bool>* cancel) {
  if (!s.other_formats_wanted) return;
  auto cancelled = [cancel] { return cancel && cancel->load(std::memory_order_relaxed); };
  if (cancelled()) return;
  Lap lap;
  // the 4-wide collapse reads the binary nodes and writes its own array: it runs next to the fp16 encoding of the binary
  // nodes below and is joined before its own fp16 copy is made
  std::thread wide_thread([&s] {
    WideBuilder wb{s};
    uint32_t need4 = 0;
    s.root_ref4 = wb.build(s.root_ref, need4);
    s.max_depth4 = need4;
  });
  struct Joiner {
    std::thread& t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } wide_joiner{wide_thread};
  // fp16 steering boxes: centre of the scene box, power-of-two scale that maps the half extent to <= 2^14
  float half_extent = 0.0f;
  const float lo3[3] = {s.root_min.x, s.root_min.y, s.root_min.z}, hi3[3] = {s.root_max.x, s.root_max.y, s.root_max.z};
  for (int c = 0; c < 3; ++c) {
    s.half_center[c] = 0.5f * (lo3[c] + hi3[c]);
    if (!(s.half_center[c] == s.half_center[c]) || std::fabs(s.half_center[c]) > 1e30f) s.half_center[c] = 0.0f;
    half_extent = std::max(half_extent, std::max(std::fabs(hi3[c] - s.half_center[c]), std::fabs(lo3[c] - s.half_center[c])));
  }
  int k = 0;
  if (half_extent > 0.0f && half_extent < 1e30f) {
    (void)std::frexp(half_extent * 1.0009765625f, &k);  // half_extent (+ padding) < 2^k
    k = 14 - k;
  }
  k = std::max(-100, std::min(100, k));
  s.half_scale = std::ldexp(1.0f, k);
  auto cv = [&](float x, int axis, bool up) -> uint16_t {
    // only NaNs are unenterable here; the "nowhere" slots are recognised box by box below.  Finite coordinates beyond
    // the fp16 range saturate OUTWARD (to_half_directed: max -> +inf, min -> -inf), so the box stays conservative
    // and the frame cannot depend on the node format chosen, whatever the scene's extent.
    if (!(x == x)) return 0x7E00u;
    return to_half_directed(((double)x - (double)s.half_center[axis]) * (double)s.half_scale, up);
  };
  s.dev_nodes_h.resize(s.dev_nodes.size());
  parallel_chunks(s.dev_nodes.size(), [&](size_t b, size_t e) {
    for (size_t i = b; i < e; ++i) {
      const DevNode& n = s.dev_nodes[i];
      DevNodeH& h = s.dev_nodes_h[i];
      // q: l.min xyz, l.max xyz, r.min xyz, r.max xyz
      for (int j = 0; j < 12; ++j) h.h[j] = cv(n.q[j], j % 3, (j / 3) & 1);
      // an inverted (empty) box and the zero-size "nowhere" box of an unused slot must stay unenterable after
      // outward rounding
      for (int side = 0; side < 2; ++side) {
        bool nowhere = true;
        for (int j = 0; j < 6; ++j) nowhere = nowhere && n.q[side * 6 + j] == kNowhere;
        if (nowhere || !(n.q[side * 6] <= n.q[side * 6 + 3]))
          for (int j = 0; j < 6; ++j) h.h[side * 6 + j] = 0x7E00u;
      }
      h.left = n.left;
      h.right = n.right;
    }
  });
  lap("  binary nodes, fp16");
  wide_thread.join();
  lap("  4-wide nodes (rest)");
  if (cancelled()) return;
  s.dev_nodes4_h.resize(s.dev_nodes4.size());
  parallel_chunks(s.dev_nodes4.size(), [&](size_t b, size_t e) {
    for (size_t i = b; i < e; ++i) {
      const DevNode4& n = s.dev_nodes4[i];
      DevNode4H& h = s.dev_nodes4_h[i];
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 4; ++c) {
          bool empty = !(n.lo[0][c] <= n.hi[0][c]);
          if (n.lo[0][c] == kNowhere && n.hi[0][c] == kNowhere && n.lo[1][c] == kNowhere && n.hi[1][c] == kNowhere && n.lo[2][c] == kNowhere &&
              n.hi[2][c] == kNowhere)
            empty = true;  // unused slot (WideBuilder)
          h.lo[a][c] = empty ? 0x7E00u : cv(n.lo[a][c], a, false);
          h.hi[a][c] = empty ? 0x7E00u : cv(n.hi[a][c], a, true);
        }
      for (int c = 0; c < 4; ++c) h.child[c] = n.child[c];
    }
  });
  lap("  4-wide nodes, fp16");
}

int32_t scene_graph_pass(const RaycaSceneDesc& d, SceneGraph& s, std::string& err) {
  if (d.node_count && !d.nodes) { err = "nodes is null"; return RAYCA_ERR_BAD_ARG; }
  const uint32_t N = d.node_count;

  // ---- SceneDrawInfo::new: world(i) = world(parent) * local(i)  (scene.rs:213-215,228,242) ----
  s.local_trs.resize(N);
  s.world_trs.resize(N);
  std::vector<std::vector<uint32_t>> children(N);
  std::vector<uint32_t> tops;
  for (uint32_t i = 0; i < N; ++i) {
    const RaycaNode& n = d.nodes[i];
    if (n.parent >= (int32_t)i) { err = "node " + std::to_string(i) + ": parent must precede child"; return RAYCA_ERR_BAD_ARG; }
    s.local_trs[i] = trs_from_abi(n.trs);
    if (n.parent < 0) {
      s.world_trs[i] = s.local_trs[i];
      tops.push_back(i);
    } else {
      s.world_trs[i] = trs_compose(s.world_trs[n.parent], s.local_trs[i]);
      children[n.parent].push_back(i);
    }
  }
  // traversal order = DFS pre-order (children ascending)
  std::vector<uint32_t> order;
  order.reserve(N);
  {
    std::vector<uint32_t> stack(tops.rbegin(), tops.rend());
    while (!stack.empty()) {
      const uint32_t n = stack.back();
      stack.pop_back();
      order.push_back(n);
      for (auto it = children[n].rbegin(); it != children[n].rend(); ++it) stack.push_back(*it);
    }
  }
  for (uint32_t n : order) {
    const RaycaNode& nd = d.nodes[n];
    if (nd.mesh != RAYCA_NONE) {
      if (nd.mesh >= d.mesh_count) { err = "mesh index out of range"; return RAYCA_ERR_BAD_ARG; }
      s.mesh_nodes.push_back(n);
    }
    if (nd.light != RAYCA_NONE) {
      if (nd.light >= d.light_count) { err = "light index out of range"; return RAYCA_ERR_BAD_ARG; }
      s.light_nodes.push_back(n);
    }
    if (nd.camera != RAYCA_NONE && !s.has_camera) {
      if (nd.camera >= d.camera_count) { err = "camera index out of range"; return RAYCA_ERR_BAD_ARG; }
      s.has_camera = true;
      s.camera_node = n;
      s.camera_yfov = d.cameras[nd.camera].yfov_radians;
    }
  }
  for (uint32_t n : s.light_nodes) {
    const RaycaLight& l = d.lights[d.nodes[n].light];
    HostLight hl;
    hl.kind = l.kind;
    hl.node = n;
    hl.material = l.material;
    hl.intensity = l.intensity;
    hl.color = rgba(l.color[0], l.color[1], l.color[2], l.color[3]);
    hl.attenuation = vec3(l.attenuation[0], l.attenuation[1], l.attenuation[2]);
    hl.ab = vec3(l.ab[0], l.ab[1], l.ab[2]);
    hl.ac = vec3(l.ac[0], l.ac[1], l.ac[2]);
    hl.local = s.local_trs[n];
    s.lights.push_back(hl);
  }
  return RAYCA_OK;
}

int32_t update_moves_geometry(const RaycaSceneDesc& d, const SceneGraph& g, const std::vector<Trs>& world_was,
                              const std::vector<HostLight>& lights_was, std::string& err) {
  auto same = [](const auto& a, const auto& b) { return std::memcmp(&a, &b, sizeof a) == 0; };
  const std::string rebuild = ": that moves geometry, which needs rayca_hip_scene_create";
  for (const uint32_t n : g.mesh_nodes)
    if (!same(g.world_trs[n], world_was[n])) {
      err = "node " + std::to_string(n) + " carries a mesh and its world transform changed" + rebuild;
      return RAYCA_ERR_UNSUPPORTED;
    }
  for (size_t i = 0; i < g.lights.size(); ++i) {
    const HostLight &a = g.lights[i], &b = lights_was[i];
    const std::string which = "light " + std::to_string(d.nodes[a.node].light) + " (node " + std::to_string(a.node) + ")";
    if ((a.kind == RAYCA_LIGHT_QUAD) != (b.kind == RAYCA_LIGHT_QUAD)) {
      err = which + " changes its kind to or from a quad light" + rebuild;
      return RAYCA_ERR_UNSUPPORTED;
    }
    if (a.kind != RAYCA_LIGHT_QUAD) continue;
    if (!same(a.local, b.local) || !same(g.world_trs[a.node], world_was[a.node])) {
      err = which + " is a quad light and its transform changed" + rebuild;
      return RAYCA_ERR_UNSUPPORTED;
    }
    if (!same(a.ab, b.ab) || !same(a.ac, b.ac) || a.material != b.material) {
      err = which + " is a quad light and its ab, ac or material changed" + rebuild;
      return RAYCA_ERR_UNSUPPORTED;
    }
  }
  return RAYCA_OK;
}

int32_t desc_validate(const RaycaSceneDesc& d, std::string& err) {
  if (d.abi_version != RAYCA_ABI_VERSION) { err = "abi version mismatch"; return RAYCA_ERR_BAD_ARG; }
  const std::pair<const char*, bool> tables[] = {
      {"nodes", d.node_count && !d.nodes},           {"meshes", d.mesh_count && !d.meshes},
      {"primitives", d.primitive_count && !d.primitives}, {"positions", d.vertex_count && !d.positions},
      {"index_bytes", d.index_byte_count && !d.index_bytes}, {"materials", d.material_count && !d.materials},
      {"textures", d.texture_count && !d.textures},  {"images", d.image_count && !d.images},
      {"image_bytes", d.image_byte_count && !d.image_bytes}, {"cameras", d.camera_count && !d.cameras},
      {"lights", d.light_count && !d.lights}};
  for (const auto& t : tables)
    if (t.second) { err = std::string(t.first) + " is null"; return RAYCA_ERR_BAD_ARG; }
  for (uint32_t i = 0; i < d.material_count; ++i) {
    const RaycaMaterial& m = d.materials[i];
    for (const uint32_t t : {m.albedo_texture, m.normal_texture, m.metallic_roughness_texture})
      if (t != RAYCA_NONE && t >= d.texture_count) { err = "material " + std::to_string(i) + ": texture index out of range"; return RAYCA_ERR_BAD_ARG; }
  }
  // every image, referenced by a texture or not: a known texel format, all texels inside image_bytes, floats on a word.
  // width x height fits 64 bits, width x height x 16 need not: the texel count is compared with the bytes left divided by the texel size.
  for (uint32_t i = 0; i < d.image_count; ++i) {
    const RaycaImage& im = d.images[i];
    const std::string which = "image " + std::to_string(i);
    if (im.color_type != RAYCA_COLOR_RGB8 && im.color_type != RAYCA_COLOR_RGBA8 && im.color_type != RAYCA_COLOR_RGBA32F) {
      err = which + ": color_type " + std::to_string(im.color_type) + " is none of RGB8, RGBA8, RGBA32F";
      return RAYCA_ERR_BAD_ARG;
    }
    const uint64_t texel = im.color_type == RAYCA_COLOR_RGB8 ? 3u : im.color_type == RAYCA_COLOR_RGBA8 ? 4u : 16u;
    const uint64_t texels = (uint64_t)im.width * im.height;   // (two 32-bit factors: no overflow)
    if (im.byte_offset > d.image_byte_count || texels > (d.image_byte_count - im.byte_offset) / texel) {
      err = which + ": " + std::to_string(im.width) + " x " + std::to_string(im.height) + " texels of " + std::to_string(texel) + " bytes at byte_offset " +
            std::to_string(im.byte_offset) + " end beyond image_byte_count " + std::to_string(d.image_byte_count);
      return RAYCA_ERR_BAD_ARG;
    }
    if (im.color_type == RAYCA_COLOR_RGBA32F && im.byte_offset % 4u != 0u) {
      err = which + ": an RGBA32F image's byte_offset " + std::to_string(im.byte_offset) + " is not a multiple of 4";
      return RAYCA_ERR_BAD_ARG;
    }
  }
  return RAYCA_OK;
}

namespace {

constexpr int kAttrWidth[6] = {3, 4, 3, 3, 3, 2};
inline void attr_pointers(const RaycaSceneDesc& d, const float* (&p)[6]) {
  p[0] = d.positions; p[1] = d.colors; p[2] = d.normals; p[3] = d.tangents; p[4] = d.bitangents; p[5] = d.uvs;
}

// The counts of two descriptors (and the two words in front of them)
bool same_counts(const RaycaSceneDesc& a, const RaycaSceneDesc& b) {
  return a.abi_version == b.abi_version && a.flags == b.flags && a.node_count == b.node_count && a.mesh_count == b.mesh_count &&
         a.primitive_count == b.primitive_count && a.vertex_count == b.vertex_count && a.index_byte_count == b.index_byte_count &&
         a.material_count == b.material_count && a.texture_count == b.texture_count && a.image_count == b.image_count &&
         a.image_byte_count == b.image_byte_count && a.camera_count == b.camera_count && a.light_count == b.light_count;
}

template <class T>
bool same_table(const T* a, const T* b, size_t n) {
  return n == 0 || std::memcmp(a, b, n * sizeof(T)) == 0;
}

// memcmp of several pairs of large arrays at once: cut into chunks that the threads take in turn; the first difference
// found stops everybody at their next chunk
struct BytePair { const uint8_t *a, *b; size_t bytes; };
bool same_bytes_parallel(const std::vector<BytePair>& pairs) {
  constexpr size_t kChunk = size_t(256) << 10;
  struct Chunk { const uint8_t *a, *b; size_t bytes; };
  std::vector<Chunk> chunks;
  size_t total = 0;
  for (const BytePair& p : pairs)
    for (size_t at = 0; at < p.bytes; at += kChunk) {
      chunks.push_back(Chunk{p.a + at, p.b + at, std::min(kChunk, p.bytes - at)});
      total += chunks.back().bytes;
    }
  std::atomic<size_t> next{0};
  std::atomic<bool> differ{false};
  // (a thread costs some tens of microseconds to start: one per 1 MiB at most)
  run_on_host_threads((unsigned)std::max<size_t>(1, std::min<size_t>(host_threads(), total >> 20)), [&](unsigned) {
    for (;;) {
      if (differ.load(std::memory_order_relaxed)) return;
      const size_t i = next.fetch_add(1, std::memory_order_relaxed);
      if (i >= chunks.size()) return;
      if (std::memcmp(chunks[i].a, chunks[i].b, chunks[i].bytes) != 0) differ.store(true, std::memory_order_relaxed);
    }
  });
  return !differ.load();
}

}  // namespace

void KeptDesc::assign(const RaycaSceneDesc& d, bool use_bvh, SceneGraph&& g) {
  valid = false;
  bvh = use_bvh;
  nodes.assign(d.nodes, d.nodes + d.node_count);
  meshes.assign(d.meshes, d.meshes + d.mesh_count);
  primitives.assign(d.primitives, d.primitives + d.primitive_count);
  const float* src[6];
  attr_pointers(d, src);
  // the large arrays: sized without a fill, then copied piecewise on the host threads (first touch of ~10^7 bytes of fresh
  // pages on one thread costs more than the copy itself)
  struct Piece { uint8_t* to; const uint8_t* from; size_t bytes; };
  std::vector<Piece> pieces;
  auto take = [&pieces](uint8_t* to, const uint8_t* from, size_t bytes) {
    constexpr size_t kChunk = size_t(1) << 20;
    for (size_t at = 0; at < bytes; at += kChunk) pieces.push_back(Piece{to + at, from + at, std::min(kChunk, bytes - at)});
  };
  for (int k = 0; k < 6; ++k) {
    const bool has = src[k] != nullptr && d.vertex_count != 0;
    attr[k].resize(has ? (size_t)d.vertex_count * kAttrWidth[k] : 0);
    if (has) take(reinterpret_cast<uint8_t*>(attr[k].data()), reinterpret_cast<const uint8_t*>(src[k]), attr[k].size() * sizeof(float));
  }
  index_bytes.resize(d.index_byte_count);
  take(index_bytes.data(), d.index_bytes, d.index_byte_count);
  image_bytes.resize(d.image_byte_count);
  take(image_bytes.data(), d.image_bytes, d.image_byte_count);
  {
    std::atomic<size_t> next{0};
    run_on_host_threads((unsigned)std::max<size_t>(1, std::min<size_t>(host_threads(), pieces.size() / 2)), [&](unsigned) {
      for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < pieces.size();) std::memcpy(pieces[i].to, pieces[i].from, pieces[i].bytes);
    });
  }
  materials.assign(d.materials, d.materials + d.material_count);
  textures.assign(d.textures, d.textures + d.texture_count);
  images.assign(d.images, d.images + d.image_count);
  cameras.assign(d.cameras, d.cameras + d.camera_count);
  lights.assign(d.lights, d.lights + d.light_count);
  graph = std::move(g);
  view = d;
  view.nodes = nodes.data();
  view.meshes = meshes.data();
  view.primitives = primitives.data();
  const float** dst[6] = {&view.positions, &view.colors, &view.normals, &view.tangents, &view.bitangents, &view.uvs};
  for (int k = 0; k < 6; ++k) *dst[k] = attr[k].empty() ? nullptr : attr[k].data();
  view.index_bytes = index_bytes.data();
  view.materials = materials.data();
  view.textures = textures.data();
  view.images = images.data();
  view.image_bytes = image_bytes.data();
  view.cameras = cameras.data();
  view.lights = lights.data();
  valid = true;
}

void KeptDesc::refresh(const RaycaSceneDesc& d, SceneGraph&& g) {
  std::copy(d.nodes, d.nodes + d.node_count, nodes.begin());
  std::copy(d.cameras, d.cameras + d.camera_count, cameras.begin());
  std::copy(d.lights, d.lights + d.light_count, lights.begin());
  std::copy(d.materials, d.materials + d.material_count, materials.begin());
  graph = std::move(g);
}

uint64_t KeptDesc::bytes() const {
  if (!valid) return 0;
  uint64_t b = sizeof(RaycaNode) * nodes.size() + sizeof(RaycaMesh) * meshes.size() + sizeof(RaycaPrimitive) * primitives.size() +
               index_bytes.size() + image_bytes.size() + sizeof(RaycaMaterial) * materials.size() + sizeof(RaycaTexture) * textures.size() +
               sizeof(RaycaImage) * images.size() + sizeof(RaycaCamera) * cameras.size() + sizeof(RaycaLight) * lights.size();
  for (const auto& a : attr) b += sizeof(float) * a.size();
  b += sizeof(Trs) * (graph.local_trs.size() + graph.world_trs.size()) + sizeof(HostLight) * graph.lights.size();
  return b;
}

int32_t desc_compare(const RaycaSceneDesc& was, bool was_bvh, const SceneGraph* was_graph, const RaycaSceneDesc& next, bool next_bvh,
                     uint32_t& action, SceneGraph& next_graph, std::string& err) {
  if (const int32_t rc = desc_validate(next, err); rc != RAYCA_OK) return rc;
  action = RAYCA_DRAW_REBUILT;
  // ---- what an update cannot change: the tree kind, the counts, the geometry, the textures, the node topology ----
  bool fixed_equal = was_bvh == next_bvh && same_counts(was, next);
  bool edited = false;   // a node's trs, a camera, a light or a material differs
  if (fixed_equal) {
    fixed_equal = same_table(was.meshes, next.meshes, next.mesh_count) && same_table(was.primitives, next.primitives, next.primitive_count) &&
                  same_table(was.textures, next.textures, next.texture_count) && same_table(was.images, next.images, next.image_count);
  }
  for (uint32_t i = 0; fixed_equal && i < next.node_count; ++i) {
    const RaycaNode &a = next.nodes[i], &b = was.nodes[i];
    fixed_equal = a.parent == b.parent && a.model == b.model && a.mesh == b.mesh && a.camera == b.camera && a.light == b.light;
    edited = edited || std::memcmp(&a.trs, &b.trs, sizeof a.trs) != 0;
  }
  if (fixed_equal) {
    const float *pa[6], *pb[6];
    attr_pointers(was, pa);
    attr_pointers(next, pb);
    std::vector<BytePair> pairs;
    for (int k = 0; fixed_equal && k < 6; ++k) {
      const bool has_a = pa[k] && was.vertex_count, has_b = pb[k] && next.vertex_count;
      fixed_equal = has_a == has_b;   // (a null array means the default attribute, not "as before")
      if (has_a && has_b && pa[k] != pb[k])
        pairs.push_back(BytePair{reinterpret_cast<const uint8_t*>(pa[k]), reinterpret_cast<const uint8_t*>(pb[k]), sizeof(float) * kAttrWidth[k] * (size_t)next.vertex_count});
    }
    if (next.index_byte_count && was.index_bytes != next.index_bytes) pairs.push_back(BytePair{was.index_bytes, next.index_bytes, (size_t)next.index_byte_count});
    if (next.image_byte_count && was.image_bytes != next.image_bytes) pairs.push_back(BytePair{was.image_bytes, next.image_bytes, (size_t)next.image_byte_count});
    fixed_equal = fixed_equal && same_bytes_parallel(pairs);
  }
  if (fixed_equal) {
    edited = edited || !same_table(was.cameras, next.cameras, next.camera_count) || !same_table(was.lights, next.lights, next.light_count) ||
             !same_table(was.materials, next.materials, next.material_count);
    if (!edited) {
      action = RAYCA_DRAW_REUSED;
      return RAYCA_OK;
    }
  }
  if (const int32_t rc = scene_graph_pass(next, next_graph, err); rc != RAYCA_OK) return rc;
  if (!fixed_equal) return RAYCA_OK;   // REBUILT
  // ---- an edit of what rayca_hip_scene_update re-reads: does it leave the geometry where it is? ----
  SceneGraph made;
  if (!was_graph) {
    if (const int32_t rc = scene_graph_pass(was, made, err); rc != RAYCA_OK) return rc;
    was_graph = &made;
  }
  std::string why;
  if (next_graph.lights.size() == was_graph->lights.size() &&
      update_moves_geometry(next, next_graph, was_graph->world_trs, was_graph->lights, why) == RAYCA_OK)
    action = RAYCA_DRAW_UPDATED;
  return RAYCA_OK;
}

namespace {

struct TriJob {  // a run of triangles of one mesh primitive under one node, and where its HostPrims go
  uint32_t node, pi, first_tri, first_out, count;
  Mat3 tangent_matrix, normal_matrix;
  uint32_t model, blas_pos;   // its BLAS and the position of its first triangle in that BLAS's initial order
};
struct OtherPrim { uint32_t prim, model, blas_pos; };   // spheres, quad-light triangles: made where they are met, few
using Soa = std::vector<float, DefaultInitAllocator<float>>;   // nine planes of n floats, one block, BLAS order

// What passes between the phases of build_host_scene (below, in the order they run)
struct HostBuild {
  const RaycaSceneDesc& d;
  const uint32_t builder;
  const bool use_bvh;
  const BuildHooks& hooks;
  HostScene& s;       // what is being built
  std::string& err;   // filled by the phase that returns an error
  Lap lap;   // RAYCA_BUILD_TIMING=1: phase times of the host build on stderr
  // the device builder (thread_local: read here, the trees are built by other threads) and the layout's settings
  // (RAYCA_LEAF_NODE_COST / RAYCA_LEAF_MAX: experiments with the price of a node step -- 0 lays the tree out as built -- and
  // with the cap on a folded leaf, which hardly ever binds: 4, 8, 16 and 32 give the same 135 379 nodes on the atrium)
  const BlasBuildFn device_builder = g_device_builder;
  const uint32_t device_ordinal = g_device_ordinal;
  const float leaf_node_cost = [] { const char* e = getenv("RAYCA_LEAF_NODE_COST"); return e ? (float)atof(e) : kLeafNodeCost; }();
  const uint32_t leaf_max = [] { const char* e = getenv("RAYCA_LEAF_MAX"); return e ? (uint32_t)std::min(std::max(atoi(e), 1), (int)kLeafMaxPrims) : kLeafCollapseMax; }();
  SceneGraph g;
  std::vector<uint32_t> models;   // flatten_slots: ascending; one BLAS each, in that order until they move into s.blas in TLAS order
  std::vector<HostBlas> blas;
  std::vector<TriJob> jobs;       // what flatten_fill has to do
  std::vector<OtherPrim> others;
  // flatten_fill: what the device builder reads, world centroids and boxes of a BLAS's primitives in the BLAS's initial order
  // (the two trees of a RAYCA_BUILDER_SAH scene start from the same order and share one copy); empty: built on the host
  std::vector<Soa> soas;
  // build_trees: the root boxes, and the reference's tree and order of the primitives inside each BLAS (RAYCA_BUILDER_SAH:
  // the order is the tie rule, the leaves are the candidate filter)
  std::vector<Box> blas_root;
  std::vector<std::vector<uint32_t>> ref_prims;
  std::vector<std::vector<BuildNode>> ref_nodes;
  std::vector<TNode> tn;                                       // order_and_reference_tables: the TLAS, the BLASes in its order,
  std::vector<uint32_t> blas_order, ref_rank, ref_leaf_flat;   // flatten index -> slot in the reference's global order / its leaf
};

// What every primitive and its shading record hold, whatever they are made from; in place (a mesh triangle's slot is not pre-zeroed)
inline void init_prim(HostPrim& hp, PrimExt& ext, uint32_t kind, uint32_t node, uint32_t material, uint32_t src) {
  hp.kind = kind; hp.node = node; hp.material = material; hp.src = src;
  std::memset(&ext, 0, sizeof ext);
  ext.kind = kind; ext.node = node; ext.material = material;
}

// SceneDrawInfo::new, then BvhScene::from_scene's order: models in ascending id; per model its meshes, then its quad lights.
// Spheres and quad-light triangles are made here; a mesh triangle gets its slot (s.prims, s.ext, its BLAS's order) and a TriJob.
int32_t flatten_slots(HostBuild& b) {
  const RaycaSceneDesc& d = b.d;
  HostScene& s = b.s;
  if (const int32_t rc = scene_graph_pass(d, b.g, b.err); rc != RAYCA_OK) return rc;
  s.nodes.assign(d.nodes, d.nodes + d.node_count);
  s.local_trs = std::move(b.g.local_trs);
  s.world_trs = std::move(b.g.world_trs);
  s.has_camera = b.g.has_camera;
  s.camera_node = b.g.camera_node;
  s.camera_yfov = b.g.camera_yfov;
  s.lights = std::move(b.g.lights);
  const std::vector<uint32_t>&mesh_nodes = b.g.mesh_nodes, &light_nodes = b.g.light_nodes;
  s.materials.assign(d.materials, d.materials + d.material_count);
  s.textures.assign(d.textures, d.textures + d.texture_count);
  s.images.assign(d.images, d.images + d.image_count);
  s.image_bytes.assign(d.image_bytes, d.image_bytes + d.image_byte_count);

  std::vector<uint32_t>& models = b.models;
  for (uint32_t n : mesh_nodes) models.push_back(d.nodes[n].model);
  for (uint32_t n : light_nodes)
    if (d.lights[d.nodes[n].light].kind == RAYCA_LIGHT_QUAD) models.push_back(d.nodes[n].model);
  std::sort(models.begin(), models.end());
  models.erase(std::unique(models.begin(), models.end()), models.end());

  std::vector<HostBlas>& blas = b.blas;
  blas.resize(models.size());
  {  // one allocation for the flatten-order array: growing it piecewise re-copied 0.5 KB per triangle several times over
    size_t total = 2 * light_nodes.size();
    for (uint32_t node : mesh_nodes) {
      const RaycaMesh& mesh = d.meshes[d.nodes[node].mesh];
      for (uint32_t pi = mesh.first_primitive; pi < mesh.first_primitive + mesh.primitive_count && pi < d.primitive_count; ++pi)
        total += d.primitives[pi].geometry == RAYCA_GEOMETRY_SPHERE ? 1u : d.primitives[pi].index_count / 3u;
    }
    s.prims.reserve(total);
    s.ext.reserve(total);
  }
  for (size_t m = 0; m < models.size(); ++m) {
    blas[m].model = models[m];
    auto push_other = [&](const HostPrim& hp, const PrimExt& ext) {  // a finished primitive at the end of the arrays and of BLAS m
      b.others.push_back(OtherPrim{hp.src, (uint32_t)m, (uint32_t)blas[m].prims.size()});
      blas[m].prims.push_back(hp.src);
      s.prims.push_back(hp);
      s.ext.push_back(ext);
    };
    for (uint32_t node : mesh_nodes) {
      if (d.nodes[node].model != models[m]) continue;
      const RaycaMesh& mesh = d.meshes[d.nodes[node].mesh];
      const Trs& trs = s.world_trs[node];
      const Mat3 tangent_matrix = mat3_from_trs(trs);                             // primitive.rs:203-204
      const Mat3 normal_matrix = mat3_transpose(mat3_from_inverse_trs(trs));      // primitive.rs:206-207
      for (uint32_t pi = mesh.first_primitive; pi < mesh.first_primitive + mesh.primitive_count; ++pi) {
        if (pi >= d.primitive_count) { b.err = "primitive index out of range"; return RAYCA_ERR_BAD_ARG; }
        const RaycaPrimitive& p = d.primitives[pi];
        if (p.geometry == RAYCA_GEOMETRY_SPHERE) {  // from_sphere  primitive.rs:262-274
          HostPrim hp{};
          PrimExt ext;
          init_prim(hp, ext, RAYCA_GEOMETRY_SPHERE, node, p.material, (uint32_t)s.prims.size());
          hp.center = point3(p.sphere_center[0], p.sphere_center[1], p.sphere_center[2]);
          hp.radius = p.sphere_radius;
          push_other(hp, ext);
          s.sphere_count++;
          continue;
        }
        // from_triangle_mesh_impl  primitive.rs:209-234: the triangles are independent -- slots are reserved
        // here, in order, and filled by all host threads in flatten_fill
        const uint32_t ntri = p.index_count / 3;
        const uint32_t first_out = (uint32_t)s.prims.size();
        for (uint32_t at = 0; at < ntri; at += 8192)  // pieces, so that one huge mesh still feeds every thread
          b.jobs.push_back(TriJob{node, pi, at, first_out + at, std::min<uint32_t>(8192u, ntri - at), tangent_matrix, normal_matrix, (uint32_t)m,
                                  (uint32_t)blas[m].prims.size() + at});
        s.prims.resize((size_t)first_out + ntri);
        s.ext.resize((size_t)first_out + ntri);
        {
          const size_t at = blas[m].prims.size();
          blas[m].prims.resize(at + ntri);  // (geometric growth: a model of many small meshes must not reallocate per mesh)
          for (uint32_t t = 0; t < ntri; ++t) blas[m].prims[at + t] = first_out + t;
        }
        s.triangle_count += ntri;
      }
    }
    for (uint32_t node : light_nodes) {  // from_quad_light  primitive.rs:310-346
      const RaycaLight& l = d.lights[d.nodes[node].light];
      if (d.nodes[node].model != models[m] || l.kind != RAYCA_LIGHT_QUAD) continue;
      const F4 ab = vec3(l.ab[0], l.ab[1], l.ab[2]), ac = vec3(l.ac[0], l.ac[1], l.ac[2]);
      const F4 normal = normalized(cross(ab, ac));
      const F4 qa = point3(0, 0, 0);
      const F4 a = qa, bb = qa + ab, dd = (qa + ab) + ac, c = qa + ac;
      const F4 tri[2][3] = {{a, dd, bb}, {a, c, dd}};
      for (int t = 0; t < 2; ++t) {
        HostPrim hp{};
        PrimExt ext;
        init_prim(hp, ext, RAYCA_GEOMETRY_TRIANGLE_MESH, node, l.material, (uint32_t)s.prims.size());
        for (int k = 0; k < 3; ++k) {
          hp.p[k] = tri[t][k];
          set_ext(ext, k, white(), normal, vec3(0, 0, 0), vec3(0, 0, 0), F2{0, 0});
        }
        hp.centroid = ((to_vec(hp.p[0]) + to_vec(hp.p[1])) + to_vec(hp.p[2])) * 0.3333f;
        push_other(hp, ext);
        s.triangle_count++;
      }
    }
  }
  return RAYCA_OK;
}

// What follows from a primitive's model-space record: the world-space vertices / centroid / box (cache_world), the 9 floats of
// the device's triangle array, and -- for a BLAS the device builds -- its row of the SoA the device builder reads
inline void finish_prim(HostBuild& b, uint32_t prim, uint32_t model, uint32_t blas_pos) {
  HostScene& s = b.s;
  HostPrim& p = s.prims[prim];
  cache_world(p, s.world_trs[p.node]);
  float* tv = &s.tris[(size_t)prim * 9];
  for (int k = 0; k < 3; ++k) {
    tv[3 * k + 0] = p.wp[k].x;
    tv[3 * k + 1] = p.wp[k].y;
    tv[3 * k + 2] = p.wp[k].z;
  }
  Soa& soa = b.soas[model];
  if (!soa.empty()) {
    const size_t n = soa.size() / 9, i = blas_pos;
    float* const q = soa.data();
    q[i] = p.wcentroid.x; q[n + i] = p.wcentroid.y; q[2 * n + i] = p.wcentroid.z;
    q[3 * n + i] = p.wmin.x; q[4 * n + i] = p.wmin.y; q[5 * n + i] = p.wmin.z;
    q[6 * n + i] = p.wmax.x; q[7 * n + i] = p.wmax.y; q[8 * n + i] = p.wmax.z;
  }
}

// One pass of all host threads fills the reserved triangle slots and finishes them; then the few others are finished.  (Three
// passes before: each touched the 0.5 KB per primitive again and paid a round of thread starts.)
int32_t flatten_fill(HostBuild& b) {
  const RaycaSceneDesc& d = b.d;
  HostScene& s = b.s;
  static const bool host_only = getenv("RAYCA_HOST_BUILD") != nullptr;
  b.soas.resize(b.blas.size());
  for (size_t m = 0; m < b.blas.size(); ++m)
    if (b.device_builder && !host_only && b.use_bvh && b.blas[m].prims.size() >= kDeviceBuildMin) b.soas[m].resize(9 * b.blas[m].prims.size());
  s.tris.resize(s.prims.size() * 9);
  if (!b.jobs.empty()) {
    const std::vector<TriJob>& jobs = b.jobs;
    std::atomic<int> failed{0};
    const char* first_error = nullptr;
    std::atomic<size_t> next_job{0};
    run_on_host_threads(std::max(1u, std::min<unsigned>(host_threads(), (unsigned)jobs.size())), [&](unsigned) {
      for (;;) {
        const size_t j = next_job.fetch_add(1);
        if (j >= jobs.size() || failed.load(std::memory_order_relaxed)) return;
        const TriJob& job = jobs[j];
        const RaycaPrimitive& p = d.primitives[job.pi];
        for (uint32_t t = 0; t < job.count; ++t) {
          const uint32_t tri = job.first_tri + t;
          HostPrim& hp = s.prims[job.first_out + t];  // written in place, every field (the array is not pre-zeroed)
          PrimExt& ext = s.ext[job.first_out + t];
          init_prim(hp, ext, RAYCA_GEOMETRY_TRIANGLE_MESH, job.node, p.material, job.first_out + t);
          hp.center = point3(0, 0, 0);
          hp.radius = 0.0f;
          const char* problem = nullptr;
          for (int k = 0; k < 3; ++k) {
            uint32_t idx;
            if (!fetch_index(d, p, tri * 3 + (uint32_t)k, idx)) { problem = "index fetch out of range or unsupported index type"; break; }
            if (idx >= p.vertex_count || p.first_vertex + idx >= d.vertex_count) { problem = "vertex index out of range"; break; }
            const uint32_t v = p.first_vertex + idx;
            hp.p[k] = point3(d.positions[3 * v], d.positions[3 * v + 1], d.positions[3 * v + 2]);
            const Color c = d.colors ? rgba(d.colors[4 * v], d.colors[4 * v + 1], d.colors[4 * v + 2], d.colors[4 * v + 3]) : white();
            const F4 nrm = d.normals ? vec3(d.normals[3 * v], d.normals[3 * v + 1], d.normals[3 * v + 2]) : vec3(0, 0, 1);
            const F4 tan = d.tangents ? vec3(d.tangents[3 * v], d.tangents[3 * v + 1], d.tangents[3 * v + 2]) : vec3(0, 0, 0);
            const F4 bit = d.bitangents ? vec3(d.bitangents[3 * v], d.bitangents[3 * v + 1], d.bitangents[3 * v + 2]) : vec3(0, 0, 0);
            const F2 uv = d.uvs ? F2{d.uvs[2 * v], d.uvs[2 * v + 1]} : F2{0, 0};
            set_ext(ext, k, c, mat3_apply(job.normal_matrix, nrm), mat3_apply(job.tangent_matrix, tan), mat3_apply(job.tangent_matrix, bit), uv);
          }
          if (problem) {
            if (!failed.exchange(1)) first_error = problem;
            return;
          }
          hp.centroid = ((to_vec(hp.p[0]) + to_vec(hp.p[1])) + to_vec(hp.p[2])) * 0.3333f;  // triangle.rs:59-63
          finish_prim(b, job.first_out + t, job.model, job.blas_pos + t);
        }
      }
    });
    if (failed.load()) { b.err = first_error ? first_error : "bad triangle data"; return RAYCA_ERR_BAD_ARG; }
  }
  for (const OtherPrim& o : b.others) finish_prim(b, o.prim, o.model, o.blas_pos);
  return RAYCA_OK;
}

// One tree over BLAS m's primitives, initially in `order`, on the host or -- where flatten_fill made an SoA -- by the device
// builder.  `quiet`: the second tree of a BLAS, built beside the first: no lap lines, and the root box is the other's to write.
bool build_blas(HostBuild& b, size_t m, bool seed_origin, std::vector<uint32_t>& order, std::vector<BuildNode>& nodes, std::string& build_err,
                bool quiet, BlasDeviceTree* keep, void* stream) {
  unsigned par_levels = 0;
  while ((1u << par_levels) < host_threads()) ++par_levels;
  BlasBuilder bb{&b.s, &order, b.use_bvh ? 255u : 0u, par_levels + 1, seed_origin};
  std::vector<BuildNode> arena(1);
  arena[0].offset = 0;
  arena[0].count = (uint32_t)order.size();
  arena[0].bounds = bb.range_bounds(0, arena[0].count);
  const uint32_t n = arena[0].count;
  const Soa& soa = b.soas[m];
  if (soa.size() == 9 * (size_t)n && n > 0) {
    // the same recursion, level by level on the GPU (bvh_build.hip): identical tree, boxes and order
    BlasBuildInput in{};
    for (int c = 0; c < 3; ++c) {
      in.cent[c] = soa.data() + (size_t)c * n;
      in.bmin[c] = soa.data() + (size_t)(3 + c) * n;
      in.bmax[c] = soa.data() + (size_t)(6 + c) * n;
    }
    in.count = n;
    in.root_min[0] = arena[0].bounds.a.x; in.root_min[1] = arena[0].bounds.a.y; in.root_min[2] = arena[0].bounds.a.z;
    in.root_max[0] = arena[0].bounds.b.x; in.root_max[1] = arena[0].bounds.b.y; in.root_max[2] = arena[0].bounds.b.z;
    in.seed_origin = seed_origin;
    in.max_depth = 255u;
    in.device = b.device_ordinal;
    in.stream = stream;
    in.layout_node_cost = seed_origin ? 0.0f : b.leaf_node_cost;
    in.layout_leaf_max = b.leaf_max;
    std::vector<uint32_t> perm;
    // (the arena as the host builder would have made it -- or, with `keep`, the tree left on the device and only its root here)
    if (!b.device_builder(in, perm, arena, build_err, keep)) return false;
    b.lap("  gpu build (total)", quiet);
    std::vector<uint32_t> permuted(n);
    parallel_chunks(n, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) permuted[i] = order[perm[i]];
    });
    order.swap(permuted);
  } else if (n > 0) {
    bb.split(arena, 0, 0);
  }
  b.lap("  host: apply order, arena", quiet);
  if (!quiet) b.blas_root[m] = arena[0].bounds;  // (the same box for both trees of a BLAS: written by one of them)
  nodes.swap(arena);
  return true;
}

// The traversed tree of a device-built BLAS that stayed on the device: the scene owns it, the BLAS knows its layout's size
void adopt_kept_tree(HostBlas& bl, const BlasDeviceTree& kept, HostScene& s) {
  if (!kept.handle) return;
  s.dev_trees.push_back(kept.handle);
  bl.dev_tree = kept.handle;
  bl.dev_node_count = kept.node_count;
  bl.dev_need = kept.need;
}

// Tlas::new: one BLAS per model.  RAYCA_BUILDER_SAH builds two independent trees over the same primitives side by side -- the
// reference's (tie order + candidate filter) on a thread of its own -- so that one's host phases run under the other's GPU levels.
int32_t build_trees(HostBuild& b) {
  HostScene& s = b.s;
  std::vector<HostBlas>& blas = b.blas;
  b.blas_root.resize(blas.size());
  b.ref_prims.resize(blas.size());
  b.ref_nodes.resize(blas.size());
  // the traversed tree of a device-built BLAS stays on the device and is laid out there (HostBlas::dev_tree) -- unless the
  // other node formats are to be made right here, on the host, from the host's copy of the binary nodes
  const bool keep_trees = !b.hooks.with_formats;
  void* const bstream[2] = {b.hooks.build_streams ? b.hooks.build_streams[0] : nullptr, b.hooks.build_streams ? b.hooks.build_streams[1] : nullptr};
  s.dev_segments.clear();
  s.dev_trees.clear();
  const bool with_reference = b.builder == RAYCA_BUILDER_SAH;
  for (size_t m = 0; m < blas.size(); ++m) {
    std::string e_ref, e;
    bool ok_ref = true;
    std::thread ref_thread;
    if (with_reference) {
      b.ref_prims[m] = blas[m].prims;
      ref_thread = std::thread([&] { ok_ref = build_blas(b, m, true, b.ref_prims[m], b.ref_nodes[m], e_ref, true, nullptr, bstream[0]); });
    }
    BlasDeviceTree kept;
    const bool ok = build_blas(b, m, !with_reference, blas[m].prims, blas[m].nodes, e, false, keep_trees ? &kept : nullptr, bstream[1]);
    adopt_kept_tree(blas[m], kept, s);
    if (with_reference) {
      ref_thread.join();
      b.lap("reference tree + SAH tree");
    }
    if (!ok_ref || !ok) { b.err = !ok_ref ? e_ref : e; return RAYCA_ERR_HIP; }
  }
  return RAYCA_OK;
}

// The TLAS over the BLAS root boxes, the BLASes moved into its order (a TLAS range [offset, offset + count) indexes s.blas
// directly), and -- RAYCA_BUILDER_SAH -- the reference's tables by flatten index: rank in its global order, leaf, leaf boxes
int32_t order_and_reference_tables(HostBuild& b) {
  HostScene& s = b.s;
  std::vector<HostBlas>& blas = b.blas;
  b.blas_order.resize(blas.size());
  for (size_t i = 0; i < blas.size(); ++i) b.blas_order[i] = (uint32_t)i;
  b.tn.assign(1, TNode{});
  if (!blas.empty()) tlas_split(b.tn, 0, b.blas_order, b.blas_root, 0, (uint32_t)blas.size());
  s.blas.clear();
  s.ref_leaf_boxes.clear();
  if (b.builder == RAYCA_BUILDER_SAH) {
    b.ref_rank.assign(s.prims.size(), 0);
    b.ref_leaf_flat.assign(s.prims.size(), 0);
    uint32_t slot = 0;
    for (uint32_t bi : b.blas_order) {
      for (uint32_t pi : b.ref_prims[bi]) b.ref_rank[pi] = slot++;
      for (const BuildNode& rn : b.ref_nodes[bi]) {
        if (rn.left >= 0 || rn.count == 0) continue;  // inner node (or the root of an empty BLAS)
        const uint32_t leaf = (uint32_t)(s.ref_leaf_boxes.size() / 8);
        const float bx[8] = {rn.bounds.a.x, rn.bounds.a.y, rn.bounds.a.z, 0.0f, rn.bounds.b.x, rn.bounds.b.y, rn.bounds.b.z, 0.0f};
        s.ref_leaf_boxes.insert(s.ref_leaf_boxes.end(), bx, bx + 8);
        for (uint32_t i = rn.offset; i < rn.offset + rn.count; ++i) b.ref_leaf_flat[b.ref_prims[bi][i]] = leaf;
      }
    }
  }
  for (uint32_t bi : b.blas_order) s.blas.push_back(std::move(blas[bi]));
  return RAYCA_OK;
}

// The binary f32 nodes of the whole scene (DevBuilder), the slot order of the primitives, and the reference's tables by slot
int32_t layout_binary(HostBuild& b) {
  HostScene& s = b.s;
  const std::vector<TNode>& tn = b.tn;
  s.dev_nodes.clear();
  s.prim_order.clear();
  s.max_depth = 0;
  if (s.blas.empty()) return RAYCA_OK;
  DevBuilder db{s, {}};
  if (b.builder == RAYCA_BUILDER_SAH) {
    // This tree's boxes only have to be conservative (the reference-leaf filter decides candidacy):
    // pad them by 2^-16 of their magnitude plus 2^-20 of the scene diagonal, two orders of magnitude
    // above the rounding of the slab and triangle arithmetic for a ray that starts within four scene
    // diagonals of the origin, so that a triangle such a ray hits is never lost because an enclosing
    // box rounds the other way.  The padding cannot know a ray's origin: rays from farther away carry
    // a slack of their own through the steering tests (trace_core.inc, RAYCA_RAY_SLACK).
    const F4 ext = as_vec(tn[0].bounds.b - tn[0].bounds.a);
    const float diag = sqrtf(ext.x * ext.x + ext.y * ext.y + ext.z * ext.z);
    db.pad_rel = 1.52587890625e-05f;
    db.pad_abs = (diag == diag && diag < FLT_MAX) ? diag * 9.5367431640625e-07f : 0.0f;
  }
  s.pad_rel = db.pad_rel;
  s.pad_abs = db.pad_abs;
  db.node_cost = b.builder == RAYCA_BUILDER_SAH ? b.leaf_node_cost : 0.0f;
  db.leaf_max = b.leaf_max;
  uint32_t base = 0;
  for (const HostBlas& bl : s.blas) {
    db.blas_base.push_back(base);
    for (uint32_t pi : bl.prims) s.prim_order.push_back(pi);
    base += (uint32_t)bl.prims.size();
  }
  if (base > kLeafFirstMask) { b.err = "too many primitives for the packed leaf reference (max 33554431)"; return RAYCA_ERR_UNSUPPORTED; }
  if (b.hooks.on_order_ready) b.hooks.on_order_ready();
  s.root_min = tn[0].bounds.a;
  s.root_max = tn[0].bounds.b;
  uint32_t need = 0;
  s.root_ref = db.emit_tlas(tn, 0, need);
  if (!db.error.empty()) { b.err = db.error; return RAYCA_ERR_BAD_ARG; }
  s.max_depth = need;
  b.lap("  binary nodes");
  s.tie_rank.clear();
  s.ref_leaf_of.clear();
  if (b.builder == RAYCA_BUILDER_SAH) {
    s.tie_rank.resize(s.prim_order.size());
    s.ref_leaf_of.resize(s.prim_order.size());
    parallel_chunks(s.prim_order.size(), [&](size_t lo, size_t hi) {
      for (size_t slot = lo; slot < hi; ++slot) {
        s.tie_rank[slot] = b.ref_rank[s.prim_order[slot]];
        s.ref_leaf_of[slot] = b.ref_leaf_flat[s.prim_order[slot]];
      }
    });
  }
  return RAYCA_OK;
}

}  // namespace

int32_t build_host_scene(const RaycaSceneDesc& d, bool use_bvh, uint32_t builder, HostScene& s, std::string& err, const BuildHooks& hooks) {
  if (d.abi_version != RAYCA_ABI_VERSION) { err = "abi version mismatch"; return RAYCA_ERR_BAD_ARG; }
  if (d.node_count && !d.nodes) { err = "nodes is null"; return RAYCA_ERR_BAD_ARG; }
  if (d.vertex_count && !d.positions) { err = "positions is null"; return RAYCA_ERR_BAD_ARG; }
  HostBuild b{d, builder, use_bvh, hooks, s, err};
  int32_t rc;
  if ((rc = flatten_slots(b)) != RAYCA_OK) return rc;
  b.lap("flatten: graph, slots");
  if ((rc = flatten_fill(b)) != RAYCA_OK) return rc;
  b.lap("flatten primitives, world space, SoA");
  if (hooks.on_prims_ready) hooks.on_prims_ready();
  if ((rc = build_trees(b)) != RAYCA_OK) return rc;
  if ((rc = order_and_reference_tables(b)) != RAYCA_OK) return rc;
  b.lap("TLAS + reference tables");
  if ((rc = layout_binary(b)) != RAYCA_OK) return rc;
  // the other three node formats are only ever traversed next to the reference-leaf filter
  s.dev_nodes4.clear();
  s.dev_nodes_h.clear();
  s.dev_nodes4_h.clear();
  s.root_ref4 = s.max_depth4 = 0;
  s.other_formats_wanted = builder == RAYCA_BUILDER_SAH && !s.blas.empty();
  if (hooks.with_formats) finish_node_formats(s);
  b.lap("device node layouts");
  return RAYCA_OK;
}

}  // namespace rayca
