// Host-side scene build on the CPU (no HIP): phase times of build_host_scene with RAYCA_BUILD_TIMING=1, and digests of
// everything it makes.  A tool for working on the builder without a GPU; built and driven by tests/host_build_probe.py.
#include "../../rayca_amd/csrc/host_scene.hpp"
#include <chrono>
#include <cstdio>
#include <cstring>
extern "C" int host_build_probe(const RaycaSceneDesc* d, unsigned builder, int repeats) {
  for (int r = 0; r < repeats; ++r) {
    rayca::HostScene s;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t rc = rayca::build_host_scene(*d, true, builder, s, err);
    const auto t1 = std::chrono::steady_clock::now();
    if (rc) { fprintf(stderr, "build failed: %s\n", err.c_str()); return rc; }
    fprintf(stderr, "[probe] build #%d: %.3f ms, %zu nodes, %zu 4-wide, stack need %u / %u\n", r, std::chrono::duration<float, std::milli>(t1 - t0).count(), s.dev_nodes.size(), s.dev_nodes4.size(), s.max_depth, s.max_depth4);
  }
  return 0;
}

// One build; `out` receives lines "name value": a 64-bit FNV-1a digest (hex) of the bytes of every array the build leaves
// behind, and the scalars themselves (floats as the hex of their bits).  HostScene::prims is left out: HostPrim has padding,
// and what it holds reaches `tris`, `ext` and the trees.  Returns the build's code, or -1 when `out` is too small.
namespace {
template <class V>
unsigned long long fnv1a(const V& v) {
  unsigned long long h = 0xcbf29ce484222325ull;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0, n = v.size() * sizeof(*v.data()); i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}
unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}
}  // namespace
extern "C" int host_build_digests(const RaycaSceneDesc* d, unsigned builder, int use_bvh, char* out, size_t cap) {
  rayca::HostScene s;
  std::string err;
  const int32_t rc = rayca::build_host_scene(*d, use_bvh != 0, builder, s, err);
  if (rc) { fprintf(stderr, "build failed: %s\n", err.c_str()); return rc; }
  std::string t;
  char line[160];
  auto put = [&](const char* name, unsigned long long v, const char* fmt) {
    snprintf(line, sizeof line, fmt, name, v);
    t += line;
  };
  auto digest = [&](const char* name, const auto& v) {
    put((std::string(name) + ".count").c_str(), v.size(), "%s %llu\n");
    put(name, fnv1a(v), "%s %016llx\n");
  };
  auto scalar = [&](const char* name, unsigned v) { put(name, v, "%s %llu\n"); };
  auto real = [&](const char* name, float v) { put(name, bits(v), "%s f%08llx\n"); };
  digest("dev_nodes", s.dev_nodes);
  digest("dev_nodes4", s.dev_nodes4);
  digest("dev_nodes_h", s.dev_nodes_h);
  digest("dev_nodes4_h", s.dev_nodes4_h);
  digest("prim_order", s.prim_order);
  digest("tie_rank", s.tie_rank);
  digest("ref_leaf_boxes", s.ref_leaf_boxes);
  digest("ref_leaf_of", s.ref_leaf_of);
  {  // the same two without the numbering of the leaves (which follows the arena, and the arena the number of host threads)
    std::vector<float> box_of_slot;
    for (const uint32_t leaf : s.ref_leaf_of) box_of_slot.insert(box_of_slot.end(), &s.ref_leaf_boxes[8 * (size_t)leaf], &s.ref_leaf_boxes[8 * (size_t)leaf] + 8);
    digest("ref_leaf_box_of_slot", box_of_slot);
  }
  digest("tris", s.tris);
  digest("ext", s.ext);
  scalar("blas.count", (unsigned)s.blas.size());
  for (size_t b = 0; b < s.blas.size(); ++b) digest(("blas" + std::to_string(b) + ".prims").c_str(), s.blas[b].prims);
  scalar("root_ref", s.root_ref);
  scalar("root_ref4", s.root_ref4);
  scalar("max_depth", s.max_depth);
  scalar("max_depth4", s.max_depth4);
  const float lo[3] = {s.root_min.x, s.root_min.y, s.root_min.z}, hi[3] = {s.root_max.x, s.root_max.y, s.root_max.z};
  for (int c = 0; c < 3; ++c) {
    real(("root_min." + std::to_string(c)).c_str(), lo[c]);
    real(("root_max." + std::to_string(c)).c_str(), hi[c]);
    real(("half_center." + std::to_string(c)).c_str(), s.half_center[c]);
  }
  real("pad_rel", s.pad_rel);
  real("pad_abs", s.pad_abs);
  real("half_scale", s.half_scale);
  scalar("triangle_count", s.triangle_count);
  scalar("sphere_count", s.sphere_count);
  if (t.size() + 1 > cap) return -1;
  std::memcpy(out, t.c_str(), t.size() + 1);
  return 0;
}
