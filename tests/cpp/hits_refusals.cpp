// The host side of rayca_hip_hits_device that needs no device, as a stand-alone program: every struct-level refusal in its
// documented order, the options' checks, the empty batch, and the kernel pickers' self-test (pick_hits_kernel among them).  The
// scene handle is 64 bytes of zeros: every path taken here ends in front of the first look at it.  Meant to be linked against a
// build of the library whose HOST code carries -fsanitize=address,undefined (DESIGN 4.17 has the command); prints "ok" and
// returns 0, or names the first expectation that failed.
#include "../../include/rayca_hip.h"
#include <cmath>
#include <cstdio>
#include <cstring>

static int failures = 0;
static const char* last_error() {
  static char buf[512];
  rayca_hip_last_error(buf, sizeof buf);
  return buf;
}
static void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (last error: %s)\n", what, last_error());
    ++failures;
  }
}
static bool says(const char* part) { return std::strstr(last_error(), part) != nullptr; }

int main() {
  alignas(16) static unsigned char dummy[64] = {};
  RaycaScene* scene = reinterpret_cast<RaycaScene*>(dummy);
  RaycaHits good{};
  good.count = 4; good.k = 3; good.rays = dummy; good.tmax_all = INFINITY; good.t_out = dummy; good.n_out = dummy;
  RaycaRenderOptions bad_opts{};
  bad_opts.context = 8; bad_opts.engine = 1;

  expect(rayca_hip_hits_device(nullptr, nullptr, &good, nullptr) == RAYCA_ERR_BAD_ARG && says("null scene"), "NULL scene");
  expect(rayca_hip_hits_device(scene, nullptr, nullptr, nullptr) == RAYCA_ERR_BAD_ARG && says("null"), "NULL query");
  // one rule broken at a time, with bad options behind it: the struct's rule is the one reported
  struct Case { const char* what; const char* message; void (*breaks)(RaycaHits&); };
  const Case cases[] = {
      {"NULL rays", "null rays", [](RaycaHits& q) { q.rays = nullptr; }},
      {"k > RAYCA_HITS_MAX", "RAYCA_HITS_MAX", [](RaycaHits& q) { q.k = RAYCA_HITS_MAX + 1u; }},
      {"unknown faces", "unknown faces", [](RaycaHits& q) { q.faces = 2; }},
      {"count_all > 1", "count_all", [](RaycaHits& q) { q.count_all = 2; }},
      {"reserved", "reserved", [](RaycaHits& q) { q.reserved = 1; }},
      {"k == 0 without count_all", "needs count_all", [](RaycaHits& q) { q.k = 0; q.t_out = nullptr; }},
      {"no output", "no output", [](RaycaHits& q) { q.t_out = nullptr; q.n_out = nullptr; }},
      {"a record output with k == 0", "k == 0", [](RaycaHits& q) { q.k = 0; q.count_all = 1; }},
  };
  const size_t n_cases = sizeof cases / sizeof cases[0];
  for (size_t first = 0; first < n_cases; ++first) {
    RaycaHits q = good;
    cases[first].breaks(q);
    expect(rayca_hip_hits_device(scene, &bad_opts, &q, nullptr) == RAYCA_ERR_BAD_ARG && says(cases[first].message), cases[first].what);
  }
  // the order: rule i together with every rule behind it that can be broken at the same time reports rule i
  for (size_t first = 0; first <= 4; ++first) {
    RaycaHits q = good;
    for (size_t j = first; j <= 4; ++j) cases[j].breaks(q);   // rays, k, faces, count_all, reserved: independent fields
    q.t_out = nullptr; q.n_out = nullptr;                     // and no output behind them
    expect(rayca_hip_hits_device(scene, &bad_opts, &q, nullptr) == RAYCA_ERR_BAD_ARG && says(cases[first].message), "the order of the refusals");
  }
  expect(rayca_hip_hits_device(scene, &bad_opts, &good, nullptr) == RAYCA_ERR_BAD_ARG && says("context"), "context > 7");
  RaycaRenderOptions o{};
  o.engine = 1;
  expect(rayca_hip_hits_device(scene, &o, &good, nullptr) == RAYCA_ERR_BAD_ARG && says("engine") && says("multi-hit query"), "an option that does not apply");
  o = RaycaRenderOptions{};
  o.traversal = RAYCA_TRAVERSAL_EXHAUSTIVE + 1;
  expect(rayca_hip_hits_device(scene, &o, &good, nullptr) == RAYCA_ERR_BAD_ARG && says("unknown traversal"), "unknown traversal");
  // the empty batch: RAYCA_OK behind the checks, statistics zeroed, nothing read of the scene
  RaycaHits empty = good;
  empty.count = 0;
  RaycaStats st;
  std::memset(&st, 0x5A, sizeof st);
  o = RaycaRenderOptions{};
  o.traversal = RAYCA_TRAVERSAL_EXHAUSTIVE; o.collect_stats = 1; o.context = 7;
  expect(rayca_hip_hits_device(scene, &o, &empty, &st) == RAYCA_OK && st.kernel_launches == 0 && st.rays_primary == 0, "the empty batch");
  empty.k = 0; empty.count_all = 1; empty.t_out = nullptr;
  expect(rayca_hip_hits_device(scene, nullptr, &empty, nullptr) == RAYCA_OK, "the empty crossing count");
  expect(rayca_hip_selftest() == RAYCA_OK, "rayca_hip_selftest (the kernel pickers)");
  if (failures == 0) std::puts("ok");
  return failures == 0 ? 0 : 1;
}
