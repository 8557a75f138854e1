// resident_draw -- the C++ mirror's SoftRenderer::draw called twice on one scene (tests/test_gpu_resident_draw.py):
//   resident_draw <box.gltf> <out dir>
// writes <out dir>/first.bin and second.bin (256x256 RGBA8) and prints one line per draw: action, builds, reuses.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "rayca.hpp"
#include "rayca_gltf.hpp"

using namespace rayca;

static void dump(const std::string& path, const std::vector<uint8_t>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) std::exit(3);
  std::fwrite(v.data(), 1, v.size(), f);
  std::fclose(f);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: resident_draw <box.gltf> <out dir>\n");
    return 2;
  }
  try {
    const std::string out = argv[2];
    SoftRenderer renderer;
    const DrawInfo before = renderer.last_draw();
    std::printf("before %u %llu %llu\n", before.action, (unsigned long long)before.counters[RAYCA_DRAW_N_BUILDS],
                (unsigned long long)before.counters[RAYCA_DRAW_N_REUSES]);
    for (const char* name : {"first", "second"}) {
      // the scene is made anew for every draw, as a host that owns no resident state would hand it over
      Scene scene;
      push_gltf_from_path(scene, argv[1]);
      scene.push_model(SoftRenderer::create_default_model());
      Image image(256, 256, ColorType::RGBA8);
      renderer.draw(scene, image);
      const DrawInfo info = renderer.last_draw();
      std::printf("%s %u %llu %llu\n", name, info.action, (unsigned long long)info.counters[RAYCA_DRAW_N_BUILDS],
                  (unsigned long long)info.counters[RAYCA_DRAW_N_REUSES]);
      dump(out + "/" + name + ".bin", image.data);
    }
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
