// denoise_scene.cpp -- the C++ host mirror's Aov() / Denoise() (include/prt_renderer.hpp) after one Tick().
// Test program only: reads a scene written by tests/helpers.py::dump_scene (textured instances, no extensions) and
// writes, as raw arrays, the average, the screen, albedo, normal_depth, the denoised average and its screen, and
// the average and screen after a second Tick (which the calls in between must not disturb).
//   usage: denoise_scene <scene.bin> <out.bin> <bounces>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "prt_renderer.hpp"

namespace {

struct Reader {
  FILE* f;
  template <class T>
  T get() {
    T v;
    if (std::fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("truncated scene file");
    return v;
  }
  template <class T>
  void arr(std::vector<T>& v, size_t n) {
    v.resize(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("truncated scene file");
  }
};

template <class T>
void put(FILE* f, const std::vector<T>& v) {
  if (std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("short write");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: denoise_scene <scene.bin> <out.bin> <bounces>\n");
    return 2;
  }
  try {
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) throw std::runtime_error("cannot open scene file");
    Reader r{fp};
    char magic[4];
    if (std::fread(magic, 1, 4, fp) != 4 || std::memcmp(magic, "PRTS", 4) != 0) throw std::runtime_error("bad magic");
    const int32_t W = r.get<int32_t>(), H = r.get<int32_t>();
    float pos[3], tgt[3];
    for (float& v : pos) v = r.get<float>();
    for (float& v : tgt) v = r.get<float>();
    const float aspect = r.get<float>();
    prt::Renderer R(W, H, 0);
    prt::Scene& S = R.scene;
    float* lw = &S.lights.point_pos[0][0];  // prt_lights is 39 consecutive floats
    for (int k = 0; k < 39; k++) lw[k] = r.get<float>();
    S.skyWidth = r.get<int32_t>();
    S.skyHeight = r.get<int32_t>();
    r.arr(S.skyPixels, 3 * (size_t)S.skyWidth * S.skyHeight);
    S.textures.resize(r.get<int32_t>());
    for (prt::Texture& t : S.textures) {
      t.width = r.get<int32_t>();
      t.height = r.get<int32_t>();
      r.arr(t.pixels, (size_t)t.width * t.height);
    }
    S.models.resize(r.get<int32_t>());
    for (prt::Model& m : S.models) {
      const int32_t T = r.get<int32_t>(), V = r.get<int32_t>();
      m.albedoTexture = r.get<int32_t>();
      m.normalTexture = r.get<int32_t>();
      m.metalnessTexture = r.get<int32_t>();
      m.emissionTexture = r.get<int32_t>();
      r.arr(m.triangles, 12 * (size_t)T);
      r.arr(m.fixedNormals, 12 * (size_t)T);
      r.arr(m.fixedTextureCoords, 6 * (size_t)T);
      r.arr(m.indices, 3 * (size_t)T);
      r.arr(m.vertices, 3 * (size_t)V);
      r.arr(m.faceNormals, 3 * (size_t)T);
    }
    S.gameobjects.resize(r.get<int32_t>());
    for (prt::GameObject& g : S.gameobjects) {
      for (float& v : g.transform) v = r.get<float>();
      g.modelIndex = r.get<uint32_t>();
    }
    std::fclose(fp);

    R.camera = prt::Camera(pos, tgt, aspect);
    R.bounces = std::atoi(argv[3]);
    R.Init();
    R.Tick();
    const std::vector<float> avg1 = R.accumulator;
    const std::vector<uint32_t> scr1 = R.screen;
    std::vector<float> albedo, normal_depth, den;
    std::vector<uint32_t> den8;
    R.Aov(albedo, normal_depth);
    prt_denoise_params p = prt::Renderer::DenoiseDefaults();
    if (p.iterations != 5 || p.normal_power != 3) throw std::runtime_error("unexpected denoiser defaults");
    R.Denoise(den, den8);
    if (R.accumulator != avg1 || R.screen != scr1) throw std::runtime_error("Denoise() changed the renderer's images");
    R.Tick();
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) throw std::runtime_error("cannot open output");
    put(fo, avg1);
    put(fo, scr1);
    put(fo, albedo);
    put(fo, normal_depth);
    put(fo, den);
    put(fo, den8);
    put(fo, R.accumulator);
    put(fo, R.screen);
    std::fclose(fo);
    std::printf("denoise_scene: %dx%d\n", W, H);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "denoise_scene: %s\n", e.what());
    return 1;
  }
  return 0;
}
