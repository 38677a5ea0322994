// variance_scene.cpp -- the C++ host mirror's TickTemporalVariance() (include/prt_renderer.hpp).
// Test program only: reads a scene written by tests/helpers.py::dump_scene (textured instances, no extensions) and a
// file of instance transforms (4 frames x instances x 16 floats), moves the camera position by (0.05, 0, 0.02) per
// call (tests/reproject_ref.py "slow"), sets frame k's transforms and writes, as raw arrays, the filtered image, its
// screen and the unfiltered history of three TickTemporalVariance() calls (clamp_k 1.5, 3 filter iterations), then of
// one more after ResetTemporal().
//   usage: variance_scene <scene.bin> <transforms.bin> <out.bin> <bounces>
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
  if (argc < 5) {
    std::fprintf(stderr, "usage: variance_scene <scene.bin> <transforms.bin> <out.bin> <bounces>\n");
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
    const size_t ninst = S.gameobjects.size();
    std::vector<float> xf;
    FILE* fx = std::fopen(argv[2], "rb");
    if (!fx) throw std::runtime_error("cannot open transforms file");
    Reader{fx}.arr(xf, 4 * ninst * 16);
    std::fclose(fx);

    R.bounces = std::atoi(argv[4]);
    R.camera = prt::Camera(pos, tgt, aspect);
    R.Init();
    prt_temporal_params p = prt::Renderer::TemporalDefaults();
    prt_denoise_variance_params q = prt::Renderer::DenoiseVarianceDefaults();
    if (p.depth_tol != 0.05f || p.normal_min != 0.9f || p.max_history != 16.0f || p.clamp_k != 0.0f ||
        p.min_temporal != 4.0f || q.iterations != 5 || q.sigma_color != 2.0f || q.color_decay != 1.0f ||
        q.variance_floor != 1e-6f)
      throw std::runtime_error("unexpected defaults");
    p.clamp_k = 1.5f;
    q.iterations = 3;
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fo) throw std::runtime_error("cannot open output");
    const float step[3] = {0.05f, 0.0f, 0.02f};
    std::vector<float> filtered, history;
    std::vector<uint32_t> screen8;
    for (int k = 0; k < 4; k++) {
      float at[3];
      for (int i = 0; i < 3; i++) at[i] = pos[i] + step[i] * (float)k;
      R.camera = prt::Camera(at, tgt, aspect);
      for (size_t g = 0; g < ninst; g++)
        std::memcpy(S.gameobjects[g].transform.data(), &xf[((size_t)k * ninst + g) * 16], 16 * sizeof(float));
      if (k == 3) R.ResetTemporal();
      R.TickTemporalVariance(filtered, screen8, history, p, q);
      put(fo, filtered);
      put(fo, screen8);
      put(fo, history);
    }
    std::fclose(fo);
    R.isPostProcessed = true;
    bool thrown = false;
    try {
      R.TickTemporalVariance(filtered, screen8, history);
    } catch (const prt::Error& e) {
      thrown = std::strstr(e.what(), "plane projection only") != nullptr;
    }
    if (!thrown) throw std::runtime_error("TickTemporalVariance() with isPostProcessed did not throw");
    std::printf("variance_scene: %dx%d\n", W, H);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "variance_scene: %s\n", e.what());
    return 1;
  }
  return 0;
}
