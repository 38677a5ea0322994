// instance_scene.cpp -- the C++ host mirror's instance-update calls (include/prt_renderer.hpp: Scene::UpdateInstances,
// Renderer::InstancesMoved, Renderer::TlasCost) and the three C entry points behind them.  Test program only.
//   usage: instance_scene            the refusals (no GPU needed)
//          instance_scene --render   on a GPU: 80 small grids over a floor (more than 64 instances: the rays walk the
//                                    instance BVH), scattered and handed over through Renderer::InstancesMoved, render
//                                    the frame of a second Renderer that was initialised with the scattered objects
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prt_renderer.hpp"

namespace {

constexpr int kN = 4, kW = 64, kH = 48, kObjects = 80;

// a (kN + 1) x (kN + 1) grid of vertices over [-1, 1]^2 at height 0, +y normals, two triangles per cell
prt::Model grid() {
  prt::Model m;
  for (int i = 0; i <= kN; i++)
    for (int k = 0; k <= kN; k++) {
      m.vertices.push_back(-1.0f + 2.0f * (float)i / kN);
      m.vertices.push_back(0.0f);
      m.vertices.push_back(-1.0f + 2.0f * (float)k / kN);
    }
  auto vid = [](int a, int b) { return a * (kN + 1) + b; };
  for (int a = 0; a < kN; a++)
    for (int b = 0; b < kN; b++) {
      const int t[6] = {vid(a, b), vid(a, b + 1), vid(a + 1, b), vid(a + 1, b), vid(a, b + 1), vid(a + 1, b + 1)};
      m.indices.insert(m.indices.end(), t, t + 6);
    }
  for (int32_t i : m.indices) {
    for (int c = 0; c < 3; c++) m.triangles.push_back(m.vertices[3 * (size_t)i + c]);
    m.triangles.push_back(0.0f);
    const float n[4] = {0, 1, 0, 0};
    m.fixedNormals.insert(m.fixedNormals.end(), n, n + 4);
    m.fixedTextureCoords.push_back(0.4995f * (m.vertices[3 * (size_t)i] + 1.0f));
    m.fixedTextureCoords.push_back(0.4995f * (m.vertices[3 * (size_t)i + 2] + 1.0f));
  }
  for (int p = 0; p < m.TriCount(); p++) {
    const float n[3] = {0, 1, 0};
    m.faceNormals.insert(m.faceNormals.end(), n, n + 3);
  }
  m.albedoTexture = 0;
  return m;
}

// object k of pose p: a small grid turned about y and lifted, on a spiral that pose 1 winds the other way and widens
prt::GameObject object(int k, int pose) {
  const float a = 0.37f * (float)k * (pose ? -1.3f : 1.0f) + (pose ? 0.8f : 0.0f);
  const float r = (pose ? 0.35f : 0.2f) + 0.03f * (float)k, s = 0.12f + 0.002f * (float)(k % 7);
  const float c = std::cos(a), sn = std::sin(a);
  prt::GameObject g;
  g.transform = {c * s, 0, sn * s, r * c, 0, s, 0, 0.2f + 0.01f * (float)((k * (pose ? 5 : 3)) % 40),
                 -sn * s, 0, c * s, r * sn, 0, 0, 0, 1};
  return g;
}

void fill(prt::Renderer& R, int pose) {
  prt::Texture t;
  t.width = t.height = 8;
  for (int i = 0; i < 64; i++) t.pixels.push_back(((i ^ (i >> 3)) & 1) ? 0x00E0D0C0u : 0x00405060u);
  R.scene.textures.push_back(t);
  R.scene.models.push_back(grid());
  prt::GameObject floor;
  floor.transform = {4, 0, 0, 0, 0, 1, 0, 0, 0, 0, 4, 0, 0, 0, 0, 1};
  R.scene.gameobjects.push_back(floor);
  for (int k = 0; k < kObjects; k++) R.scene.gameobjects.push_back(object(k, pose));
  const float lp[4][3] = {{2, 3, 1}, {-2, 3, -1}, {0, 4, 0}, {1, 2, -2}};
  for (int i = 0; i < 4; i++)
    for (int c = 0; c < 3; c++) {
      R.scene.lights.point_pos[i][c] = lp[i][c];
      R.scene.lights.point_color[i][c] = 6.0f;
    }
  const float pos[3] = {0.5f, 3.0f, -4.5f}, target[3] = {0, 0.3f, 0};
  R.camera = prt::Camera(pos, target, (float)kW / (float)kH);
  R.bounces = 2;
}

int render() {
  prt::Renderer A(kW, kH, 0), B(kW, kH, 0);
  fill(A, 0);
  fill(B, 1);
  A.Init();
  B.Init();
  A.Tick();
  const std::vector<float> before = A.accumulator;
  const double built = A.TlasCost();
  for (int k = 0; k < kObjects; k++) A.scene.gameobjects[1 + (size_t)k] = object(k, 1);
  A.InstancesMoved();
  A.Tick();
  B.Tick();  // (the frame counter seeds the paths: B's second frame is the one A's second frame must equal)
  prt::check(prt_reset_accumulation(B.Context(), 1));
  B.Tick();
  if (A.accumulator == before) {
    std::fprintf(stderr, "instance_scene: the motion does not show\n");
    return 1;
  }
  if (std::memcmp(A.accumulator.data(), B.accumulator.data(), A.accumulator.size() * sizeof(float)) != 0 ||
      A.screen != B.screen) {
    std::fprintf(stderr, "instance_scene: InstancesMoved and a fresh Init render different frames\n");
    return 1;
  }
  const double refit = A.TlasCost(), fresh = B.TlasCost();
  if (!(built > 0.0) || !(refit > 0.0) || !(fresh > 0.0) || refit != A.TlasCost()) {
    std::fprintf(stderr, "instance_scene: TlasCost built %g refitted %g fresh %g\n", built, refit, fresh);
    return 1;
  }
  std::printf("instance_scene: render ok (TlasCost built %.6g, refitted %.6g, fresh %.6g)\n", built, refit, fresh);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--render") == 0) {
    try {
      return render();
    } catch (const std::exception& e) {
      std::fprintf(stderr, "instance_scene: %s\n", e.what());
      return 1;
    }
  }
  int bad = 0;
  const float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double cost = 7.0;
  uint64_t nb = 5, sb = 6;
  bad += prt_update_instances(nullptr, T, 1, 0u) != PRT_ERR_INVALID_ARGUMENT;
  bad += prt_update_instances(nullptr, nullptr, 1, PRT_IN_DEVICE) != PRT_ERR_INVALID_ARGUMENT;
  bad += prt_tlas_cost(nullptr, &cost) != PRT_ERR_INVALID_ARGUMENT || cost != 7.0;
  bad += prt_read_tlas(nullptr, nullptr, 0, nullptr, 0, &nb, &sb) != PRT_ERR_INVALID_ARGUMENT || nb != 5 || sb != 6;
  if (bad) {
    std::fprintf(stderr, "instance_scene: %d unexpected answers\n", bad);
    return 1;
  }
  std::printf("instance_scene: ok\n");
  return 0;
}
