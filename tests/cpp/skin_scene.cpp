// skin_scene.cpp -- the C++ host mirror's skinning calls (include/prt_renderer.hpp: Scene::SetSkin, Renderer::SetSkin,
// Renderer::SkinModel) and the two C entry points behind them.  Test program only.
//   usage: skin_scene            the refusals (no GPU needed)
//          skin_scene --render   on a GPU: a 12 x 9 grid over a floor, bound to two joints and posed through
//                                Renderer::SkinModel, renders the frame that a second Renderer renders after
//                                ModelChanged with the arrays skin_mesh_host() (csrc/prt_skin.h) derives on the host
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prt_renderer.hpp"
#include "prt_skin.h"

namespace {

constexpr int kNX = 12, kNZ = 9, kW = 64, kH = 48;

// a (kNX + 1) x (kNZ + 1) grid of vertices over [-1, 1]^2 at height y, +y normals, two triangles per cell
prt::Model grid(float y) {
  prt::Model m;
  for (int i = 0; i <= kNX; i++)
    for (int k = 0; k <= kNZ; k++) {
      m.vertices.push_back(-1.0f + 2.0f * (float)i / kNX);
      m.vertices.push_back(y);
      m.vertices.push_back(-1.0f + 2.0f * (float)k / kNZ);
    }
  auto vid = [](int a, int b) { return a * (kNZ + 1) + b; };
  for (int a = 0; a < kNX; a++)
    for (int b = 0; b < kNZ; b++) {
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

void fill(prt::Renderer& R) {
  prt::Texture t;
  t.width = t.height = 8;
  for (int i = 0; i < 64; i++) t.pixels.push_back(((i ^ (i >> 3)) & 1) ? 0x00E0D0C0u : 0x00405060u);
  R.scene.textures.push_back(t);
  R.scene.models.push_back(grid(0.0f));   // the floor
  R.scene.models.push_back(grid(0.5f));   // the skinned sheet
  prt::GameObject a, b;
  a.transform = {3, 0, 0, 0, 0, 1, 0, 0, 0, 0, 3, 0, 0, 0, 0, 1};
  b.modelIndex = 1;
  R.scene.gameobjects = {a, b};
  const float lp[4][3] = {{2, 3, 1}, {-2, 3, -1}, {0, 4, 0}, {1, 2, -2}};
  for (int i = 0; i < 4; i++)
    for (int c = 0; c < 3; c++) {
      R.scene.lights.point_pos[i][c] = lp[i][c];
      R.scene.lights.point_color[i][c] = 6.0f;
    }
  const float pos[3] = {0.5f, 2.5f, -3.5f}, target[3] = {0, 0.3f, 0};
  R.camera = prt::Camera(pos, target, (float)kW / (float)kH);
  R.bounces = 3;
}

int render() {
  prt::Renderer A(kW, kH, 0), B(kW, kH, 0);
  fill(A);
  fill(B);
  A.Init();
  B.Init();
  const prt::Model& sheet = A.scene.models[1];
  const size_t V = sheet.vertices.size() / 3, T = (size_t)sheet.TriCount();
  prt::Skin skin;
  skin.jointCount = 2;
  skin.positions = sheet.vertices;
  for (size_t v = 0; v < V; v++) {
    const float n[3] = {0, 1, 0};
    skin.normals.insert(skin.normals.end(), n, n + 3);
    const float w = 0.5f * (sheet.vertices[3 * v] + 1.0f);  // joint 1 takes over along x
    const uint16_t j[4] = {0, 1, 0, 0};
    const float ws[4] = {1.0f - w, w, 0.0f, 0.0f};
    skin.joints.insert(skin.joints.end(), j, j + 4);
    skin.weights.insert(skin.weights.end(), ws, ws + 4);
  }
  const float c = std::cos(0.7f), s = std::sin(0.7f);
  const float M[24] = {1, 0, 0, 0, 0, 1, 0, 0.1f, 0, 0, 1, 0,          // joint 0: lifted a little
                       c, -s, 0, 0.2f, s, c, 0, 0.4f, 0, 0, 1.2f, 0};  // joint 1: turned about z, stretched along z
  A.Tick();
  A.SetSkin(1, skin);
  A.SkinModel(1, M, 2);
  A.Tick();
  // the same pose derived on the host and handed over as arrays
  prt::Model& m = B.scene.models[1];
  std::vector<float> tmp(3 * V);
  prt::skin_mesh_host((int32_t)V, (int32_t)T, skin.positions.data(), skin.normals.data(), sheet.indices.data(),
                      skin.joints.data(), skin.weights.data(), M, m.triangles.data(), m.fixedNormals.data(),
                      m.vertices.data(), m.faceNormals.data(), tmp.data());
  B.Tick();
  const std::vector<float> bind = B.accumulator;
  B.ModelChanged(1);
  B.Tick();
  if (A.accumulator == bind) {
    std::fprintf(stderr, "skin_scene: the pose does not show\n");
    return 1;
  }
  if (std::memcmp(A.accumulator.data(), B.accumulator.data(), A.accumulator.size() * sizeof(float)) != 0 ||
      A.screen != B.screen) {
    std::fprintf(stderr, "skin_scene: SkinModel and ModelChanged render different frames\n");
    return 1;
  }
  // Upload binds the kept skin again (prt_set_meshes discarded it): the bind pose, then the same pose, the same frame
  A.Init();
  A.SkinModel(1, M, 2);
  A.Tick();
  B.Init();
  B.Tick();
  if (std::memcmp(A.accumulator.data(), B.accumulator.data(), A.accumulator.size() * sizeof(float)) != 0) {
    std::fprintf(stderr, "skin_scene: after Init the kept skin renders another frame\n");
    return 1;
  }
  A.scene.RemoveSkin(nullptr, 1);
  std::printf("skin_scene: render ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--render") == 0) {
    try {
      return render();
    } catch (const std::exception& e) {
      std::fprintf(stderr, "skin_scene: %s\n", e.what());
      return 1;
    }
  }
  int bad = 0;
  const float M[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  prt_skin k{};
  bad += prt_set_mesh_skin(nullptr, 0, &k) != PRT_ERR_INVALID_ARGUMENT;
  bad += prt_set_mesh_skin(nullptr, 0, nullptr) != PRT_ERR_INVALID_ARGUMENT;
  bad += prt_skin_mesh(nullptr, 0, M, 1, 0u) != PRT_ERR_INVALID_ARGUMENT;
  bad += prt_skin_mesh(nullptr, 0, nullptr, 1, PRT_IN_DEVICE) != PRT_ERR_INVALID_ARGUMENT;
  prt::Scene sc;  // the scene keeps a skin without a context
  sc.SetSkin(nullptr, 0, prt::Skin{});
  bad += sc.skins.size() != 1;
  sc.RemoveSkin(nullptr, 0);
  bad += !sc.skins.empty();
  if (bad) {
    std::fprintf(stderr, "skin_scene: %d unexpected answers\n", bad);
    return 1;
  }
  std::printf("skin_scene: ok\n");
  return 0;
}
