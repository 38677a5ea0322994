// deform_check.cpp -- the C++ host mirror's deforming-mesh calls (include/prt_renderer.hpp: Renderer::TrackModel,
// TickTemporalVariance(..., deform = true)) and the three C entry points behind them.  Test program only: it links
// against the calls, and without a device checks what they answer before a context is used.
//   usage: deform_check            the refusals (no GPU needed)
//          deform_check --mirror   never run by the tests: keeps the mirror's member functions instantiated
#include <cstdio>
#include <cstring>
#include <vector>

#include "prt_renderer.hpp"

namespace {

// every new member of the mirror, so that the program fails to compile or link if one is missing
void mirror(prt::Renderer& R) {
  std::vector<float> filtered, history;
  std::vector<uint32_t> screen8;
  R.TrackModel(0);
  R.ModelChanged(0);
  R.TickTemporalVariance(filtered, screen8, history, prt::Renderer::TemporalDefaults(),
                         prt::Renderer::DenoiseVarianceDefaults(), true);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--mirror") == 0) {
    try {
      prt::Renderer R(64, 48, 0);
      mirror(R);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "deform_check: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  int bad = 0;
  float img[16 * 4] = {};
  uint32_t ids[16] = {};
  const float xf[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float motion[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  prt_temporal_params p{};
  prt_camera cam{};
  bad += prt_temporal_defaults(&p) != PRT_OK;
  bad += prt_snapshot_mesh(nullptr, 0) != PRT_ERR_INVALID_ARGUMENT;
  bad += prt_render_aov_deform(nullptr, 4, 4, 0u, img, img, ids, img, 0u) != PRT_ERR_INVALID_ARGUMENT;
  bad += prt_reproject_deform(nullptr, &p, 4, 4, &cam, img, img, ids, &cam, img, img, ids, motion, 1, img, img, xf, img,
                              img, nullptr, 0u) != PRT_ERR_INVALID_ARGUMENT;
  if (bad) {
    std::fprintf(stderr, "deform_check: %d unexpected answers\n", bad);
    return 1;
  }
  std::printf("deform_check: ok\n");
  return 0;
}
