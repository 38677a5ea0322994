// prt_surface.hip -- the primary-surface record of the plain wavefront pipeline: the shading forms of
// iteration 0 that fill it and that shade from it, both built from prt_shade2.h's shade2_body.  Its own translation
// unit, so the kernels of every other launch keep their machine code.
//
// Path 1 of a pixel starts at the pixel centre, so while the primary hits are reused (WaveBufs::phit) everything the
// shading of iteration 0 reads before its first random draw repeats frame after frame: the 96-byte ShadeTri gather, the
// instance / mesh / texture descriptors, three texel gathers and three sRGB lookups, the TBN and the normal transform,
// the hit point, and for a miss the sky lookup with its double-precision atan2 / acos.  The record (SurfBufs,
// prt_launch.h; the entry's layout: prt_shade2.h surf_store) keeps the results per tile-map entry, indexed
// (base + item) % pitems like phit and lvis, in three planes of 16-byte words (48 bytes an entry) and a fourth for the
// emission of the meshes that have an emission texture.
//   k_shade2s<DEFER, kSurfFill>  iteration 0 of a kPrimReuse pass whose record is stale: k_shade2<false, true> /
//                                k_shade2d<true>, which also stores what hit_attributes / miss_radiance just gave
//                                it.  Plain stores; two frames of a pixel store the same values (as lvis_learn)
//   k_shade2s<DEFER, kSurfRead>  ... whose record is valid: the prefetch loads the entry's words in index order and
//                                the item is shaded from them by the same shade_hit, entered behind the attributes;
//                                phit, stri, texels, srgb, sky and the descriptors are never touched, and of the ray
//                                only the direction is read
//   k_shade2s<true, kSurfInit>   the read form of a deferred pass with no k_wave_init in front of it (shade2_body): it
//                                walks the items by index and computes seed, jitter and the primary ray's direction
//                                itself -- each a pure function of the pixel and the frame index -- so the 72 bytes
//                                per item that k_wave_init writes and iteration 0 reads straight back are never moved.
//                                PRT_INIT_FOLD=0 keeps k_wave_init and the plain read form
// Every random draw, nk, nb, vis, T, the next ray, seed and rinfo are what the other forms write: the rest of shade_hit
// runs on the same bits.  Both forms store hp only for the items that queue a shadow ray.
// Writer: the fill form; readers: the read form of a later pass or call on the same wavefront state, ordered by the
// state's stream; the host stamps the record once the filling pass is enqueued (prt_api_render.cpp) and keys it on the
// primary hits' generation, the context's shading epoch and the call's normal-map and skybox flags.
#include "prt_shade2.h"

namespace prt {

template <bool DEFER, int SURF>
__global__ void __launch_bounds__(kBlock, 4) k_shade2s(SceneDev S, TraceArgs A, TileMap M, WaveBufs B, uint32_t iter,
                                                       SurfBufs R, float4* __restrict__ out) {
  shade2_body<false, true, DEFER, SURF>(S, A, M, B, iter, R, out);
}

void launch_shade2s(hipStream_t s, unsigned grid, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                    const WaveBufs& B, uint32_t it, bool defer, int surf, const SurfBufs& R, float4* out) {
#define PRT_LAUNCH(D, F) hipLaunchKernelGGL((k_shade2s<D, F>), dim3(grid), dim3(kBlock), 0, s, S, A, M, B, it, R, out)
  if (defer) {
    if (surf == kSurfInit) PRT_LAUNCH(true, kSurfInit);
    else if (surf == kSurfRead) PRT_LAUNCH(true, kSurfRead);
    else PRT_LAUNCH(true, kSurfFill);
  } else {
    if (surf == kSurfRead) PRT_LAUNCH(false, kSurfRead);
    else PRT_LAUNCH(false, kSurfFill);
  }
#undef PRT_LAUNCH
}

}  // namespace prt
