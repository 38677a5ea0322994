// prt_defer.hip -- the deferred resolve of the plain wavefront pipeline (no extensions, render mode 0):
// the shading form that fills one record plane per iteration and the one resolve launch per pass, both built from
// prt_shade2.h's shared pieces (shade2_body; resolve_segment, pixel_value).  Its own translation unit.
#include "prt_shade2.h"

namespace prt {

// ---- shading of P(iter) into the iteration's record plane: k_shade2<false, I0> with the throughput in the plane
template <bool I0>
__global__ void __launch_bounds__(kBlock, I0 ? 4 : 1) k_shade2d(SceneDev S, TraceArgs A, TileMap M, WaveBufs B, uint32_t iter) {
  shade2_body<false, I0, true>(S, A, M, B, iter);
}

// ---- deferred resolve (plain pipeline, no extensions, render mode 0): the pass's paths resolved once,
// after its last traversal launch, instead of by a k_res2d launch per iteration.  The shading of iteration i wrote
// its records into plane i (rinfo / ne / nb / nk / vis / T of B point at plane 0; plane i lies i * n entries on), and
// an item is shaded in consecutive iterations from 0: path 1's segments, then (kRiQueued at path 1's end) path 2's.
// A lane follows that chain through the rinfo planes to each path's last segment and walks back from there: the last
// segment's resolved value is L, every earlier one gives L = resolve_segment(record k) + L * T_k -- what resolve_item
// computes, in its order, the (result, throughput) stack never stored.  Path 1's radiance stays in registers.
// Planes behind an item's last iteration hold an earlier pass's records and are never read; an item without a pixel
// (rinfo 0 from k_wave_init, which wrote its frame entry) is skipped.
// the path whose segments are the iterations first..last (rl = rinfo of `last`), bottom-up
__device__ __forceinline__ V3 resolve_path(const SceneDev& S, const WaveBufs& B, uint32_t item, uint32_t first,
                                           uint32_t last, uint32_t rl, uint32_t fl) {
  V3 L = resolve_segment(S, B, (size_t)last * B.n + item, rl, fl);
  for (uint32_t k = last; k > first; k--) {                                                // result + Trace(..) * throughput
    const size_t e = (size_t)(k - 1u) * B.n + item;
    const V3 Rk = resolve_segment(S, B, e, B.rinfo[e], fl);
    const float4 Tk = B.T[e];
    L = Rk + L * v3(Tk.x, Tk.y, Tk.z);
  }
  return L;
}
// the last iteration of the path that starts at iteration `it` with rinfo r: its segments carry kStNeeCont up to the
// last one.  (it + 1 < iters always holds for a continuing segment; the bound keeps a damaged chain inside the planes)
__device__ __forceinline__ uint32_t path_end(const WaveBufs& B, uint32_t item, uint32_t iters, uint32_t it, uint32_t& r) {
  while (((r >> 16) & 3u) == kStNeeCont && it + 1u < iters) r = B.rinfo[(size_t)(++it) * B.n + item];
  return it;
}
// LEARN: a pass whose iteration 0 used the light-visibility record (k_res2d<true>'s part: plane 0 is S(0)'s answers)
template <bool LEARN>
__global__ void __launch_bounds__(kBlock, 8) k_resolve_pass(SceneDev S, TraceArgs A, WaveBufs B, uint32_t iters,
                                                            float4* __restrict__ out) {
  const uint32_t fl = A.flags;
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t item = blockIdx.x * kBlock + threadIdx.x; item < B.n; item += stride) {
    uint32_t r = B.rinfo[item];
    if (!(r & kRiFresh)) continue;
    if constexpr (LEARN) {
      if (r & kRiLearn) lvis_learn(B, item, r);
    }
    const uint32_t e1 = path_end(B, item, iters, 0u, r);
    const V3 L1 = resolve_path(S, B, item, 0u, e1, r, fl);
    V3 L = L1;
    if (fl & kAA) {  // path 2 starts in the iteration after path 1's end (start_path2)
      if (!(r & kRiQueued) || e1 + 1u >= iters) continue;
      r = B.rinfo[(size_t)(e1 + 1u) * B.n + item];
      const uint32_t e2 = path_end(B, item, iters, e1 + 1u, r);
      L = resolve_path(S, B, item, e1 + 1u, e2, r, fl);
    }
    const V3 res = pixel_value(L1, L, fl);
    out[item] = make_float4(res.x, res.y, res.z, B.s1[item].w);
  }
}

// the launches of a deferred pass that prt_wave2.hip's launch_wave2_iter hands over (grids as its own)
void launch_shade2d(hipStream_t s, unsigned grid, const SceneDev& S, const TraceArgs& A, const TileMap& M,
                    const WaveBufs& B, uint32_t it, bool i0) {
  if (i0) hipLaunchKernelGGL(k_shade2d<true>, dim3(grid), dim3(kBlock), 0, s, S, A, M, B, it);
  else hipLaunchKernelGGL(k_shade2d<false>, dim3(grid), dim3(kBlock), 0, s, S, A, M, B, it);
}
void launch_resolve_pass(hipStream_t s, unsigned grid, const SceneDev& S, const TraceArgs& A, const WaveBufs& B,
                         uint32_t iters, float4* out, bool learn) {
  if (learn) hipLaunchKernelGGL(k_resolve_pass<true>, dim3(grid), dim3(kBlock), 0, s, S, A, B, iters, out);
  else hipLaunchKernelGGL(k_resolve_pass<false>, dim3(grid), dim3(kBlock), 0, s, S, A, B, iters, out);
}

}  // namespace prt
