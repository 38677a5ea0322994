"""The three wavefront pipelines without extensions, at the same settings: the per-iteration plain chain (PRT_MERGE=0
PRT_DEFER_RESOLVE=0), the deferred one (PRT_MERGE=0) and the merged one (PRT_MERGE=1).  Their kernels shade a segment
with the same shade_miss / shade_hit and resolve it with the same resolve_segment (prt_shade2.h), each around its own
record layout, throughput index and ray source, so every call must give the same bits in all three: the average image
(uint32 views: NaN payloads included), the RGB8 frame, and (segments, shadow_rays).  The other modules hold the
pipelines to each other pairwise, in different files and at different settings.

The "small" scene at 70x45 (neither a multiple of the 8x8 tile: padding entries), 4 spp, AA on (the merged pipeline
needs it).  Three calls per context on a static camera: the dense pass, the pass that learns the light-visibility
record, and a pass answered from it (the I0 / LEARN forms of every pipeline).  prt_stats tells the chains apart:
pipeline 3 is the deferred one, and the merged one needs one traversal launch fewer than the plain ones."""
import functools

import numpy as np
import pytest

from helpers import gpu_scene
from prt import _lib, scenes
from wave_env import contexts, env_or_unset

pytestmark = pytest.mark.gpu

W, H, SPP, CALLS = 70, 45, 4, 3
# name -> (switches, prt_stats.pipeline, traversal launches per call at `bounces` with AA)
PIPELINES = {
    "plain": (dict(PRT_MERGE="0", PRT_DEFER_RESOLVE="0"), 2, lambda b: 2 * b + 1),
    "deferred": (dict(PRT_MERGE="0", PRT_DEFER_RESOLVE=None), 3, lambda b: 2 * b + 1),
    "merged": (dict(PRT_MERGE="1", PRT_DEFER_RESOLVE=None), 2, lambda b: 2 * b),
}


@functools.lru_cache(maxsize=None)
def _scene():
    return scenes.config_small()


@pytest.mark.parametrize("skybox", [True, False], ids=["sky", "nosky"])
@pytest.mark.parametrize("gamma", [True, False], ids=["gamma", "linear"])
@pytest.mark.parametrize("bounces", [1, 2, 4])
def test_three_pipelines_same_bits(monkeypatch, bounces, gamma, skybox):
    sd = _scene()
    flags = _lib.FLAGS_DEFAULT & ~(_lib.FLAG_GAMMA | _lib.FLAG_SKYBOX)
    flags |= (_lib.FLAG_GAMMA if gamma else 0) | (_lib.FLAG_SKYBOX if skybox else 0)
    assert flags & _lib.FLAG_AA
    res = {}
    with contexts(len(PIPELINES)) as cs:
        for c, (name, (switches, pipeline, launches)) in zip(cs, PIPELINES.items()):
            gpu_scene(c, sd, W, H)
            calls = []
            with env_or_unset(monkeypatch, **switches):
                for k in range(CALLS):
                    avg, rgb8, st = c.render(W, H, SPP, bounces, flags=flags, frame_index=2 * k)
                    assert (st.pipeline, st.iterations) == (pipeline, launches(bounces)), (name, k)
                    calls.append((avg, rgb8, (st.segments, st.shadow_rays)))
            res[name] = (calls, c.ray_totals(), c.shadow_reuse())
    # the third call took answers from the record (in every pipeline alike), so the I0 forms ran
    assert res["plain"][2] > 0
    want = res["plain"]
    for name in ("deferred", "merged"):
        got = res[name]
        for k in range(CALLS):
            assert np.array_equal(got[0][k][0].view(np.uint32), want[0][k][0].view(np.uint32)), (name, k, "avg")
            assert np.array_equal(got[0][k][1], want[0][k][1]), (name, k, "rgb8")
            assert got[0][k][2] == want[0][k][2], (name, k, "rays")
        assert got[1] == want[1] and got[2] == want[2], name
