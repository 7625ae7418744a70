"""GPU: the candidate kernel whose blocks find their parts of the list from the heads (replay_cand_kernel,
csrc/arx_replay.hip; the numbering: csrc/arx_cand_plan.hpp) leaves every result as it was.  (The file's name is
from the kernel these cases were first written for, a lane per candidate query; it was measured slower and not
kept)

The reference in every case is a renderer with the path cache off and the same settings, as in
tests/test_gpu_path_filter.py, whose helpers and scenes these tests share.  "Equal" means both IR channels'
bits and the (queries, receiver hits, misses) counters.  Every case asserts from path_filter_state(candidates=True)
that the frame it compares was a filtered replay with the candidates the case is about, so it cannot pass
without running the kernel.  A reference frame is made once per listener position.
"""
import numpy as np
import pytest

from audiorenderingv2_amd.scene import Scene
from test_gpu_path_filter import box_scene, frame, make, same, state

pytestmark = pytest.mark.gpu

EMITTER = (-1.5, 1.2, 0.0)
NEAR = ((1.5, 1.2, 0.3), 0.0)     # 3 m from the emitter: the emitter is outside the receiver's grown box
MOVED = ((0.9, 1.7, -0.8), 75.0)  # 2.6 m
# The receiver behind the room's z = 2 wall but for a cap a few centimetres high: few rays end on it, while
# every segment that ends on the wall in front of it crosses its box.
IN_THE_WALL = ((1.0, 1.2, 2.95), 0.0)


def run_case(scene, rays, fif, stops, frames, check, **over):
    """A cached renderer against a cache-off one at every stop: fif + 2 frames at the first (each frame set
    traces once, one launch records, the next replays), then `frames` at every stop, each of them a filtered
    replay that `check(info, want, n)` accepts."""
    n = rays[0] * rays[1] * rays[2]
    ref = make(scene, rays, False, emitter=EMITTER, listener=stops[0], **over)
    r = make(scene, rays, True, fif, emitter=EMITTER, listener=stops[0], **over)
    try:
        want = frame(ref)
        for k in range(fif + 2):
            same(frame(r), want, f"warm-up frame {k}")
        assert state(r) == "replayed"
        for stop in stops:
            for x in (ref, r):
                x.setSphereCenterInOptix(*stop)
            want = frame(ref)
            for k in range(frames):
                got = frame(r)
                info = r.path_filter_state(candidates=True)
                print(stop, k, "reference", want[2], "filter", info)
                assert state(r) == "replayed" and info["filtered"], (stop, k, state(r), info)
                check(info, want[2], n)
                same(got, want, (stop, k))
    finally:
        r.close()
        ref.close()


def many_bounces(info, ref, n):
    # more than 64 candidates in a 1024-slot stretch is certain with more than 256 among 4 096 rays: a second
    # part exists, and its rays' chains are several queries long
    assert info["candidate_rays"] > 256, info
    assert info["candidate_queries"] >= 3 * info["candidate_rays"], info
    assert 0 < ref[1] < info["candidate_rays"], (ref, info)  # rays that are queried and never shaded


@pytest.mark.parametrize("fif,frames", [(1, 2), (2, 4)], ids=["one-frame", "two-in-flight"])
def test_many_candidate_bounces_per_ray(fif, frames):
    """4 096 rays x 32 bounces in the closed box: candidate rays with several candidate bounces each, several
    parts per stretch.  Two listener positions; once more with two frames in flight."""
    stops = [NEAR, MOVED] if fif == 1 else [NEAR]
    run_case(box_scene(False), (16, 16, 16), fif, stops, frames, many_bounces, max_bounces=32)


def test_more_parts_than_blocks():
    """266 240 rays x 8 in the box, where nearly every ray is a candidate: more than 2 048 x 64 candidate rays
    are more parts than the launch has blocks, so blocks take several parts; 260 stretches are two tiles of heads."""
    def check(info, ref, n):
        assert info["candidate_rays"] > 2048 * 64, info
        assert ref[1] > 0, ref

    run_case(box_scene(False), (65, 64, 64), 1, [NEAR], 2, check)


def test_bit_63():
    """64 bounces, walls that absorb 2 %: most rays run all 64 queries, so masks reach their top bit."""
    box = box_scene(False)
    scene = Scene(box.tri_v, np.full(12, 0.02, np.float32), box.names)

    def check(info, ref, n):
        assert ref[0] > 48 * n, (ref, n)
        assert info["candidate_queries"] > info["candidate_rays"] > 0, info

    run_case(scene, (16, 8, 8), 1, [IN_THE_WALL], 2, check, max_bounces=64)


def test_ragged_sizes():
    """2 431 rays: no multiple of 64 or of 1 024, so the last stretch is partly filled -- and holds candidates."""
    def check(info, ref, n):
        assert n == 2431 and ref[1] > 0, (n, ref)
        assert info["candidate_rays"] >= ref[1], (info, ref)

    run_case(box_scene(False), (17, 13, 11), 1, [NEAR, MOVED], 2, check)


def test_a_ray_that_ends_on_a_flagged_last_query():
    """The marked box: a ray that ends on a receiver-marked triangle of the scene's own is shaded in the
    finish from its flagged last query, not from a receiver hit of the query."""
    def check(info, ref, n):
        assert ref[1] > 0, ref
        assert info["candidate_rays"] >= ref[1], (info, ref)

    run_case(box_scene(True), (16, 16, 16), 1, [NEAR, MOVED], 2, check)
