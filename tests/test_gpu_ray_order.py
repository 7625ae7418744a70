"""GPU: the direction buffer kept across launches and the ray pool handed out longest ray first
(arx_debug_set_ray_order, include/arx.h) leave every result as it was.

A ray's direction is a function of (seed, ray id) and the int64 histogram and the counters do not
depend on the order rays run in, so mode 1 (directions kept; a measuring launch, a device sort of the
pool's slots, then launches on the sorted buffer), mode 0 (kept, ray order) and mode 2 (directions
re-made by every launch: the behaviour before the cache) must agree bit for bit -- through the
measuring frame, the first sorted frame and the ones after it, through every change of the order's
key, and through a listener move, which is deliberately not in the key.

Pool shape: 600 000 rays x 8 bounces at 16 kHz on the conference stand-in, the shape of
test_gpu_frames.py::test_ray_pool_launches_share_the_grid_in_flight -- the smallest that takes the
pool on 256 CUs (96 rays x 5120 waves = 491 520).  Small shape: 36 000 rays, no pool.
"""
import ctypes as C

import numpy as np
import pytest

from audiorenderingv2_amd import AudioRenderer, RenderSettings, debug_ray_directions, receiver_local
from audiorenderingv2_amd._lib import check, lib
from audiorenderingv2_amd.scene import CONFERENCE_EMITTER, CONFERENCE_LISTENER

pytestmark = pytest.mark.gpu

POOL = (100, 100, 60)
SMALL = (60, 60, 10)
S = dict(sample_rate=16000, base_power=3.62, max_bounces=8, hrtf_absorption_rate=0.5)
MOVED = ((1.0, 1.2, -0.5), 30.0)


def make(conference, rays, mode, fif=1):
    r = AudioRenderer(RenderSettings(**dict(S, rays=rays)), scene=conference, receiver=receiver_local())
    r.set_ray_order(mode)
    r.set_frames_in_flight(fif)
    r.setEmitterPosInOptix(CONFERENCE_EMITTER)
    r.setSphereCenterInOptix(CONFERENCE_LISTENER, 0.0)
    return r


def result(r):
    """The last frame: both IR channels' bits and (queries, receiver hits, misses)."""
    L, R = r.get_ir()
    st = r.stats()
    return L.view(np.uint32), R.view(np.uint32), (st["queries"], st["receiver_hits"], st["misses"])


def frame(r, sub=None):
    if sub is None:
        r.render()
    else:
        r.clear_histogram()
        r.trace_rays(*sub)
        r.finalize_ir()
    return result(r)


def same(a, b, what):
    assert a[2] == b[2], (what, a[2], b[2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


@pytest.mark.parametrize("fif", [1, 2])
def test_sorted_pool_frames_are_bit_identical(conference, fif):
    """Mode 1: the measuring frame, the first sorted frame and two more per frame set, against one
    mode-2 render.  With two frames in flight each frame set measures and sorts on its own."""
    ref = make(conference, POOL, 2)
    r = make(conference, POOL, 1, fif)
    try:
        want = frame(ref)
        assert want[0].any() and want[2][1] > 0
        for k in range(4 * fif):
            same(frame(r), want, f"mode 1 frame {k}")
            buf = r.ray_order_buffer(0)
            assert buf["sorted"] and 0 < buf["n_static"] < 600_000, (k, buf["sorted"], buf["n_static"])
        assert not ref.ray_order_buffer(0)["sorted"]
    finally:
        r.close()
        ref.close()


def test_every_key_change_measures_again(conference):
    """Between mode-1 frames: the emitter moves, the scene is set again, a trace_rays sub-range (another
    first ray and count), the count grown past the buffer (it reallocates).  Each next frame, and the
    sorted frame after it, equals a mode-2 renderer's with the same settings (mode 2 keeps nothing
    from launch to launch, so one such renderer serves every step)."""
    ref = make(conference, POOL, 2)
    r = make(conference, POOL, 1)
    try:
        # sub-ranges first, so the full launch at the end outgrows the direction buffer
        steps = [("sub-range", None, (0, 500_000)),
                 ("other first ray", None, (100_000, 600_000)),
                 ("emitter", lambda x: x.setEmitterPosInOptix((-4.0, 1.5, 1.0)), (100_000, 600_000)),
                 ("scene set again", lambda x: x.set_scene(conference), (100_000, 600_000)),
                 ("count grown", None, None)]
        seen = []
        for what, change, sub in steps:
            for x in (r, ref):
                if change:
                    change(x)
            want = frame(ref, sub)
            assert want[0].any()
            same(frame(r, sub), want, what + ": measuring frame")
            assert r.ray_order_buffer(0)["sorted"]
            same(frame(r, sub), want, what + ": sorted frame")
            seen.append(want)
        # the steps differ from each other, so a stale frame could not pass for the next
        for i, j in [(0, 1), (1, 2), (3, 4)]:
            assert not np.array_equal(seen[i][0], seen[j][0]), (i, j)
    finally:
        r.close()
        ref.close()


def test_listener_is_not_in_the_key(conference):
    """A listener move keeps the sorted buffer (no new measuring launch) and the frame at the new
    position equals mode 2's there."""
    ref = make(conference, POOL, 2)
    r = make(conference, POOL, 1)
    try:
        frame(r)
        frame(r)
        before = r.ray_order_buffer(600_000)["dirs"].copy()
        for x in (r, ref):
            x.setSphereCenterInOptix(*MOVED)
        want = frame(ref)
        got = frame(r)
        same(got, want, "after the move")
        assert want[0].any()
        # the scatter's order inside a cost bin is not repeatable, so an untouched buffer means no new sort
        assert np.array_equal(r.ray_order_buffer(600_000)["dirs"], before)
    finally:
        r.close()
        ref.close()


def test_small_launches_keep_directions_and_sort_nothing(conference):
    ref = make(conference, SMALL, 2)
    try:
        want = frame(ref)
        assert want[0].any() and want[2][1] > 0
        for mode in (1, 0):
            r = make(conference, SMALL, mode)
            try:
                for k in range(3):
                    same(frame(r), want, f"mode {mode} frame {k}")
                buf = r.ray_order_buffer(36_000)
                assert not buf["sorted"] and buf["n_static"] == 36_000 and buf["first_ray"] == 0
                assert np.array_equal(buf["dirs"][:, :3], debug_ray_directions(1, 0, 36_000))
            finally:
                r.close()
    finally:
        ref.close()


def test_sorted_buffer_is_a_permutation(conference):
    """The sorted buffer read back: slots below n_static untouched, the pool's slots a permutation of
    theirs (equal as multisets of directions); mode 0 on the same renderer puts ray order back."""
    r = make(conference, POOL, 1)
    try:
        frame(r)
        n = 600_000
        buf = r.ray_order_buffer(n)
        ns = buf["n_static"]
        assert buf["sorted"] and buf["first_ray"] == 0
        n_static, share = C.c_uint64(), C.c_uint32()
        check(lib().arx_debug_ray_order_host(n, 0, 0, None, None, C.byref(share)))
        check(lib().arx_debug_ray_order_host(n, share.value, 0, C.byref(n_static), None, None))
        assert ns == n_static.value == n - ((n * share.value) >> 8)  # the kernel's own split
        want = debug_ray_directions(1, 0, n)
        got = buf["dirs"]
        assert not got[:, 3].any()
        assert np.array_equal(got[:ns, :3], want[:ns])
        assert not np.array_equal(got[ns:, :3], want[ns:])  # it did move something

        def rows(a):
            v = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 3)
            return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]

        assert np.array_equal(rows(got[ns:, :3]), rows(want[ns:]))
        sorted_frame = frame(r)
        r.set_ray_order(0)
        same(frame(r), sorted_frame, "mode 0 after mode 1")
        buf = r.ray_order_buffer(n)
        assert not buf["sorted"] and np.array_equal(buf["dirs"][:, :3], want)
    finally:
        r.close()
