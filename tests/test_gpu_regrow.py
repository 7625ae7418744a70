"""GPU: a buffer that is in use, is too small and is replaced gives the bits of a buffer made at that size.

Each case makes a call at a small size and then at a larger one on ONE renderer, and compares the second
result, bit for bit, with the same call on a fresh renderer: IRs, the (queries, receiver hits, misses)
counters and the analyses where the call has them.  The scene is the closed 12-triangle box of the band and
listener tests with 16 x 16 x 16 rays and a 1 s IR at 1 kHz.
"""
import struct

import numpy as np
import pytest

from audiorenderingv2_amd import AudioRenderer, RenderGroup, RenderSettings, cardioid_cube, receiver_local
from audiorenderingv2_amd.scene import Scene, _box_tris

pytestmark = pytest.mark.gpu

RAYS = (16, 16, 16)
SR = 1000
S = dict(rays=RAYS, sample_rate=SR, ir_length_in_seconds=1, base_power=3.62, max_bounces=8, hrtf_absorption_rate=0.5)
EMITTER = (-1.5, 1.2, 0.0)
HOME = ((1.5, 1.2, 0.3), 0.0)
POSES = [HOME, ((0.8, 1.6, -0.7), 120.0), ((1.8, 1.3, -0.5), 45.0), ((1.0, 1.5, 0.8), 270.0), ((0.0, 1.4, 0.8), 200.0),
         ((2.0, 1.0, 1.0), 10.0), ((0.5, 2.0, -1.2), 300.0), ((1.2, 0.9, -0.2), 75.0), ((2.2, 1.8, 0.0), 180.0)]
COUNTERS = ("queries", "receiver_hits", "misses")


def arr(poses):
    return np.array([[*p, yaw] for p, yaw in poses], np.float32)


def band_table(n_bands):
    return np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.9, (n_bands, 12)).astype(np.float32)


def box(absorption):
    walls = _box_tris(np.array([[-3.0, 0.0, -2.0]], np.float32), np.array([[3.0, 3.0, 2.0]], np.float32))
    return Scene(walls, np.asarray(absorption, np.float32), ["wall"] * 12)


def fresh(table=None):
    """A renderer on the box; with a table, the scene carries the eight-band table's column minimum, which
    every narrower table of the same generator is at least."""
    scene = box(np.full(12, 0.25, np.float32) if table is None else band_table(8).min(axis=0))
    r = AudioRenderer(RenderSettings(**S), scene=scene, receiver=receiver_local())
    r.setEmitterPosInOptix(EMITTER)
    r.setSphereCenterInOptix(*HOME)
    if table is not None:
        r.set_band_absorption(table)
    return r


def plain(v):
    """Anything a call returns, as values that compare by their bits (a NaN by its bits, an array by its bytes)."""
    if isinstance(v, float):
        return struct.pack("<d", v)
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, dict):
        return tuple((k, plain(x)) for k, x in sorted(v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(plain(x) for x in v)
    if isinstance(v, (set, frozenset)):
        return tuple(sorted(v))
    return v


def counters(stats):
    return [tuple(int(x) for x in stats[k].reshape(-1)) for k in COUNTERS]


def batch(out):
    """What a band or listener call computed: IRs, counters, analyses, the broadband set."""
    assert out["ir"][0].any() and sum(counters(out["stats"])[1]) > 0
    return plain((out["ir"], counters(out["stats"]), out["acoustics"], out.get("broadband")))


def frame(r):
    """One frame at the renderer's listener: IR, counters, the three analyses."""
    r.render()
    r.analyze_ir()
    st = r.stats()
    assert st["receiver_hits"] > 0
    return plain((r.get_ir(), [st[k] for k in COUNTERS], [r.acoustics(ch) for ch in ("left", "right", "sum")]))


def test_band_table_and_scratch():
    """4 bands, then 8 on the same scene: the table and the band scratch grow."""
    r, f = fresh(band_table(4)), fresh(band_table(8))
    try:
        small = batch(r.render_bands(irs=True))
        r.set_band_absorption(band_table(8))
        got = batch(r.render_bands(irs=True))
        assert got == batch(f.render_bands(irs=True)) and got != small
    finally:
        r.close()
        f.close()


def test_listener_chunk_pinned_block_and_tree_arrays():
    """2 poses, then 9 at a forced chunk of 8: the chunk scratch, the pinned block and the widened tree arrays
    grow; then a frame of the renderer's own at its listener."""
    r, f = fresh(), fresh()
    try:
        batch(r.render_listeners(arr(POSES[:2]), irs=True))
        for x in (r, f):
            x.set_listener_chunk(8)
        assert batch(r.render_listeners(arr(POSES), irs=True)) == batch(f.render_listeners(arr(POSES), irs=True))
        assert frame(r) == frame(f)
    finally:
        r.close()
        f.close()


def filters(n_bands, taps, seed):
    return np.random.Generator(np.random.PCG64(seed)).uniform(-0.2, 0.2, (n_bands, taps))


def test_listener_bands_filter_bank():
    """Filters of 9 taps over 2 poses, then of 33 taps over 5: the filter bank and the scratch grow."""
    r, f = fresh(band_table(4)), fresh(band_table(4))
    try:
        batch(r.render_listener_bands(arr(POSES[:2]), irs=True, filters=filters(4, 9, 1)))
        g = filters(4, 33, 2)
        got = batch(r.render_listener_bands(arr(POSES[:5]), irs=True, filters=g))
        assert got == batch(f.render_listener_bands(arr(POSES[:5]), irs=True, filters=g))
    finally:
        r.close()
        f.close()


def test_synth_and_walk_scratch():
    """arx_combine_bands at ir_len 1000, then 4000; arx_convolute_walk over 2 blocks, then 6."""
    rng = np.random.Generator(np.random.PCG64(3))
    r, f = fresh(), fresh()
    try:
        g = filters(4, 31, 4)
        irs = {n: tuple(rng.exponential(1e-3, (4, n)).astype(np.float32) for _ in range(2)) for n in (1000, 4000)}
        r.combine_bands(irs[1000], g)
        got = r.combine_bands(irs[4000], g)["ir"]
        assert got[0].any() and plain(got) == plain(f.combine_bands(irs[4000], g)["ir"])
        B = 256
        L, R = (rng.exponential(1e-3, (3, SR)).astype(np.float32) for _ in range(2))
        x = rng.uniform(-1, 1, 6 * B)
        r.convolute_walk((L, R), [0, 1], x[:2 * B], B, B)
        sched = [0, 1, 1, 2, 0, 2]
        got = r.convolute_walk((L, R), sched, x, B, B)["out"]
        assert got.any() and plain(got) == plain(f.convolute_walk((L, R), sched, x, B, B)["out"])
        assert r.walk_state() == f.walk_state()
    finally:
        r.close()
        f.close()


@pytest.mark.parametrize("grouped", [False, True], ids=["renderer", "group"])
def test_file_convolution_staging(grouped):
    """A 1.5 s file, then a 3.5 s file: the staging buffers grow -- one renderer's, and those of a group of
    device 0 listed twice."""
    def make():
        if not grouped:
            return fresh()
        g = RenderGroup(RenderSettings(**S), devices=[0, 0], scene=box(np.full(12, 0.25, np.float32)), receiver=receiver_local())
        g.setEmitterPosInOptix(EMITTER)
        g.setSphereCenterInOptix(*HOME)
        return g

    x = np.random.Generator(np.random.PCG64(5)).standard_normal(7 * SR // 2).astype(np.float32)
    r, f = make(), make()
    try:
        for y in (r, f):
            y.render()
        r.convoluteAudioFile(x[:3 * SR // 2])
        got = r.convoluteAudioFile(x)[:2]
        assert got[0].any() and got[1].any() and plain(got) == plain(f.convoluteAudioFile(x)[:2])
    finally:
        r.close()
        f.close()


def test_directivity_cube_and_plane():
    """A res 4 cube, then a res 16 cube, arx_render_bands after each: the cube grows, the plane is remade."""
    orders = [0.0, 1.0, 2.0, 3.0]
    r, f = fresh(band_table(4)), fresh(band_table(4))
    try:
        r.set_source_directivity(cardioid_cube(4, orders))
        small = batch(r.render_bands(irs=True))
        for x in (r, f):
            x.set_source_directivity(cardioid_cube(16, orders))
        got = batch(r.render_bands(irs=True))
        assert got == batch(f.render_bands(irs=True)) and got != small
    finally:
        r.close()
        f.close()


def test_frame_sets_released_and_remade():
    """Three frames in flight, three renders, back to one: the sets are released and set 0 is remade."""
    r, f = fresh(), fresh()
    try:
        r.set_frames_in_flight(3)
        for _ in range(3):
            r.render()
        r.set_frames_in_flight(1)
        assert frame(r) == frame(f)
    finally:
        r.close()
        f.close()
