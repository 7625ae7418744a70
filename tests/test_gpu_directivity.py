"""GPU: directional sources (include/arx.h "Directional sources") -- arx_render_bands and
arx_render_listener_bands with a pattern installed.

The room is the 12-triangle box of tests/test_gpu_bands.py, (-3, 0, -2) to (3, 3, 2), emitter (-1.5, 1.2, 0),
listener (1.5, 1.2, 0.3); 16 kHz, 64 x 64 x 16 = 65 536 rays, 16 bounces, hrtf 0.5, base power 3.62, patterns
of res 4.  The band tables are test_gpu_bands.band_table's and the scene carries their column minimum.  Every
comparison is on bits; no tolerance anywhere.

The oracle case rests on one fact: for a gain 2^-j the directed ray is the plain ray scaled exactly -- every
step of a ray's energy is an f32 product, which commutes with a power of two while nothing underflows (e0 is
about 1e-5 and sixteen reflections take at most 1e-16 off it) -- and e * 2^-j > thres is e > thres * 2^j.
So the reference of (band, level j) is the CPU oracle's per-ray records on the scene carrying that band's
absorption with energy_thres * 2^j, from which numpy rebuilds the fixed-point deposits.
"""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pyoracle as po
from audiorenderingv2_amd import (ArxError, RenderSettings, debug_ray_directions, directivity_gains, frac_bits,
                                  source_rotation)
from audiorenderingv2_amd._lib import lib
from audiorenderingv2_amd.scene import Scene
from conftest import oracle_threads, world_scene
from test_gpu_bands import render_bands, same
from test_gpu_listener_bands import BOX_EMITTER, box_scene, call, loop, make, same_cells, thres

pytestmark = pytest.mark.gpu

RAYS = (64, 64, 16)
N = 64 * 64 * 16
LISTENER = ((1.5, 1.2, 0.3), 0.0)
RES = 4
OVER = dict(max_bounces=16)
INVALID, NOT_READY = 1, 4
LEVELS = np.array([1.0, 0.5, 0.25, 0.0], np.float32)
YAW90 = source_rotation(90.0)
TILT = source_rotation(33.0, -20.0, 71.0)
# five poses, each turned; all batched (none holds the emitter in its grown box)
POSES = [((1.5, 1.2, 0.3), 0.0), ((0.8, 1.6, -0.7), 120.0), ((2.2, 2.0, 1.1), 40.0), ((-0.2, 0.9, 1.2), 250.0),
         ((1.9, 0.8, -1.3), 310.0)]


def renderer(n_bands, **over):
    scene, table = box_scene(False, n_bands)
    return make(scene, RAYS, True, BOX_EMITTER, LISTENER, table, **{**OVER, **over})


def level_cube(n_bands, seed=11):
    """Texels in {1, 1/2, 1/4, 0}, another arrangement per band."""
    idx = np.random.Generator(np.random.PCG64(seed)).integers(0, 4, (n_bands, 6, RES, RES))
    return LEVELS[idx]


def bit_cube(n_bands, seed=5):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 2, (n_bands, 6, RES, RES)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ray_dirs():
    """The launch's ray directions by ray id (seed 1); shared, never written."""
    return debug_ray_directions(1, 0, N)


def counters(bands):
    return [b[2] for b in bands]


# ---------------------------------------------------------------- 1. the plane ---
@pytest.mark.parametrize("n_bands", [3, 8])
def test_plane_equals_the_host_lookup(n_bands):
    """The device plane, row for row of the cache's direction copy, is arx_directivity_gains_host's."""
    r = renderer(n_bands)
    try:
        r.render_bands(acoustics=False)  # the recording
        assert r.path_cache_state()["state"] in ("recorded", "replayed")
        # the cache's direction copy is the frame set's buffer of the recording launch, slot for slot
        slots = r.ray_order_buffer(N)["dirs"][:, :3]
        assert np.array_equal(np.sort(slots.view(np.uint32), axis=0), np.sort(ray_dirs().view(np.uint32), axis=0))
        cube = level_cube(n_bands) * np.float32(0.8125) + np.float32(0.125)
        made = lib().arx_debug_directivity_planes_made(r.handle)
        for k, m in enumerate((np.eye(3), TILT)):
            r.set_source_directivity(cube)
            r.set_source_orientation(m)
            plane = r.directivity_plane()
            W = 4 if n_bands <= 4 else 8
            assert plane.shape == (N, W)
            want = directivity_gains(cube, slots, m, W)
            assert np.array_equal(plane.view(np.uint32), want.view(np.uint32))
            assert not plane[:, n_bands:].any() and plane[:, :n_bands].min() > 0
            part = r.directivity_plane(1000, 77)
            assert np.array_equal(part, plane[1000:1077])
        # a one-band cube serves every band, the padding stays 0
        r.set_source_directivity(cube[1])
        plane = r.directivity_plane()
        want = directivity_gains(cube[1], slots, TILT, W)
        assert all(np.array_equal(plane[:, b], want[:, 0]) for b in range(n_bands)) and not plane[:, n_bands:].any()
        # made once per change, reused otherwise
        assert lib().arx_debug_directivity_planes_made(r.handle) == made + 3
        r.directivity_plane(0, 1)
        r.render_bands(acoustics=False)
        assert lib().arx_debug_directivity_planes_made(r.handle) == made + 3
    finally:
        r.close()


def test_plane_needs_a_pattern_and_a_recording():
    r = renderer(3)
    try:
        with pytest.raises(ArxError) as e:
            r.directivity_plane(0, 1)
        assert e.value.status == NOT_READY and "arx_set_source_directivity" in str(e.value)
        r.set_source_directivity(level_cube(3))
        with pytest.raises(ArxError) as e:
            r.directivity_plane(0, 1)
        assert e.value.status == NOT_READY and "recording" in str(e.value)
    finally:
        r.close()


# ------------------------------------------------------- 2. omni is the old path ---
def test_all_ones_is_the_undirected_call_and_dropping_restores_it():
    r = renderer(3)
    try:
        plain, _ = render_bands(r)
        plain_batch = call(r, POSES[:2])
        r.set_source_directivity(np.ones((3, 6, RES, RES), np.float32))
        ones, _ = render_bands(r)
        for b in range(3):
            same(ones[b], plain[b], f"all-ones band {b}")  # IR bits, counters, acoustics bytes
        same_cells(call(r, POSES[:2])["cells"], plain_batch["cells"], "all-ones batch")
        r.set_source_directivity(np.ones((6, RES, RES), np.float32))  # one band for all
        assert r.n_directivity_bands == 1
        ones, _ = render_bands(r)
        for b in range(3):
            same(ones[b], plain[b], f"one-band all-ones band {b}")
        # a pattern that takes rays away, then dropped: the undirected launchers' counts again
        r.set_source_directivity(bit_cube(3))
        cut, _ = render_bands(r)
        assert all(c[0] < p[0] for c, p in zip(counters(cut), counters(plain)))
        cut_batch = call(r, POSES[:2])
        assert cut_batch["cells"][1][0][2][0] < plain_batch["cells"][1][0][2][0]
        r.set_source_directivity(None)
        assert r.n_directivity_bands == 0
        again, _ = render_bands(r)
        assert counters(again) == counters(plain)
        for b in range(3):
            same(again[b], plain[b], f"dropped band {b}")
        same_cells(call(r, POSES[:2])["cells"], plain_batch["cells"], "dropped batch")
    finally:
        r.close()


# ---------------------------------------------------- 3. exact partition, no oracle ---
@pytest.mark.parametrize("n_bands", [3, 5])
def test_a_mask_and_its_complement_add_up_to_the_undirected_run(n_bands):
    r = renderer(n_bands, energy_thres=0.0)
    try:
        plain, _ = render_bands(r)
        h_plain = r.band_histograms()
        assert h_plain.shape == (n_bands, 2, r.ir_length) and h_plain.any()
        mask = bit_cube(n_bands)
        r.set_source_directivity(mask)
        half_a, _ = render_bands(r)
        h_a = r.band_histograms()
        r.set_source_directivity(np.float32(1.0) - mask)
        half_b, _ = render_bands(r)
        h_b = r.band_histograms()
        for b in range(n_bands):
            hits = plain[b][2][1]
            assert min(half_a[b][2][1], half_b[b][2][1]) >= hits / 4, (b, half_a[b][2], half_b[b][2], hits)
            assert tuple(x + y for x, y in zip(half_a[b][2], half_b[b][2])) == plain[b][2], b
        assert np.array_equal(h_a + h_b, h_plain)
    finally:
        r.close()


# -------------------------------------------- 4. against the oracle, power-of-two levels ---
REC_DTYPE = np.dtype([("energy", "<f4"), ("distance", "<f4"), ("depth", "<i4"), ("bin", "<i4"), ("queries", "<i4"),
                      ("last_tri", "<i4"), ("path_hash", "<u4")])


def oracle_records(absorption, energy_thres):
    """orc_trace_records of the whole launch on the box carrying `absorption`, in blocks side by side."""
    assert C.sizeof(po.OrcRayRecord) == REC_DTYPE.itemsize
    scene, _ = box_scene(False, 3)
    tv, ta = world_scene(Scene(scene.tri_v, absorption, scene.names), *LISTENER)
    osc = po.Scene(tv, ta, bvh=True)
    s = RenderSettings(rays=RAYS, **{**dict(sample_rate=16000, base_power=3.62, hrtf_absorption_rate=0.5), **OVER})
    p = po.make_params(rays=RAYS, sample_rate=16000, ir_seconds=s.ir_length_in_seconds, base_power=3.62,
                       energy_thres=energy_thres, max_bounces=16, hrtf=0.5, seed=s.seed, emitter=BOX_EMITTER,
                       listener=LISTENER[0])
    block = 8192

    def one(first):
        rec = (po.OrcRayRecord * block)()
        po.lib().orc_trace_records(C.byref(osc.s), C.byref(p), first, block, rec)
        return np.frombuffer(rec, dtype=REC_DTYPE).copy()

    with ThreadPoolExecutor(max_workers=oracle_threads()) as pool:
        return np.concatenate(list(pool.map(one, range(0, N, block)))), p, (ta == -1.0)


@functools.lru_cache(maxsize=None)
def oracle_case(energy_thres):
    """Per band the raw [L | R] histograms (stereo and mono) and the counters a directed render of level_cube(3)
    must give, from the oracle's records alone; asserts that every non-zero level of every band holds at least
    50 receiver hits."""
    _, table = box_scene(False, 3)
    cube = level_cube(3)
    gains = directivity_gains(cube, ray_dirs(), None, 4)  # by ray id, as the oracle numbers its rays
    out = []
    for b in range(3):
        hist = {mono: np.zeros((2, 32000), np.int64) for mono in (False, True)}
        cnt = [0, 0, 0]
        for j in range(3):
            rec, p, is_left = oracle_records(table[b], float(np.float32(energy_thres) * np.float32(2.0 ** j)))
            rays = gains[:, b] == LEVELS[j]
            rc = rec[rays]
            got = rc["bin"] >= 0
            assert int(got.sum()) >= 50, (b, j, int(got.sum()))
            cnt[0] += int(rc["queries"].sum())
            cnt[1] += int(got.sum())
            cnt[2] += int(((rc["depth"] == -1) & (rc["bin"] < 0)).sum())
            n = p.ir_length
            assert n == 32000
            e0 = np.float32(po.lib().orc_initial_energy(C.byref(p)))
            inv_unit = np.ldexp(1.0, frac_bits(N)) / np.float64(e0)
            scale = np.float32(2.0 ** -j)
            h = rc[got & (rc["bin"] < n)]
            left = is_left[h["last_tri"]]
            k = h["bin"].astype(np.int64)
            delay = int(16000 * 0.00044)
            kk = np.where(k + delay < n, k + delay, k)
            own = np.rint((h["energy"] * scale).astype(np.float64) * inv_unit).astype(np.int64)
            other = np.rint(((h["energy"] * (np.float32(1.0) - np.float32(0.5))) * scale).astype(np.float64) * inv_unit).astype(np.int64)
            for mono in (False, True):
                np.add.at(hist[mono][0], k[left], own[left])
                np.add.at(hist[mono][1], k[~left], own[~left])
            np.add.at(hist[False][1], kk[left], other[left])
            np.add.at(hist[False][0], kk[~left], other[~left])
        # rays at gain 0 count nothing: they are in no level above
        out.append((hist, tuple(cnt), p))
    return out


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
@pytest.mark.parametrize("thres_factor", [0.0, 0.02], ids=["thres0", "thres"])
def test_power_of_two_levels_against_the_oracle(thres_factor, mono):
    energy_thres = thres(RAYS, thres_factor) if thres_factor else 0.0
    want = oracle_case(energy_thres)
    r = renderer(3, energy_thres=energy_thres, mono=mono)
    try:
        r.set_source_directivity(level_cube(3))
        bands, _ = render_bands(r)
        raw = r.band_histograms()
        for b in range(3):
            hist, cnt, p = want[b]
            print(f"band {b}: counters {bands[b][2]} oracle {cnt}")
            assert bands[b][2] == cnt, (b, bands[b][2], cnt)
            assert np.array_equal(raw[b], hist[mono]), b
            p.is_mono = 1 if mono else 0
            irl, irr = po.finalize_ir(p, hist[mono][0], hist[mono][1])
            p.is_mono = 0
            assert np.array_equal(bands[b][0], irl.view(np.uint32)) and np.array_equal(bands[b][1], irr.view(np.uint32)), b
        if thres_factor:  # the threshold does end bands early: the case differs from thres0's
            assert [w[1] for w in want] != [w[1] for w in oracle_case(0.0)]
    finally:
        r.close()


# ------------------------------------------------------------------- 5. turning ---
def test_turning_the_source_costs_no_recording():
    cube = level_cube(3) * np.float32(0.75) + np.float32(0.25) * bit_cube(3, seed=9)
    r = renderer(3)
    try:
        r.set_source_directivity(cube)
        first, _ = render_bands(r)
        state = r.path_cache_state(queries=True)
        made = lib().arx_debug_directivity_planes_made(r.handle)
        r.set_source_orientation(90.0)
        out = r.render_bands(irs=True, acoustics=True)
        assert out["stats"]["warm_launches"].tolist() == [0, 0, 0]
        assert r.path_cache_state(queries=True) == state  # no new recording: the same records, the same last launch
        assert lib().arx_debug_directivity_planes_made(r.handle) == made + 1
        turned, _ = render_bands(r)
        assert counters(turned) != counters(first)
        fresh = renderer(3)
        try:
            fresh.set_source_orientation(YAW90)
            fresh.set_source_directivity(cube)
            want, _ = render_bands(fresh)
        finally:
            fresh.close()
        for b in range(3):
            same(turned[b], want[b], f"turned band {b}")
            assert np.array_equal(out["ir"][0][b].view(np.uint32), want[b][0])
        r.set_source_orientation(0.0)
        back, _ = render_bands(r)
        for b in range(3):
            same(back[b], first[b], f"turned back band {b}")
        # the pattern and the orientation survive a new table and a new scene
        scene, table = box_scene(False, 3)
        r.set_source_orientation(YAW90)
        r.set_band_absorption(table)
        r.set_scene(scene)
        r.set_band_absorption(table)
        assert r.n_directivity_bands == 3
        again, _ = render_bands(r)
        for b in range(3):
            same(again[b], want[b], f"after set_scene band {b}")
    finally:
        r.close()


# ------------------------------------------------------------ 6. the listener batch ---
@pytest.mark.parametrize("chunk", [1, 2])
def test_listener_batch_equals_the_loop(chunk):
    r = renderer(3)
    ref = renderer(3)
    try:
        for x in (r, ref):
            x.set_source_directivity(level_cube(3))
            x.set_source_orientation(TILT)
        r.set_listener_chunk(chunk)
        got = call(r, POSES)
        assert [int(x) for x in got["stats"]["route"][:, 0]] == [0] * 5  # all batched
        want, _ = loop(ref, POSES)
        same_cells(got["cells"], want, f"chunk {chunk}")
        plain = renderer(3)
        try:
            undirected = call(plain, POSES[:1])
        finally:
            plain.close()
        assert got["cells"][0][0][2] != undirected["cells"][0][0][2]  # the pattern does reach the batch
    finally:
        r.close()
        ref.close()


# -------------------------------------------------------------------- 7. errors ---
def test_band_count_mismatch_changes_nothing():
    scene4, table4 = box_scene(False, 4)
    r = make(scene4, RAYS, True, BOX_EMITTER, LISTENER, table4, **OVER)
    try:
        r.set_source_directivity(level_cube(4))
        before, _ = render_bands(r)
        raw = r.band_histograms()
        r.set_source_directivity(level_cube(3))  # installing is fine: the rule is checked at render time
        for fn in (lambda: r.render_bands(irs=True), lambda: call(r, POSES[:2]), lambda: r.directivity_plane(0, 1)):
            with pytest.raises(ArxError) as e:
                fn()
            assert e.value.status == INVALID and "3 bands" in str(e.value), str(e.value)
        assert r.n_directivity_bands == 3 and np.array_equal(r.band_histograms(), raw)  # previous results in place
        # rejected patterns and orientations leave the installed ones
        bad = level_cube(3)
        bad[2, 1, 3, 0] = np.nan
        with pytest.raises(ArxError) as e:
            r.set_source_directivity(bad)
        assert e.value.status == INVALID and "band 2" in str(e.value) and "face 1" in str(e.value)
        with pytest.raises(ArxError):
            r.set_source_directivity(np.full((9, 6, 2, 2), 0.5, np.float32))
        with pytest.raises(ArxError):
            r.set_source_orientation(np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1]]))
        assert r.n_directivity_bands == 3
        r.set_source_directivity(level_cube(4))
        after, _ = render_bands(r)
        for b in range(4):
            same(after[b], before[b], f"band {b}")
    finally:
        r.close()
