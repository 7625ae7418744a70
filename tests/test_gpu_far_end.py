"""GPU: the far end of the impulse response -- the distance limit, the drop and the fold -- on every render route.

Three rules decide what a ray does near the end of the IR (devicePrograms.cu:125-136, :227-236; restated by
oracle/arx_oracle.c's trace_one):
  * distance limit: a ray asks for no further query once dist >= ir_seconds * 343 + 1 (wants_query);
  * drop: a receiver hit whose bin k = roundf(dist / 343 * sr) is >= ir_len counts as a hit and adds nothing;
  * fold: the opposite ear's share goes to k + delay, or to k itself when k + delay >= ir_len, with
    delay = (int)(sr * 0.00044).
shade() holds them for the traced frame, the replay and the candidate chains, band_shade() for the band kernels,
and the filtered routes rebuild a frame's query count from recorded counts, which is right only if a ray ended
by the distance limit is counted like one ended by max_bounces.

The scene: a closed hall of 12 triangles, (-6, 0, -5.5) to (6, 8, 5.5), absorption 0.05 on every wall, emitter
(-3, 3, 2), base power 3.62, hrtf 0.5, energy_thres 0 and a 1 s IR (344 m of path).  Its volume, about
1000 m^3, is near sigma x 344 m for the receiver's cross-section, which puts the most arrivals at the end of
the IR.  Pose A with 64 x 64 x 64 rays is compared with the CPU oracle; pose B and a walk of three more
poses, each turned, with 64 x 64 x 16 rays serve the comparisons between two GPU routes.  The low sample
rates are deliberate: the fold's window is 0.44 ms of path whatever the rate, and at 2500 Hz a bin is 13.7 cm
long, so the two bins at the boundary hold tens of hits each where 16 kHz has a handful.

Conditions on the inputs are asserted from the oracle's per-ray records, with the real placement
(conftest.world_scene), before anything is compared (far_end_classes, pose_classes): enough hits in every
boundary class, enough drops and folds, and all three ray endings at once with 48 bounces.  What the
fixtures measured is kept in profiles/r20/far_end_classes.json.  The placement needed no adjustment: pose A
as first chosen satisfies every minimum.

"Equal" means both IR channels' bits and (queries, receiver hits, misses), and, wherever both sides carry an
analysis, the bytes of the three arx_acoustics: the late bins feed T30 and the decay curve.  Every
comparison is on bits.  The oracle frames are made once per setting and shared; so are the frames of the
cache-off renderers the GPU routes are compared with.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pyoracle as po
from audiorenderingv2_amd import AudioRenderer, RenderGroup, RenderSettings, receiver_local
from audiorenderingv2_amd.scene import Scene, _box_tris
from conftest import oracle_threads, world_scene
from test_gpu_bands import frame, oracle_frame, render_bands, same, thres
from test_gpu_listener_bands import arr, call, loop, same_cells
from test_gpu_listeners import acou_key, check as check_listeners, routes

pytestmark = pytest.mark.gpu

HALL = Scene(_box_tris(np.array([[-6.0, 0.0, -5.5]], np.float32), np.array([[6.0, 8.0, 5.5]], np.float32)),
             np.full(12, 0.05, np.float32), ["wall"] * 12)
EMITTER = (-3.0, 3.0, 2.0)
A = ((3.0, 4.0, -2.0), 0.0)
B = ((-2.0, 5.0, 3.0), 75.0)
WALK = [((1.0, 2.0, 0.5), 140.0), ((4.5, 6.0, 3.5), 200.0), ((-4.0, 1.5, -3.5), 310.0)]
POSES = [A, B] + WALK
FULL = (64, 64, 64)   # against the oracle
PART = (64, 64, 16)   # one GPU route against another
S = dict(base_power=3.62, hrtf_absorption_rate=0.5, energy_thres=0.0, ir_length_in_seconds=1)
BATCHED, SINGLE = 0, 1


def n_of(rays):
    return rays[0] * rays[1] * rays[2]


# ------------------------------------------------------------------ the oracle ---
def oracle_params(pose, rays, sample_rate, max_bounces=64, ir_length_in_seconds=1, hrtf_absorption_rate=0.5, mono=False):
    return po.make_params(rays=rays, sample_rate=sample_rate, ir_seconds=ir_length_in_seconds, base_power=3.62,
                          energy_thres=0.0, max_bounces=max_bounces, hrtf=hrtf_absorption_rate, mono=mono,
                          emitter=EMITTER, listener=pose[0])


@functools.lru_cache(maxsize=None)
def _oracle_hist(pose, rays, sample_rate, *rest):
    p = oracle_params(pose, rays, sample_rate, *rest)
    L, R, st = po.Scene(*world_scene(HALL, *pose), bvh=True).trace(p, threads=oracle_threads())
    return p, L, R, st


def oracle_hist(pose, rays, sample_rate, max_bounces=64, ir_length_in_seconds=1, hrtf_absorption_rate=0.5, mono=False):
    """(params, left and right i64 histograms, stats) of the oracle's whole launch; shared, never written."""
    return _oracle_hist(pose, rays, sample_rate, max_bounces, ir_length_in_seconds, hrtf_absorption_rate, mono)


def oracle(pose, rays, sample_rate, **over):
    """The oracle's frame as same() takes it; it has no analysis."""
    p, L, R, st = oracle_hist(pose, rays, sample_rate, **over)
    irl, irr = po.finalize_ir(p, L, R)
    return irl.view(np.uint32), irr.view(np.uint32), (st["queries"], st["receiver_hits"], st["misses"]), None


def classes(rec, sample_rate, max_bounces, seconds=1):
    """How the rays of a launch end, from the oracle's records (the record's own bin: np.round is not roundf)."""
    n, delay = sample_rate * seconds, int(sample_rate * 0.00044)
    received = rec["last_tri"] >= 12
    k = rec["bin"][received].astype(np.int64)
    going = ~received & (rec["depth"] >= 0) & (rec["depth"] < max_bounces)  # neither received, missed nor out of bounces
    return dict(sample_rate=sample_rate, max_bounces=max_bounces, delay=delay, received=int(received.sum()),
                dropped=int((k >= n).sum()), k_last=int((k == n - 1).sum()), k_len=int((k == n).sum()),
                kd_last=int((k + delay == n - 1).sum()), kd_len=int((k + delay == n).sum()),
                folds=int(((k < n) & (k + delay >= n)).sum()) if delay else 0,
                distance_limited=int((going & (rec["distance"] >= np.float32(seconds * 343 + 1))).sum()),
                all_bounces=int((rec["depth"] == max_bounces).sum()))


def record_classes(jobs):
    """classes() of (pose, rays, sample_rate, max_bounces) jobs.  The record pass is single-threaded: each job's
    rays go to it in blocks of 16 384, side by side."""
    block = 16384

    scenes = {pose: po.Scene(*world_scene(HALL, *pose), bvh=True) for pose in {job[0] for job in jobs}}  # read only

    def one(task):
        (pose, rays, sample_rate, max_bounces), first = task
        return scenes[pose].records(oracle_params(pose, rays, sample_rate, max_bounces), first, min(block, n_of(rays) - first))

    tasks = [(job, first) for job in jobs for first in range(0, n_of(job[1]), block)]
    with ThreadPoolExecutor(max_workers=oracle_threads()) as pool:
        recs = list(pool.map(one, tasks))
    return {job: classes(np.concatenate([r for (j, _), r in zip(tasks, recs) if j == job]), job[2], job[3]) for job in jobs}


A_JOBS = [(A, FULL, sr, 64) for sr in (1000, 2500, 5000, 16000, 48000)] + [(A, FULL, 2500, 48)]
POSE_JOBS = [(p, PART, sr, mb) for p in POSES for sr in (2500, 16000) for mb in (64, 48)]


@pytest.fixture(scope="module")
def far_end_classes():
    """Pose A with 262 144 rays: the boundary classes are populated, or no comparison below means anything."""
    got = record_classes(A_JOBS)
    for (_, _, sr, mb), c in got.items():
        if mb == 64:
            assert c["dropped"] >= 500 and c["distance_limited"] >= 20000, c
            assert c["folds"] >= 10 or c["delay"] == 0, c  # 1000 Hz has no delay and so no fold
        else:  # three endings in one launch
            assert min(c["received"], c["distance_limited"], c["all_bounces"]) >= 1000, c
    c = got[(A, FULL, 2500, 64)]
    assert min(c["k_last"], c["k_len"], c["kd_last"], c["kd_len"]) >= 10, c
    return got


@pytest.fixture(scope="module")
def pose_classes():
    """Every pose with 65 536 rays, A included: each frame has a drop, a fold and distance-limited rays."""
    got = record_classes(POSE_JOBS)
    for c in got.values():
        assert c["dropped"] >= 1 and c["folds"] >= 1 and c["distance_limited"] >= 1000, c
    return got


# ------------------------------------------------------------------ renderers ---
def make(cache, rays=PART, pose=A, absorption=None, table=None, **over):
    scene = HALL if absorption is None else Scene(HALL.tri_v, absorption, HALL.names)
    r = AudioRenderer(RenderSettings(**{**S, "rays": rays, **over}), scene=scene, receiver=receiver_local())
    r.set_path_cache(1 if cache else 0)
    r.setEmitterPosInOptix(EMITTER)
    r.setSphereCenterInOptix(*pose)
    if table is not None:
        r.set_band_absorption(table)
    return r


class Refs:
    """Cache-off renderers, one per (absorption, shape, settings), and their analysed frames by pose."""

    def __init__(self):
        self.rs, self.frames, self.analyses = {}, {}, {}

    def want(self, pose, absorption=None, rays=PART, as_dicts=False, **over):
        """The frame with its analysis as bytes, or (as_dicts) as test_gpu_listeners.check takes it."""
        rk = (None if absorption is None else absorption.tobytes(), rays, tuple(sorted(over.items())))
        if rk not in self.rs:
            self.rs[rk] = make(False, rays, pose, absorption, **over)
        if (rk, pose) not in self.frames:
            r = self.rs[rk]
            r.setSphereCenterInOptix(*pose)
            self.frames[(rk, pose)] = frame(r, analyse=True)
            self.analyses[(rk, pose)] = tuple(acou_key(r.acoustics(ch)) for ch in ("left", "right", "sum"))
            assert r.path_cache_state()["state"] == "off"
        return self.frames[(rk, pose)][:3] + (self.analyses[(rk, pose)],) if as_dicts else self.frames[(rk, pose)]

    def close(self):
        for r in self.rs.values():
            r.close()


@pytest.fixture(scope="module")
def refs():
    x = Refs()
    yield x
    x.close()


def group_frame(g):
    g.render()
    L, R = g.get_ir()
    st = g.stats()
    return L.view(np.uint32), R.view(np.uint32), (st["queries"], st["receiver_hits"], st["misses"]), None


# ------------------------------------------------------------------ 1. the traced frame against the oracle ---
@pytest.mark.parametrize("sample_rate", [1000, 2500, 5000, 16000, 48000])
def test_traced_frame_equals_the_oracle(far_end_classes, sample_rate):
    """delay 0 (1000 Hz: no fold at all), 1, 2, 7 and 21 (48 kHz)."""
    r = make(False, FULL, sample_rate=sample_rate, max_bounces=64)
    try:
        got = frame(r)
        same(got, oracle(A, FULL, sample_rate), sample_rate)
        assert got[2][1] > 170000 and got[0].any() and got[1].any()
    finally:
        r.close()


VARIANTS = {"path-0": {}, "path-8": {}, "path-1": {}, "path-2": {}, "path-3": {},
            "mono": dict(mono=True),
            # hrtf 1: the opposite ear's share is exactly zero and hist_add skips it; hrtf 0: it is the whole energy
            "hrtf-0": dict(hrtf_absorption_rate=0.0), "hrtf-1": dict(hrtf_absorption_rate=1.0),
            "bounces-48": dict(max_bounces=48),          # received, distance-limited and out-of-bounces rays at once
            "two-seconds": dict(ir_length_in_seconds=2)}  # the limit at 687 m: a few rays of 64 bounces reach it


@pytest.mark.parametrize("what", list(VARIANTS))
def test_traced_frame_at_2500_hz(far_end_classes, what):
    over = {"max_bounces": 64, **VARIANTS[what]}
    r = make(False, FULL, sample_rate=2500, **over)
    try:
        if what.startswith("path-"):
            r.set_trace_path(int(what[5:]))
        got = frame(r)
        same(got, oracle(A, FULL, 2500, **over), what)
        if what == "mono":
            assert np.array_equal(got[0], got[1])
    finally:
        r.close()


def test_group_of_two_and_three_shards_at_2500_hz(far_end_classes):
    """RenderGroup(devices=[0, 0]) and three trace_rays shards of one renderer: the whole launch's frame."""
    want = oracle(A, FULL, 2500)
    g = RenderGroup(RenderSettings(**{**S, "rays": FULL, "sample_rate": 2500, "max_bounces": 64}), devices=[0, 0],
                    scene=HALL, receiver=receiver_local())
    try:
        g.setEmitterPosInOptix(EMITTER)
        g.setSphereCenterInOptix(*A)
        same(group_frame(g), want, "group of two")
    finally:
        g.close()
    r = make(False, FULL, sample_rate=2500, max_bounces=64)
    try:
        r.clear_histogram()
        for b, e in ((0, 70001), (70001, 200000), (200000, n_of(FULL))):
            r.trace_rays(b, e)
        r.finalize_ir()
        L, R = r.get_ir()
        st = r.stats()
        same((L.view(np.uint32), R.view(np.uint32), (st["queries"], st["receiver_hits"], st["misses"]), None), want,
             "three shards")
    finally:
        r.close()


@pytest.mark.parametrize("sample_rate", [2500, 16000])
def test_the_far_end_shows_in_the_oracle(far_end_classes, sample_rate):
    """The 3 s histogram cut to one second is the 1 s histogram up to the fold's window, and its rays go on past
    344 m: the 1 s frames above do end rays at the limit and do fold."""
    _, l1, r1, st1 = oracle_hist(A, FULL, sample_rate)
    _, l3, r3, st3 = oracle_hist(A, FULL, sample_rate, ir_length_in_seconds=3)
    keep = sample_rate - 2 * int(sample_rate * 0.00044)
    assert np.array_equal(l3[:keep], l1[:keep]) and np.array_equal(r3[:keep], r1[:keep])
    assert l3[:keep].sum() == l1[:keep].sum() > 0 and r3[:keep].sum() == r1[:keep].sum() > 0
    assert not np.array_equal(l3[keep:sample_rate], l1[keep:]) or not np.array_equal(r3[keep:sample_rate], r1[keep:])
    assert st3["queries"] > st1["queries"]
    assert l3[sample_rate:].any() and r3[sample_rate:].any()  # what the 1 s frame drops


# ------------------------------------------------------------------ 2. the path cache, unfiltered and filtered ---
def warm(r, want, filtered, fif=1):
    """Each frame set traces once, one launch records, the next replays: every frame equal to want."""
    states = []
    for k in range(fif + 2):
        same(frame(r, analyse=True), want, f"warm-up frame {k}")
        states.append(r.path_cache_state()["state"])
        assert r.path_filter_state()["filtered"] == (filtered and states[-1] != "traced"), (k, states)
    assert states == ["traced"] * fif + ["recorded", "replayed"], states


def walk(r, refs, filtered, **settings):
    for pose in [B] + WALK + [A]:
        r.setSphereCenterInOptix(*pose)
        same(frame(r, analyse=True), refs.want(pose, **settings), pose)
        assert r.path_cache_state()["state"] == "replayed", pose
        assert r.path_filter_state()["filtered"] == filtered, pose


@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "filtered"])
@pytest.mark.parametrize("sample_rate,max_bounces", [(2500, 64), (2500, 48), (16000, 64), (16000, 48)])
def test_replayed_walk_equals_cache_off(refs, pose_classes, sample_rate, max_bounces, filtered):
    """Traced, recorded and replayed at A -- equal to the cache-off frame, which is the oracle's -- then the walk."""
    settings = dict(sample_rate=sample_rate, max_bounces=max_bounces)
    r = make(True, **settings)
    try:
        r.set_path_filter(filtered)
        want = refs.want(A, **settings)
        same(want, oracle(A, PART, **settings), "cache-off frame against the oracle")
        warm(r, want, filtered)
        walk(r, refs, filtered, **settings)
    finally:
        r.close()


def test_replayed_walk_with_two_frames_in_flight(refs, pose_classes):
    settings = dict(sample_rate=2500, max_bounces=64)
    r = make(True, **settings)
    try:
        r.set_frames_in_flight(2)
        warm(r, refs.want(A, **settings), True, fif=2)
        walk(r, refs, True, **settings)
    finally:
        r.close()


@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "filtered"])
def test_replayed_whole_launch_equals_the_oracle(refs, far_end_classes, filtered):
    """262 144 rays x 64 bounces (402 MB of records, under the default cap): the replayed frames at A are the
    oracle's, and the frame at B the cache-off renderer's."""
    settings = dict(sample_rate=2500, max_bounces=64)
    r = make(True, FULL, **settings)
    try:
        r.set_path_filter(filtered)
        want = refs.want(A, rays=FULL, **settings)
        same(want, oracle(A, FULL, 2500), "cache-off frame against the oracle")
        warm(r, want, filtered)
        r.setSphereCenterInOptix(*B)
        same(frame(r, analyse=True), refs.want(B, rays=FULL, **settings), "B")
        assert r.path_cache_state()["state"] == "replayed" and r.path_filter_state()["filtered"] == filtered
    finally:
        r.close()


# ------------------------------------------------------------------ 3. render_listeners ---
@pytest.mark.parametrize("chunk", [1, 0], ids=["chunk-1", "chunk-auto"])
@pytest.mark.parametrize("sample_rate,max_bounces", [(2500, 64), (16000, 64), (2500, 65)])
def test_render_listeners_is_the_loop(refs, pose_classes, sample_rate, max_bounces, chunk):
    """The five poses in one call; 65 bounces are past the filter's limit, so every listener goes the one-listener
    route with the unfiltered replay."""
    settings = dict(sample_rate=sample_rate, max_bounces=max_bounces)
    r = make(True, **settings)
    try:
        for _ in range(3):
            r.render()
        assert r.path_cache_state()["state"] == "replayed"
        r.set_listener_chunk(chunk)
        out = r.render_listeners(arr(POSES), irs=True)
        assert routes(out) == [SINGLE if max_bounces > 64 else BATCHED] * len(POSES), routes(out)
        check_listeners(out, [refs.want(pose, as_dicts=True, **settings) for pose in POSES], f"chunk {chunk}")
        st = out["stats"][0]
        same((out["ir"][0][0].view(np.uint32), out["ir"][1][0].view(np.uint32),
              (int(st["queries"]), int(st["receiver_hits"]), int(st["misses"])), None),
             oracle(A, PART, **settings), "A against the oracle")
    finally:
        r.close()


# ------------------------------------------------------------------ 4. render_bands ---
def band_table(n_bands):
    """PCG64(7)'s uniform(0.05, 0.09, (B, 12)) as f32; the scene carries its column minimum."""
    return np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.09, (n_bands, 12)).astype(np.float32)


def banded(n_bands, **over):
    table = band_table(n_bands)
    return make(True, absorption=table.min(axis=0), table=table, **over), table


# f32(e0 * 0.0105) with 65 536 rays, chosen on the CPU: with energy_thres 0 the weakest ray still going at the limit
# carries more than that in band 2 and less in bands 0, 1 and 3, so bands 0, 1 and 3 lose rays to this threshold
# before 344 m and band 2 loses none.  test_render_bands asserts exactly that from the oracle's query counts.
DYING = thres(PART, 0.0105)
DYING_BANDS = [True, True, False, True]


BAND_CASES = {"2500-4": (2500, 4, {}), "2500-8": (2500, 8, {}), "16000-4": (16000, 4, {}), "16000-8": (16000, 8, {}),
              "2500-4-threshold": (2500, 4, dict(energy_thres=DYING)),
              "2500-4-mono": (2500, 4, dict(mono=True)), "2500-4-hrtf-0.25": (2500, 4, dict(hrtf_absorption_rate=0.25))}


@pytest.mark.parametrize("what", list(BAND_CASES))
def test_render_bands(refs, pose_classes, what):
    """Each band is the frame of a cache-off renderer that carries the band's column, and band 0 the oracle's.
    With energy_thres 0 every band reaches the far end; with the threshold some bands die before it."""
    sample_rate, n_bands, over = BAND_CASES[what]
    settings = dict(sample_rate=sample_rate, max_bounces=64, **over)
    r, table = banded(n_bands, **settings)
    try:
        bands, _ = render_bands(r)
        for b in range(n_bands):
            same(bands[b], refs.want(A, absorption=table[b], **settings), f"{what} band {b}")
        same(bands[0], oracle_frame(HALL, table[0], PART, EMITTER, A, **{**S, **settings}), f"{what} band 0, oracle")
        if "mono" in over:
            assert all(np.array_equal(x[0], x[1]) for x in bands)
        if "energy_thres" in over:
            free = [oracle_frame(HALL, table[b], PART, EMITTER, A, **{**S, **settings, "energy_thres": 0.0})[2][0]
                    for b in range(n_bands)]
            cut = [oracle_frame(HALL, table[b], PART, EMITTER, A, **{**S, **settings})[2][0] for b in range(n_bands)]
            assert all(c <= f for c, f in zip(cut, free)) and [c < f for c, f in zip(cut, free)] == DYING_BANDS, (cut, free)
            assert [x[2][0] for x in bands] == cut
        # a listener move needs no new recording; B's far end through the same walk
        r.setSphereCenterInOptix(*B)
        bands, stats = render_bands(r)
        assert stats["warm_launches"].tolist() == [0] * n_bands
        for b in range(n_bands):
            same(bands[b], refs.want(B, absorption=table[b], **settings), f"{what} band {b} at B")
    finally:
        r.close()


# ------------------------------------------------------------------ 5. render_listener_bands ---
@pytest.mark.parametrize("n_bands", [4, 8])
@pytest.mark.parametrize("sample_rate", [2500, 16000])
def test_render_listener_bands(refs, pose_classes, sample_rate, n_bands):
    """Poses x bands in one call: the loop of set_listener + render_bands on a second renderer, and cell by cell
    the cache-off renderer at that pose with that band's column."""
    settings = dict(sample_rate=sample_rate, max_bounces=64)
    r, table = banded(n_bands, **settings)
    other, _ = banded(n_bands, **settings)
    try:
        out = call(r, POSES)
        assert [int(x) for x in out["stats"]["route"][:, 0]] == [BATCHED] * len(POSES)
        same_cells(out["cells"], loop(other, POSES)[0], "the loop")
        for j, pose in enumerate(POSES):
            for b in range(n_bands):
                same(out["cells"][j][b], refs.want(pose, absorption=table[b], **settings), (pose, b))
    finally:
        r.close()
        other.close()
