"""GPU: two frames in flight (arx_set_frames_in_flight) give the results of one frame at a time.

A render / convolute loop on a renderer with two frames in flight alternates two streams, histograms
and IRs, so frame k + 1 traces while frame k finishes and is convolved.  The frames meet where they
share state, and these tests drive exactly those places without synchronising between frames:
  * the listener moves and the emitter moves between frames (the receiver refit and the re-gridding
    write the tree the previous frame may still be tracing);
  * the seed changes (other rays) and the convolution plan is shared (IR spectra, scratch);
  * every frame convolves into the SAME caller buffers as well as into buffers of its own.
Bar: every frame's convolution, the last IR and the last frame's counters bit-identical to the same
sequence on a renderer with one frame in flight (itself parity-tested against the oracle in
test_gpu_parity.py).  The reference renders one frame at a time (AudioRenderer.cpp:489-523).
"""
import numpy as np
import pytest

from audiorenderingv2_amd import (ArxError, AudioRenderer, DeviceBuffer, RenderGroup, RenderSettings, device_count,
                                  receiver_local)
from audiorenderingv2_amd.scene import CONFERENCE_EMITTER, CONFERENCE_LISTENER

pytestmark = pytest.mark.gpu

S = dict(rays=(60, 60, 10), sample_rate=16000, base_power=3.62, max_bounces=8, hrtf_absorption_rate=0.5)
# (listener, yaw, emitter, seed) per frame: plain, listener moved and turned, listener walked far off
# the first quantization grid (re-gridding; outside the room, so that frame's IR is empty), back in
# the room with another seed, emitter moved
FRAMES = [
    (CONFERENCE_LISTENER, 0.0, CONFERENCE_EMITTER, 1),
    ((1.0, 1.2, -0.5), 30.0, CONFERENCE_EMITTER, 1),
    ((30.0, 1.2, 25.0), 90.0, CONFERENCE_EMITTER, 1),
    ((1.0, 1.2, -0.5), 30.0, CONFERENCE_EMITTER, 7),
    ((1.0, 1.2, -0.5), 30.0, (-4.0, 1.5, 1.0), 7),
]


def bits(a):
    return np.asarray(a).view(np.uint32)


def run_sequence(obj, members, audio, fif, rays=S["rays"]):
    """The frame loop without a synchronisation between frames; returns per-frame convolutions (own
    buffers), the shared buffers' final content, the last IR and the last frame's counters."""
    obj.set_frames_in_flight(fif)
    n = audio.size
    x = DeviceBuffer.from_numpy(0, audio)
    own = [(DeviceBuffer(0, 4 * n), DeviceBuffer(0, 4 * n)) for _ in FRAMES]
    shared = (DeviceBuffer(0, 4 * n), DeviceBuffer(0, 4 * n))
    for (lst, yaw, em, seed), (ol, orr) in zip(FRAMES, own):
        obj.setEmitterPosInOptix(em)
        obj.setSphereCenterInOptix(lst, yaw)
        obj.set_seed(seed)
        if isinstance(obj, RenderGroup):
            obj.render(timed=False)
        else:
            obj.clear_histogram()
            obj.trace_rays(0, int(np.prod(rays)))
            obj.finalize_ir()
        m = members[0]
        m.convolute_device(x.ptr, n, ol.ptr, orr.ptr)
        m.convolute_device(x.ptr, n, shared[0].ptr, shared[1].ptr)
    ir = members[0].get_ir()  # synchronises the last frame
    st = members[0].stats()
    outs = [(ol.to_numpy(np.float32), orr.to_numpy(np.float32)) for ol, orr in own]
    sh = (shared[0].to_numpy(np.float32), shared[1].to_numpy(np.float32))
    for b in [x, *shared] + [b for pair in own for b in pair]:
        b.close()
    return outs, sh, ir, (st["queries"], st["receiver_hits"], st["misses"])


@pytest.fixture(scope="module")
def audio():
    return (0.5 * np.sin(2 * np.pi * 440 * np.arange(3 * 16000 + 321) / 16000)).astype(np.float32)


# 16-bit BVH2 + LDS stack, global stack, CW4 with two frames in flight; three frames
@pytest.mark.parametrize("trace_path,frames", [(0, 2), (2, 2), (8, 2), (0, 3)])
def test_renderer_frames_in_flight_equal_one_at_a_time(conference, audio, trace_path, frames):
    res = {}
    for fif in (1, frames):
        r = AudioRenderer(RenderSettings(**S), scene=conference, receiver=receiver_local())
        try:
            r.set_trace_path(trace_path)
            res[fif] = run_sequence(r, [r], audio, fif)
        finally:
            r.close()
    (o1, s1, ir1, st1), (o2, s2, ir2, st2) = res[1], res[frames]
    assert ir1[0].any() and st1[1] > 0
    for k, (a, b) in enumerate(zip(o1, o2)):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), f"frame {k}"
    # consecutive frames differ, so the comparison above sees each frame's own IR
    assert o1[0][0].any() and not o1[2][0].any()
    assert not np.array_equal(o1[0][0], o1[1][0]) and not np.array_equal(o1[3][0], o1[4][0])
    assert np.array_equal(bits(s1[0]), bits(s2[0])) and np.array_equal(bits(s1[1]), bits(s2[1]))
    assert np.array_equal(bits(s2[0]), bits(o2[-1][0]))  # the shared buffers hold the last frame's
    assert np.array_equal(bits(ir1[0]), bits(ir2[0])) and np.array_equal(bits(ir1[1]), bits(ir2[1]))
    assert st1 == st2


# frames in flight per frame: both growths (1 -> 3, twice) and both shrinks (3 -> 2, 2 -> 1)
FIF_SCHEDULE = [1, 1, 3, 3, 3, 3, 2, 2, 2, 1, 3, 3]


def run_schedule(conference, audio, change):
    """Twelve frames cycling FRAMES, each render() (with its analysis) and a convolution into buffers of
    its own, nothing synchronising between frames; change: set_frames_in_flight before every frame whose
    number in FIF_SCHEDULE differs from the last one's.  Before those frames (changing or not) the
    acoustics and counters of the frame just finished are read.  Returns the per-frame convolutions,
    those reads, the last IR and the last frame's counters."""
    r = AudioRenderer(RenderSettings(**S), scene=conference, receiver=receiver_local())
    n = audio.size
    x = DeviceBuffer.from_numpy(0, audio)
    own = [(DeviceBuffer(0, 4 * n), DeviceBuffer(0, 4 * n)) for _ in FIF_SCHEDULE]
    reads = []
    try:
        r.set_auto_analyze(True)
        for k, (ol, orr) in enumerate(own):
            lst, yaw, em, seed = FRAMES[k % len(FRAMES)]
            if k > 0 and FIF_SCHEDULE[k] != FIF_SCHEDULE[k - 1]:
                if change:
                    r.set_frames_in_flight(FIF_SCHEDULE[k])
                st = r.stats()
                reads.append((r.acoustics("sum"), (st["queries"], st["receiver_hits"], st["misses"])))
            r.setEmitterPosInOptix(em)
            r.setSphereCenterInOptix(lst, yaw)
            r.set_seed(seed)
            r.render()
            r.convolute_device(x.ptr, n, ol.ptr, orr.ptr)
        ir = r.get_ir()  # synchronises the last frame
        st = r.stats()
        outs = [(ol.to_numpy(np.float32), orr.to_numpy(np.float32)) for ol, orr in own]
        return outs, reads, ir, (st["queries"], st["receiver_hits"], st["misses"])
    finally:
        for b in [x] + [b for pair in own for b in pair]:
            b.close()
        r.close()


def test_changing_frames_in_flight_between_frames(conference, audio):
    """The number of frames in flight changes four times during one renderer's life: sets are
    allocated, the current one is kept (its IR, counters and analysis still describe the last frame
    right after the change) and sets are freed.  Everything equals the same frames on a renderer that
    keeps one frame in flight."""
    o1, reads1, ir1, st1 = run_schedule(conference, audio, change=False)
    o2, reads2, ir2, st2 = run_schedule(conference, audio, change=True)
    assert ir1[0].any() and st1[1] > 0
    for k, (a, b) in enumerate(zip(o1, o2)):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), f"frame {k}"
    # consecutive frames differ, so a stale set cannot pass for the current one
    for k in range(len(o1) - 1):
        assert not np.array_equal(o1[k][0], o1[k + 1][0]), f"frames {k}, {k + 1}"
    assert len(reads1) == len(reads2) == 4
    for i, ((a1, c1), (a2, c2)) in enumerate(zip(reads1, reads2)):
        assert c1 == c2, f"counters after change {i}"
        assert a1.keys() == a2.keys()
        for key in a1:  # field for field; NaN (an invalid quantity) equals NaN
            u, v = a1[key], a2[key]
            assert u == v or (isinstance(u, float) and u != u and v != v), f"{key} after change {i}"
    assert np.array_equal(bits(ir1[0]), bits(ir2[0])) and np.array_equal(bits(ir1[1]), bits(ir2[1]))
    assert st1 == st2


@pytest.mark.parametrize("frames", [2, 3])
def test_ray_pool_launches_share_the_grid_in_flight(conference, audio, frames):
    """Launches large enough for the ray pool (C3's shape: 600K rays here) take half the CUs' wave
    slots each with frames in flight (arx_stats.trace_grid_cus), so two frames' launches run side by
    side; the full grid with one.  Every output bit-identical to one frame at a time."""
    rays = (100, 100, 60)
    res, grid = {}, {}
    for fif in (1, frames):
        r = AudioRenderer(RenderSettings(**dict(S, rays=rays)), scene=conference, receiver=receiver_local())
        try:
            res[fif] = run_sequence(r, [r], audio, fif, rays)
            grid[fif] = r.stats()["trace_grid_cus"]
        finally:
            r.close()
    assert grid[1] >= 2 and grid[frames] == grid[1] // 2, grid
    (o1, s1, ir1, st1), (o2, s2, ir2, st2) = res[1], res[frames]
    assert ir1[0].any() and st1[1] > 0
    for k, (a, b) in enumerate(zip(o1, o2)):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), f"frame {k}"
    assert np.array_equal(bits(s1[0]), bits(s2[0])) and np.array_equal(bits(s1[1]), bits(s2[1]))
    assert np.array_equal(bits(ir1[0]), bits(ir2[0])) and np.array_equal(bits(ir1[1]), bits(ir2[1]))
    assert st1 == st2


@pytest.mark.parametrize("rays,trace_path", [(S["rays"], 0), ((100, 100, 60), 2)])
def test_launches_that_cannot_share_keep_the_full_grid_in_flight(conference, rays, trace_path):
    """A launch without the ray pool (about a ray per lane, C2's shape) is its longest lane's chain, and
    a trace on the renderer's one global stack waits for the other frames' traces: both keep the full
    grid with frames in flight."""
    r = AudioRenderer(RenderSettings(**dict(S, rays=rays)), scene=conference, receiver=receiver_local())
    try:
        r.set_trace_path(trace_path)
        r.setEmitterPosInOptix(CONFERENCE_EMITTER)
        r.setSphereCenterInOptix(CONFERENCE_LISTENER, 0.0)
        r.render()
        full = r.stats()["trace_grid_cus"]
        r.set_frames_in_flight(2)
        r.render()
        r.get_ir()
        assert r.stats()["trace_grid_cus"] == full >= 2
    finally:
        r.close()


def test_group_render_two_frames_in_flight_equal_one_at_a_time(conference, audio):
    res = {}
    for fif in (1, 2):
        g = RenderGroup(RenderSettings(**S), devices=[0], scene=conference, receiver=receiver_local())
        try:
            res[fif] = run_sequence(g, g.members, audio, fif)
        finally:
            g.close()
    for k, (a, b) in enumerate(zip(res[1][0], res[2][0])):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), f"frame {k}"
    assert np.array_equal(bits(res[1][2][0]), bits(res[2][2][0])) and res[1][3] == res[2][3]


def test_rccl_group_two_frames_in_flight_equal_one_at_a_time(conference, audio):
    """Every GPU of the box in one RCCL group, two frames in flight: each frame's all-reduce runs on
    its own set's stream, ordered after the previous frame's by the renderer's event chain.  Skipped
    on a one-GPU box; bench.py keeps one frame in flight for N > 1 until this has run on a node."""
    n = device_count()
    if n < 2:
        pytest.skip(f"needs >= 2 GPUs (this box has {n})")
    res = {}
    for fif in (1, 2):
        g = RenderGroup(RenderSettings(**S), devices=list(range(n)), scene=conference, receiver=receiver_local())
        try:
            res[fif] = run_sequence(g, g.members, audio, fif)
        finally:
            g.close()
    for k, (a, b) in enumerate(zip(res[1][0], res[2][0])):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), f"frame {k}"
    assert np.array_equal(bits(res[1][2][0]), bits(res[2][2][0])) and res[1][3] == res[2][3]


def test_oversubscribed_group_two_frames_in_flight(conference):
    """Three shards summed on one device (hist_add), two frames in flight: the same IRs."""
    s = RenderSettings(**S)
    irs = {}
    for fif in (1, 2):
        g = RenderGroup(s, devices=[0, 0, 0], scene=conference, receiver=receiver_local())
        try:
            g.set_frames_in_flight(fif)
            g.setEmitterPosInOptix(CONFERENCE_EMITTER)
            out = []
            for lst, yaw, _, seed in FRAMES[1:4]:  # moved, off the grid, back in the room
                g.setSphereCenterInOptix(lst, yaw)
                g.set_seed(seed)
                g.render(timed=False)
            out.append(g.get_ir())
            irs[fif] = out
        finally:
            g.close()
    assert irs[1][0][0].any()
    assert np.array_equal(bits(irs[1][0][0]), bits(irs[2][0][0])) and np.array_equal(bits(irs[1][0][1]), bits(irs[2][0][1]))


def test_frames_in_flight_refuses_a_callers_stream_or_histogram():
    r = AudioRenderer(RenderSettings(rays=(4, 4, 4), sample_rate=16000))
    try:
        with pytest.raises(ArxError):
            r.set_frames_in_flight(4)
        r.set_frames_in_flight(2)
        with pytest.raises(ArxError):
            r.set_stream(r.get_stream())
        with pytest.raises(ArxError):
            r.attach_histogram(r.histogram_device_ptr()[0], 2 * r.ir_length)
        r.set_frames_in_flight(1)
        r.set_stream(r.get_stream())  # allowed again with one frame in flight
    finally:
        r.close()


def test_sharded_group_convolution_two_frames_in_flight(conference, audio):
    """The time-block sharded convolution (arx_group_convolute_device) of an oversubscribed group with
    two frames in flight: every frame's output frames, assembled from the ranks' shards, equal the
    same loop's with one frame in flight."""
    n = audio.size
    results = {}
    for fif in (1, 2):
        g = RenderGroup(RenderSettings(**S), devices=[0, 0, 0], scene=conference, receiver=receiver_local())
        g.set_frames_in_flight(fif)
        x = [DeviceBuffer.from_numpy(0, audio) for _ in range(3)]
        outs = []
        for lst, yaw, em, seed in FRAMES:
            bufs = [(DeviceBuffer(0, 4 * n), DeviceBuffer(0, 4 * n)) for _ in range(3)]
            g.setEmitterPosInOptix(em)
            g.setSphereCenterInOptix(lst, yaw)
            g.set_seed(seed)
            g.render(timed=False)
            g.convolute_device([b.ptr for b in x], n, [b[0].ptr for b in bufs], [b[1].ptr for b in bufs])
            outs.append(bufs)
        g.synchronize()
        frames = []
        for bufs in outs:
            L, R = np.zeros(n, np.float32), np.zeros(n, np.float32)
            for rank, (bl, br) in enumerate(bufs):
                b, e = g.conv_shard(n, rank)
                L[b:e] = bl.to_numpy(np.float32, n)[b:e]
                R[b:e] = br.to_numpy(np.float32, n)[b:e]
                bl.close()
                br.close()
            frames.append((L, R))
        for b in x:
            b.close()
        g.close()
        results[fif] = frames
    assert any(f[0].any() for f in results[1])
    for (a, b), (c, d) in zip(results[1], results[2]):
        assert np.array_equal(bits(a), bits(c)) and np.array_equal(bits(b), bits(d))
