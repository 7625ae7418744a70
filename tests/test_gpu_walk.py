"""GPU: the walk-through convolution (arx_convolute_walk, include/arx.h) is the loop it stands for --
arx_set_ir_device + arx_stream_process_device block after block on a fresh stream with the same
crossfade -- bit for bit, whatever the tile, the pointers' homes or the IRs the schedule leaves out;
it agrees with the CPU oracle's streams blended by hand; and it leaves its renderer alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle as po
from audiorenderingv2_amd import (ArxError, AudioRenderer, DeviceBuffer, LiveStream, RenderSettings, fade_weights,
                                  receiver_local, walk_blocks, walk_schedule)
from audiorenderingv2_amd._lib import lib
from audiorenderingv2_amd.scene import Scene, _box_tris

pytestmark = pytest.mark.gpu

INVALID = 1  # ARX_ERR_INVALID_ARGUMENT
# (sample rate, IR seconds, block B, fade F): the smallest shapes at which each part can go wrong
SHAPES = [(8000, 2, 4096, 4096),   # N = 8192, the LDS limit, P = 4
          (22050, 2, 1000, 600),   # N - B != B, P = 45
          (16000, 1, 256, 85),     # P = 63
          (8000, 2, 16, 7),        # P = 1000, more partitions than blocks
          (8000, 1, 1, 1)]         # N = 16, the smallest plan, fewer bins than a workgroup
SCHEDULE = [0, 0, 0, 0, 1, 2, 2, 2, 2, 3, 3, 0, 0, 0]  # back-to-back transitions, a return to an earlier IR


def make_irs(sr, seed, secs=2):
    """One left/right IR pair as tests/test_gpu_stream_crossfade.py builds it: 500 random taps plus a
    direct-sound tap on frame 0, without which blocks of 1 or 16 frames would all be zero."""
    rng = np.random.default_rng(seed)
    n = sr * secs
    irs = []
    for _ in range(2):
        ir = np.zeros(n, np.float32)
        ir[rng.integers(0, n, 500)] = rng.exponential(1e-3, 500).astype(np.float32)
        ir[0] = np.float32(rng.exponential(1e-3))
        irs.append(ir)
    return irs


def rel_err(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def renderer(sr, secs, ir=None):
    r = AudioRenderer(RenderSettings(rays=(1, 1, 1), sample_rate=sr, ir_length_in_seconds=secs))
    if ir is not None:
        r.set_ir(*ir)
    return r


@functools.lru_cache(maxsize=None)
def ir_stack(sr, secs, k, seed):
    """k IR pairs as ([k, n] left, [k, n] right)."""
    pairs = [make_irs(sr, seed + j, secs) for j in range(k)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def signal(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def ragged_frames(B):
    """The input ends a third into block 9 (on its boundary for B < 3): blocks 10 and later have none."""
    return 9 * B + B // 3


def loop(sr, secs, L, R, sched, x, B, F, shape="hann"):
    """The definition: a fresh stream on a renderer of its own, the IR set from device memory before
    block 0 and before every block whose index differs from the block before, one process_device each."""
    sched = [int(j) for j in sched]
    n, nb = sr * secs, len(sched)
    r = renderer(sr, secs)
    try:
        s = LiveStream(r, B, crossfade_frames=F, fade=shape)
        dl, dr = DeviceBuffer.from_numpy(0, L), DeviceBuffer.from_numpy(0, R)
        d_in = DeviceBuffer.from_numpy(0, np.concatenate([x, np.zeros(1)]))
        d_out = DeviceBuffer(0, 2 * nb * B * 8)
        for b, j in enumerate(sched):
            if b == 0 or j != sched[b - 1]:
                r.set_ir_device(dl.ptr + j * n * 4, dr.ptr + j * n * 4)
            m = min(max(x.size - b * B, 0), B)
            s.process_device(d_in.ptr + b * B * 8 if m else 0, m, d_out.ptr + 2 * b * B * 8)
        r.stats()  # synchronises the renderer's stream
        out = d_out.to_numpy(np.float64).reshape(-1, 2)
        crossfades = s.crossfades
        s.close()
        for buf in (dl, dr, d_in, d_out):
            buf.close()
        return out, crossfades
    finally:
        r.close()


@functools.lru_cache(maxsize=None)
def main_case(shape_index, faded):
    """Test 1's inputs and the loop's output for one shape, with its fade or without: shared, not modified."""
    sr, secs, B, F = SHAPES[shape_index]
    L, R = ir_stack(sr, secs, 4, 1000 * shape_index)
    x = signal(ragged_frames(B), 77 + shape_index)
    want, crossfades = loop(sr, secs, L, R, SCHEDULE, x, B, F if faded else 0)
    want.setflags(write=False)
    return L, R, x, want, crossfades


@pytest.mark.parametrize("shape_index", range(len(SHAPES)))
def test_equals_the_loop_bit_for_bit(shape_index):
    sr, secs, B, F = SHAPES[shape_index]
    r = renderer(sr, secs)
    try:
        for faded in (True, False):
            L, R, x, want, crossfades = main_case(shape_index, faded)
            assert crossfades == (4 if faded else 0)
            assert np.abs(want).max() > 0.0
            got = r.convolute_walk((L, R), SCHEDULE, x, B, F if faded else 0, "hann")
            assert got["out"].shape == (14 * B, 2)
            bad = [b for b in range(14) if not np.array_equal(got["out"][b * B:(b + 1) * B], want[b * B:(b + 1) * B])]
            assert not bad, (faded, bad)
            assert got["ms"] > 0.0
            st = r.walk_state()
            assert (st["blocks"], st["transitions"], st["irs_transformed"]) == (14, 4 if faded else 0, 4)
            n_trans = 4 if faded else 0
            assert st["scratch_bytes"] == lib().arx_debug_walk_bytes(sr * secs, B, 4, 14, n_trans, F if faded else 0)
        faded_out, plain_out = main_case(shape_index, True)[3], main_case(shape_index, False)[3]
        assert not np.array_equal(faded_out[4 * B:5 * B], plain_out[4 * B:5 * B])  # the fade is there
        assert np.array_equal(faded_out[3 * B:4 * B], plain_out[3 * B:4 * B])
    finally:
        r.close()


@pytest.mark.parametrize("shape_index", [0, 2])
def test_against_the_cpu_oracle(shape_index):
    """Independent of the stream: one oracle stream per IR hears the whole zero-extended input; a plain
    block is its IR's output, a transition block old + w (new - old) on the first F frames, new after."""
    sr, secs, B, F = SHAPES[shape_index]
    L, R, x, _, _ = main_case(shape_index, True)
    nb = len(SCHEDULE)
    xz = np.concatenate([x, np.zeros(nb * B - x.size)])
    refs = []
    for j in range(4):
        s = po.Stream(B, L[j], R[j])
        refs.append(np.stack([s.process(xz[b * B:(b + 1) * B]) for b in range(nb)]))  # [block, 2 B] zipped
    w2 = np.repeat(fade_weights("linear", F), 2)
    r = renderer(sr, secs)
    try:
        got = r.convolute_walk((L, R), SCHEDULE, x, B, F, "linear")["out"].reshape(nb, 2 * B)
    finally:
        r.close()
    for b, j in enumerate(SCHEDULE):
        new = refs[j][b]
        want = new.copy()
        transition = b > 0 and SCHEDULE[b - 1] != j
        if transition:
            old = refs[SCHEDULE[b - 1]][b]
            want[:w2.size] = old[:w2.size] + w2 * (new[:w2.size] - old[:w2.size])
        err = rel_err(got[b], want)
        print(f"block {b}: rel err {err:.3e}")
        assert err < 1e-12, b
        if transition:  # and the blend is visible at this tolerance
            assert rel_err(got[b], new) > 1e-6, b


def test_tile_seams():
    """23 blocks whose IR changes at blocks 1, 7, 8 and 16 are 27 items: tiles of 1, 3 and 5 put their
    seams inside runs, between a transition's two items and between two transitions."""
    sr, secs, B, F = SHAPES[2]
    sched = [0] + [1] * 6 + [2] + [3] * 8 + [0] * 7
    assert len(sched) == 23 and [b for b in range(1, 23) if sched[b] != sched[b - 1]] == [1, 7, 8, 16]
    L, R = ir_stack(sr, secs, 4, 2000)
    x = signal(17 * B + 100, 5)
    want, crossfades = loop(sr, secs, L, R, sched, x, B, F)
    assert crossfades == 4
    r = renderer(sr, secs)
    try:
        for tile in (1, 3, 5, 0):
            r.set_walk_tile(tile)
            got = r.convolute_walk((L, R), sched, x, B, F)["out"]
            assert np.array_equal(got, want), tile
            st = r.walk_state()
            assert (st["blocks"], st["transitions"]) == (23, 4)
            if tile:
                assert st["tiles"] == -(-27 // tile), tile
        with pytest.raises(ArxError):
            r.set_walk_tile(65)
        with pytest.raises(ArxError):
            r.set_walk_tile(-1)
    finally:
        r.close()


def test_dedupe_and_unused_irs():
    sr, secs, B, F = SHAPES[2]
    L, R = (a.copy() for a in ir_stack(sr, secs, 6, 3000))
    for j in (0, 2, 3, 5):
        L[j] = np.nan
        R[j] = np.nan
    sched = [1, 1, 4, 4, 1, 1, 1, 4, 1, 4, 4]  # A B A: each of the two is transformed once
    x = signal(6 * B + 17, 6)
    want, _ = loop(sr, secs, L, R, sched, x, B, F)
    r = renderer(sr, secs)
    try:
        got = r.convolute_walk((L, R), sched, x, B, F)["out"]
        assert np.isfinite(got).all()
        assert np.array_equal(got, want)
        st = r.walk_state()
        assert st["irs_transformed"] == 2 and st["transitions"] == 5
    finally:
        r.close()


def test_host_and_device_pointers():
    sr, secs, B, F = SHAPES[2]
    L, R, x, want, _ = main_case(2, True)
    nb = len(SCHEDULE)
    r = renderer(sr, secs)
    bufs = []
    try:
        host = r.convolute_walk((L, R), SCHEDULE, x, B, F)["out"]
        dl, dr, dx = (DeviceBuffer.from_numpy(0, a) for a in (L, R, x))
        d_out = DeviceBuffer(0, 2 * nb * B * 8)
        bufs += [dl, dr, dx, d_out]
        res = r.convolute_walk((dl, dr), SCHEDULE, dx, B, F, n_irs=4, n_frames=x.size, out=d_out)
        assert res["out"] is d_out
        dev = d_out.to_numpy(np.float64).reshape(-1, 2)
        mixed = r.convolute_walk((dl.ptr, dr.ptr), SCHEDULE, x, B, F, n_irs=4)["out"]  # device IRs, host audio
        d_out2 = DeviceBuffer(0, 2 * nb * B * 8)
        bufs.append(d_out2)
        r.convolute_walk((L, R), SCHEDULE, dx, B, F, n_frames=x.size, out=d_out2)       # host IRs, device audio
        mixed2 = d_out2.to_numpy(np.float64).reshape(-1, 2)
        for name, got in (("host", host), ("device", dev), ("mixed", mixed), ("mixed2", mixed2)):
            assert np.array_equal(got, want), name
    finally:
        for b in bufs:
            b.close()
        r.close()


def test_leaves_the_renderer_alone():
    sr, secs, B, F = SHAPES[2]
    L, R = ir_stack(sr, secs, 5, 4000)
    own = [make_irs(sr, 4100 + k, secs) for k in range(3)]
    r, twin = renderer(sr, secs, own[0]), renderer(sr, secs, own[0])
    try:
        s, s_twin = (LiveStream(q, B, crossfade_frames=60, fade="linear") for q in (r, twin))
        rng = np.random.default_rng(9)
        blocks = [rng.uniform(-1, 1, B) for _ in range(6)]
        outs, outs_twin = [], []
        for k in range(6):
            if k in (2, 4):
                r.set_ir(*own[k // 2])
                twin.set_ir(*own[k // 2])
            if k == 3:  # two walk calls between the stream's blocks, the second larger: the scratch grows
                before = r.get_ir()
                x1 = signal(3 * B + 5, 10)
                sched1 = [0, 0, 1, 1, 2, 2]
                got1 = r.convolute_walk((L, R), sched1, x1, B, F)
                bytes1 = r.walk_state()["scratch_bytes"]
                x2 = signal(9 * 512, 11)
                sched2 = [4, 3, 3, 3, 2, 2, 1, 0, 0, 0, 4, 4, 4, 4, 4, 2, 2, 2, 2, 2]
                got2 = r.convolute_walk((L, R), sched2, x2, 512, 512, "linear")
                assert r.walk_state()["scratch_bytes"] > bytes1
                got3 = r.convolute_walk((L, R), sched1, x1, B, F)  # and the kept scratch serves the smaller again
                after = r.get_ir()
                assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
                assert np.array_equal(after[0], own[1][0])
            outs.append(s.process(blocks[k]))
            outs_twin.append(s_twin.process(blocks[k]))
        for k in range(6):
            assert np.array_equal(outs[k], outs_twin[k]), k
        assert s.crossfades == s_twin.crossfades == 2
        assert s.crossfade == (60, "linear")
        assert np.array_equal(got1["out"], loop(sr, secs, L, R, sched1, x1, B, F)[0])
        assert np.array_equal(got3["out"], got1["out"])
        assert np.array_equal(got2["out"], loop(sr, secs, L, R, sched2, x2, 512, 512, "linear")[0])
    finally:
        r.close()
        twin.close()


def test_from_a_listener_batch_on_the_device():
    """The chain scene -> path cache -> listener batch -> audible walk without the IRs visiting the host."""
    walls = _box_tris(np.array([[-3.0, 0.0, -2.0]], np.float32), np.array([[3.0, 3.0, 2.0]], np.float32))
    scene = Scene(walls, np.full(12, 0.25, np.float32), ["wall"] * 12)
    sr, B = 16000, 4096
    r = AudioRenderer(RenderSettings(rays=(16, 16, 16), sample_rate=sr, base_power=3.62, max_bounces=8,
                                     hrtf_absorption_rate=0.5), scene=scene, receiver=receiver_local())
    bufs = []
    try:
        r.setEmitterPosInOptix((-1.5, 1.2, 0.0))
        r.setSphereCenterInOptix((1.5, 1.2, 0.3), 0.0)
        poses = np.array([[1.5, 1.2, 0.3, 0.0], [0.8, 1.6, -0.7, 120.0], [0.0, 1.4, 0.8, 200.0], [-0.5, 1.2, -0.4, 30.0]],
                         np.float32)
        n = r.ir_length
        dl, dr = DeviceBuffer(0, 4 * n * 4), DeviceBuffer(0, 4 * n * 4)
        bufs += [dl, dr]
        r.render_listeners(poses, irs=(dl, dr), acoustics=False)
        x = signal(4 * B + 1234, 12)
        sched = walk_schedule(x.size, B, n, 4)
        assert sched.size == walk_blocks(x.size, B, n) == 5 + 8 and sorted(set(sched.tolist())) == [0, 1, 2, 3]
        got = r.convolute_walk((dl, dr), sched, x, B, B, "hann", n_irs=4)["out"]
        L, R = dl.to_numpy(np.float32).reshape(4, n), dr.to_numpy(np.float32).reshape(4, n)
        assert all(L[j].any() and R[j].any() for j in range(4))
        assert not np.array_equal(L[0], L[1])
        want, crossfades = loop(sr, 2, L, R, sched, x, B, B, "hann")
        assert crossfades == 3
        assert np.array_equal(got, want)
        whole = r.auralise_walk(poses, x, B)
        assert np.array_equal(whole["ir_of_block"], sched)
        assert np.array_equal(whole["out"], want)
    finally:
        for b in bufs:
            b.close()
        r.close()


def test_errors():
    sr, secs, B, F = SHAPES[2]
    L, R = ir_stack(sr, secs, 4, 1000 * 2)
    x = signal(3 * B, 13)
    sched = [0, 1, 2, 3]
    r = renderer(sr, secs)
    d = DeviceBuffer(0, 4096)
    try:
        good = r.convolute_walk((L, R), sched, x, B, F)
        state = r.walk_state()
        bad_calls = {
            "NULL IRs": lambda: r.convolute_walk((0, 0), sched, x, B, F, n_irs=4),
            "NULL right IR": lambda: r.convolute_walk((d.ptr, 0), sched, x, B, F, n_irs=4),
            "NULL out": lambda: r.convolute_walk((L, R), sched, x, B, F, out=0),
            "NULL in with frames": lambda: r.convolute_walk((L, R), sched, 0, B, F, n_frames=5),
            "no IRs": lambda: r.convolute_walk((d.ptr, d.ptr), sched, x, B, F, n_irs=0),
            "index too large": lambda: r.convolute_walk((L, R), [0, 1, 4, 3], x, B, F),
            "index negative": lambda: r.convolute_walk((L, R), [0, -1, 2, 3], x, B, F),
            "too many frames": lambda: r.convolute_walk((L, R), sched, signal(4 * B + 1, 14), B, F),
            "block 0": lambda: r.convolute_walk((L, R), sched, x[:0], 0, 0),
            "block negative": lambda: r.convolute_walk((L, R), sched, x[:0], -16, 0),
            "block above 4096": lambda: r.convolute_walk((L, R), sched, x, 4097, 0),
            "fade negative": lambda: r.convolute_walk((L, R), sched, x, B, -1),
            "fade above the block": lambda: r.convolute_walk((L, R), sched, x, B, B + 1),
            "shape number": lambda: r.convolute_walk((L, R), sched, x, B, F, 2),
            "shape name": lambda: r.convolute_walk((L, R), sched, x, B, F, "cosine"),
        }
        for name, call in bad_calls.items():
            with pytest.raises(ArxError) as e:
                call()
            assert e.value.status == INVALID, name
        st = lib().arx_convolute_walk(r.handle, L.ctypes.data, R.ctypes.data, 4, None, 4, x.ctypes.data, x.size, B, F, 1,
                                      good["out"].ctypes.data, None)
        assert st == INVALID  # a NULL schedule
        short = renderer(1000, 1)  # ir_len = 1000: a block of 2000 is within 4096 but above ir_len
        try:
            Ls = np.zeros((1, 1000), np.float32)
            with pytest.raises(ArxError) as e:
                short.convolute_walk((Ls, Ls), [0], x[:10], 2000, 0)
            assert e.value.status == INVALID
        finally:
            short.close()
        assert r.walk_state() == state
        empty = r.convolute_walk((L, R), [], x[:0], B, F)
        assert empty["out"].shape == (0, 2) and empty["ms"] == 0.0
        assert r.walk_state() == state  # n_blocks == 0 touches nothing
        again = r.convolute_walk((L, R), sched, x, B, F)  # and the renderer is as usable as before
        assert np.array_equal(again["out"], good["out"])
    finally:
        d.close()
        r.close()
