"""The streaming convolution's crossfade at an IR change (arx_stream_set_crossfade): a transition
block is computed with the old and the new partition spectra from the same delay line and blended
in the time domain.  The oracle of a transition block is built here from two po.Stream objects
(old and new IR) fed the same blocks: old + w * (new - old) on the first F frames, new after."""
import numpy as np
import pytest

import pyoracle as po
from audiorenderingv2_amd import ArxError, AudioRenderer, DeviceBuffer, LiveStream, RenderSettings, fade_weights

pytestmark = pytest.mark.gpu


def make_irs(sr, seed, secs=2):
    """One left/right IR pair, built like test_gpu_live.py's live_renderer(), plus a direct-sound tap
    on frame 0: twelve blocks of 1 or 16 frames reach only the IR's first frames, which the 500
    random taps of 2 s mostly leave empty -- every output would be zero and the blend unseen."""
    rng = np.random.default_rng(seed)
    n = sr * secs
    irs = []
    for _ in range(2):
        ir = np.zeros(n, np.float32)
        ir[rng.integers(0, n, 500)] = rng.exponential(1e-3, 500).astype(np.float32)
        ir[0] = np.float32(rng.exponential(1e-3))
        irs.append(ir)
    return irs


def renderer_with(sr, irs):
    r = AudioRenderer(RenderSettings(rays=(1, 1, 1), sample_rate=sr, ir_length_in_seconds=2))
    r.set_ir(*irs)
    return r


def rel_err(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def blend(old, new, w):
    """The transition block's oracle on zipped L/R frames."""
    ref = new.copy()
    w2 = np.repeat(w, 2)
    ref[:w2.size] = old[:w2.size] + w2 * (new[:w2.size] - old[:w2.size])
    return ref


@pytest.mark.parametrize("sr,block,fade,shape", [(8000, 4096, 4096, "hann"),    # N = 8192, the LDS limit
                                                 (16000, 256, 85, "linear"),
                                                 (22050, 1000, 1000, "hann"),   # N - B != B
                                                 (8000, 16, 7, "hann"),
                                                 (8000, 1, 1, "linear")])       # N = 16, the smallest plan
def test_transition_blocks_match_blended_oracle(sr, block, fade, shape):
    irs = [make_irs(sr, 100 * block + k) for k in range(4)]
    r = renderer_with(sr, irs[0])
    s = LiveStream(r, block, crossfade_frames=fade, fade=shape)
    assert s.crossfade == (fade, shape)
    w = fade_weights(shape, fade)
    refs = [po.Stream(block, *ir) for ir in irs]  # every IR's stream hears the whole input
    change_before = {4: 1, 5: 2, 9: 3}            # back-to-back transitions, then one on the ragged block
    cur = 0
    rng = np.random.default_rng(sr + block)
    for k in range(12):
        if k in change_before:
            cur = change_before[k]
            r.set_ir(*irs[cur])
        n = block // 3 if (k == 9 and block >= 3) else block
        x = rng.uniform(-1, 1, n)
        outs = [ref.process(x) for ref in refs]
        want = blend(outs[cur - 1], outs[cur], w) if k in change_before else outs[cur]
        got = s.process(x)
        err = rel_err(got, want)
        print(f"block {k}: rel err {err:.3e}")
        assert err < 1e-12, k
        if k in change_before:  # and the blend is visible at this tolerance
            assert rel_err(got, outs[cur]) > 1e-6, k
    assert s.crossfades == 3


def test_fade_off_and_steady_state_are_todays_bits():
    sr, block = 16000, 256
    ir_a, ir_b = make_irs(sr, 1), make_irs(sr, 2)
    rs = [renderer_with(sr, ir_a) for _ in range(3)]
    plain, zero, faded = (LiveStream(r, block) for r in rs)
    zero.set_crossfade(0, "linear")
    faded.set_crossfade(100, "hann")
    rng = np.random.default_rng(3)
    for k in range(7):
        if k == 3:
            for r in rs:
                r.set_ir(*ir_b)
        x = rng.uniform(-1, 1, block)
        a, b, c = plain.process(x), zero.process(x), faded.process(x)
        assert np.array_equal(a, b), k
        if k != 3:
            assert np.array_equal(a, c), k
        else:
            assert not np.array_equal(a[:200], c[:200])  # the fade is there
            assert np.array_equal(a[200:], c[200:])      # and ends after its 100 frames
    assert (plain.crossfades, zero.crossfades, faded.crossfades) == (0, 0, 1)


@pytest.mark.parametrize("sr,block,fade", [(8000, 4096, 4096), (22050, 1000, 600), (8000, 16, 16)])
def test_same_ir_transition_is_bit_identical(sr, block, fade):
    irs = make_irs(sr, block)
    r0, r1 = renderer_with(sr, irs), renderer_with(sr, irs)
    plain = LiveStream(r0, block)
    faded = LiveStream(r1, block, crossfade_frames=fade, fade="hann")
    rng = np.random.default_rng(block)
    for k in range(5):
        if k == 3:
            r0.set_ir(*irs)
            r1.set_ir(*irs)
        x = rng.uniform(-1, 1, block)
        assert np.array_equal(plain.process(x), faded.process(x)), k
    assert faded.crossfades == 1 and plain.crossfades == 0


def test_no_fade_on_first_block_or_after_reset():
    sr, block = 8000, 256
    irs = [make_irs(sr, 20 + k) for k in range(3)]
    r = renderer_with(sr, irs[0])
    s = LiveStream(r, block, crossfade_frames=block, fade="linear")
    r.set_ir(*irs[1])  # before the very first block
    ref = po.Stream(block, *irs[1])
    rng = np.random.default_rng(21)
    for k in range(3):
        x = rng.uniform(-1, 1, block)
        assert rel_err(s.process(x), ref.process(x)) < 1e-12, k
    assert s.crossfades == 0
    s.reset()
    r.set_ir(*irs[2])  # between the reset and the next block
    ref = po.Stream(block, *irs[2])
    x = rng.uniform(-1, 1, block)
    assert rel_err(s.process(x), ref.process(x)) < 1e-12
    assert s.crossfades == 0
    r.set_ir(*irs[0])  # the stream has a previous block again: this one fades
    ref_old, ref_new = ref, po.Stream(block, *irs[0])
    ref_new.process(x)
    x = rng.uniform(-1, 1, block)
    want = blend(ref_old.process(x), ref_new.process(x), fade_weights("linear", block))
    assert rel_err(s.process(x), want) < 1e-12
    assert s.crossfades == 1


def test_fade_bounds_the_boundary_step():
    sr, block, a, b = 8000, 256, 0.5, 0.875
    n = 2 * sr
    scale = n / (n // 2)  # the live path's scale

    def delta(g):
        ir = np.zeros(n, np.float32)
        ir[0] = g
        return ir, ir.copy()

    def ears(blocks):  # zipped blocks -> (frames, 2)
        return np.concatenate(blocks).reshape(-1, 2)

    ones = np.ones(block)
    r = renderer_with(sr, delta(a))
    s = LiveStream(r, block)
    before = [s.process(ones) for _ in range(2)]
    r.set_ir(*delta(b))
    y = ears([before[1], s.process(ones)])
    click = np.abs(y[block] - y[block - 1])
    print("hard switch: step", click, "expected", abs(b - a) * scale)
    assert np.all(np.abs(click - abs(b - a) * scale) <= 1e-12 * abs(b - a) * scale)  # the test can see the click
    for shape in ("linear", "hann"):
        r = renderer_with(sr, delta(a))
        s = LiveStream(r, block, crossfade_frames=block, fade=shape)
        before = [s.process(ones) for _ in range(2)]
        r.set_ir(*delta(b))
        y = ears([before[1], s.process(ones)])
        w = fade_weights(shape, block)
        bound = abs(b - a) * scale * max(w[0], np.diff(w).max(), 1.0 - w[-1]) * (1 + 1e-9)
        step = np.abs(np.diff(y, axis=0)).max()
        print(f"{shape}: largest step {step:.6e}, bound {bound:.6e}")
        assert step <= bound, shape
        assert s.crossfades == 1


def test_device_path_equals_host_path():
    sr, block = 22050, 1000
    ir_a, ir_b = make_irs(sr, 31), make_irs(sr, 32)
    r0, r1 = renderer_with(sr, ir_a), renderer_with(sr, ir_a)
    host = LiveStream(r0, block, crossfade_frames=700, fade="hann")
    dev = LiveStream(r1, block, crossfade_frames=700, fade="hann")
    d_out = DeviceBuffer(r1.settings.device, 2 * block * 8)
    rng = np.random.default_rng(33)
    for k in range(4):
        if k == 2:
            r0.set_ir(*ir_b)
            r1.set_ir(*ir_b)
        x = rng.uniform(-1, 1, block)
        want = host.process(x)
        d_in = DeviceBuffer.from_numpy(r1.settings.device, x)
        dev.process_device(d_in.ptr, block, d_out.ptr)
        r1.stats()  # synchronises the renderer's stream
        assert np.array_equal(d_out.to_numpy(np.float64), want), k
        d_in.close()
    assert host.crossfades == 1 and dev.crossfades == 1
    d_out.close()


def test_crossfade_rejects_bad_arguments():
    r = renderer_with(8000, make_irs(8000, 41))
    s = LiveStream(r, 256)
    assert s.crossfade[0] == 0 and s.crossfades == 0
    for frames, shape in [(257, "hann"), (-1, "hann"), (16, 2), (16, "cosine")]:
        with pytest.raises(ArxError):
            s.set_crossfade(frames, shape)
    assert s.crossfade[0] == 0
    with pytest.raises(ArxError):
        LiveStream(r, 256, crossfade_frames=4096)
    s.set_crossfade(256, "linear")
    assert s.crossfade == (256, "linear")
    s.set_crossfade(0)
    assert s.crossfade[0] == 0
