"""GPU: the room-acoustic analysis (arx_analyze_ir: decay curves, EDT / T20 / T30, C50 / C80, D50, Ts)
against the definitions restated in Python (acoustics_ref.py) and the host function.

Histograms are injected without tracing (a DeviceBuffer of 2*ir_len int64 attached with
arx_attach_histogram), so every shape costs an upload and a handful of small launches.  Bars: the decay
curve of all three channels equals the Python ints exactly; the integer fields and the valid mask
equal the host function's exactly; the floats are within 1e-9 relative of the numpy reference
(acoustics_ref.RTOL), NaN and +inf in the same places; the same call twice gives the same bytes.
Both scan shapes (one workgroup per channel, tiled) are held to all of it.
"""
import ctypes as C

import numpy as np
import pytest

import acoustics_ref as ref
from audiorenderingv2_amd import (ArxError, AudioRenderer, DeviceBuffer, RenderGroup, RenderSettings,
                                  acoustics_from_histogram, receiver_local)
from audiorenderingv2_amd._lib import ArxAcoustics, lib

pytestmark = pytest.mark.gpu

CHANNELS = ("left", "right", "sum")
# the CPU suite's three shapes and 44.1 kHz x 3 s = 132 300 bins, then the edge inputs
CASES = [f"decay{i}" for i in range(len(ref.SHAPES))] + ["decay_44k"] + list(ref.EDGE_NAMES)


def raw(r, channel):
    a = ArxAcoustics()
    st = lib().arx_get_acoustics(r.handle, channel, C.byref(a))
    return st, bytes(a)


def analyze_injected(L, R, sr, shape):
    n = L.size
    assert n % sr == 0
    r = AudioRenderer(RenderSettings(rays=(4, 4, 4), ir_length_in_seconds=n // sr, sample_rate=sr))
    buf = DeviceBuffer.from_numpy(0, np.concatenate([L, R]).astype(np.int64))
    try:
        r.set_scan_shape(shape)
        r.attach_histogram(buf.ptr, 2 * n)
        r.analyze_ir()
        got = {ch: r.acoustics(ch) for ch in CHANNELS}
        curves = {ch: r.edc(ch) for ch in CHANNELS}
        first = [raw(r, c) for c in range(3)]
        r.analyze_ir()
        again = [raw(r, c) for c in range(3)]
        assert np.array_equal(buf.to_numpy(np.int64), np.concatenate([L, R]))  # the analysis only reads it
        r.attach_histogram(None)
    finally:
        r.close()
        buf.close()
    return got, curves, first, again


@pytest.mark.parametrize("shape", [1, 2])
@pytest.mark.parametrize("name", CASES)
def test_injected_histograms(name, shape):
    L, R, sr, want = ref.case(name)
    got, curves, first, again = analyze_injected(L, R, sr, shape)
    host = acoustics_from_histogram(L, R, sr, got["sum"]["unit"])
    for ch in CHANNELS:
        assert np.array_equal(curves[ch], want[ch][1]), (name, ch)
        for k in ref.INTS + ("valid", "unit"):
            assert got[ch][k] == host[ch][k], (name, ch, k, got[ch][k], host[ch][k])
        ref.assert_matches(got[ch], want[ch][0], f"{name} {ch}")
    assert all(st == 0 for st, _ in first + again)
    assert [b for _, b in first] == [b for _, b in again]  # the same call twice: the same bytes


def test_not_ready_and_bad_channel():
    r = AudioRenderer(RenderSettings(rays=(4, 4, 4), ir_length_in_seconds=1, sample_rate=1000))
    try:
        assert raw(r, 0)[0] == 4  # ARX_ERR_NOT_READY: nothing was analysed yet
        with pytest.raises(ArxError) as ei:
            r.edc("left")
        assert ei.value.status == 4
        r.analyze_ir()  # the renderer's own (all zero) histogram: no scene needed
        a = r.acoustics("sum")
        assert a["total"] == 0 and a["valid"] == set() and a["onset_bin"] == -1 and np.isnan(a["ts_s"])
        assert not r.edc("sum").any()
        for bad in (-1, 3, "centre"):
            with pytest.raises(ArxError) as ei:
                r.acoustics(bad)
            assert ei.value.status == 1
            with pytest.raises(ArxError) as ei:
                r.edc(bad)
            assert ei.value.status == 1
        r.clear_histogram()  # a new frame: its analysis is not there yet
        assert raw(r, 0)[0] == 4
    finally:
        r.close()


# c1_scene at test_gpu_parity.py's test_c1_dense_bitwise settings
C1 = dict(rays=(64, 64, 8), sample_rate=16000, base_power=3.62, max_bounces=8, hrtf_absorption_rate=0.5)
C1_LISTENER, C1_EMITTER = (2.5, 9.9, 0.0), (0.5, 3.0, 1.0)


def c1_renderer(scene, **kw):
    r = AudioRenderer(RenderSettings(**dict(C1, **kw)), scene=scene, receiver=receiver_local())
    r.setEmitterPosInOptix(C1_EMITTER)
    r.setSphereCenterInOptix(C1_LISTENER, 0.0)
    return r


def histogram_of(r):
    ptr, n = r.histogram_device_ptr()
    out = np.empty(n, np.int64)
    r.get_ir()  # synchronises the frame
    assert lib().arx_memcpy(0, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes) == 0
    return out[:n // 2].copy(), out[n // 2:].copy()


def test_a_real_render(c1_scene):
    res = {}
    for mono in (False, True):
        r = c1_renderer(c1_scene, mono=mono)
        try:
            r.render()
            r.analyze_ir()
            L, R = histogram_of(r)
            acou = {ch: r.acoustics(ch) for ch in CHANNELS}
            rawb = [raw(r, c)[1] for c in range(3)]
            curves = {ch: r.edc(ch) for ch in CHANNELS}
            ir = r.get_ir()
            assert r.analysis_times().size == 1 and r.analysis_times()[0] > 0
        finally:
            r.close()
        assert L.any() and R.any()
        for ch, h in zip(CHANNELS, (L, R, L + R)):
            assert np.array_equal(curves[ch], np.cumsum(h[::-1])[::-1]), ch
        host = acoustics_from_histogram(L, R, C1["sample_rate"], acou["sum"]["unit"])
        want = ref.reference(L, R, C1["sample_rate"])
        for ch in CHANNELS:
            for k in ref.INTS + ("valid", "unit"):
                assert acou[ch][k] == host[ch][k], (ch, k)
            ref.assert_matches(acou[ch], want[ch][0], f"c1 {ch}")
        if not mono:  # unit is the IR's: float(hist * unit)
            assert np.array_equal(ir[0].view(np.uint32), (L * acou["sum"]["unit"]).astype(np.float32).view(np.uint32))
        res[mono] = (rawb, curves, ir)
    # is_mono merges the two ears of the f32 IR (finalize) and leaves the histogram's ears apart: channels
    # 0 and 1 of the analysis are still each ear's own curve (checked above), not the merged one
    rawb, curves, ir = res[True]
    assert np.array_equal(ir[0].view(np.uint32), ir[1].view(np.uint32))
    assert not np.array_equal(res[False][2][0], res[False][2][1])
    assert not np.array_equal(curves["left"], curves["right"]) and not np.array_equal(curves["left"], curves["sum"])
    assert rawb[0] != rawb[2] and rawb[1] != rawb[2]


def test_auto_analysis_with_frames_in_flight(c1_scene):
    seeds = (1, 7, 19)
    one = {}
    for seed in seeds:  # one frame at a time, analysed by hand, auto-analysis off
        r = c1_renderer(c1_scene, seed=seed)
        try:
            r.render()
            ir = r.get_ir()
            assert raw(r, 0)[0] == 4  # off by default: render() queued no analysis
            assert r.analysis_times().size == 0
            r.analyze_ir()
            one[seed] = ([raw(r, c) for c in range(3)], [r.edc(c) for c in range(3)], ir)
        finally:
            r.close()
    r = c1_renderer(c1_scene)
    try:
        r.set_frames_in_flight(2)
        r.set_auto_analyze(True)
        assert raw(r, 0)[0] == 4
        def snapshot():
            return [raw(r, c) for c in range(3)], [r.edc(c) for c in range(3)], r.get_ir()

        def same(got, want, what):
            assert all(st == 0 for st, _ in got[0])
            assert [b for _, b in got[0]] == [b for _, b in want[0]], what
            for c in range(3):
                assert np.array_equal(got[1][c], want[1][c]), (what, c)
            for ear in range(2):  # get_ir(): bit-identical with auto-analysis on and off
                assert np.array_equal(got[2][ear].view(np.uint32), want[2][ear].view(np.uint32)), what

        for seed in seeds:  # the frame sets rotate: each frame's results come from its own buffers
            r.set_seed(seed)
            r.render()
            same(snapshot(), one[seed], seed)
        for seed in seeds[:2]:  # two frames started back to back: the getters refer to the last one
            r.set_seed(seed)
            r.render()
        same(snapshot(), one[seeds[1]], "back to back")
        assert r.analysis_times().size == len(seeds) + 2
    finally:
        r.close()
    assert one[1][0] != one[7][0] and one[7][0] != one[19][0]  # the seeds give different results


def test_group_member_analysis(c1_scene):
    r = c1_renderer(c1_scene)
    try:
        r.render()
        r.analyze_ir()
        want = ([raw(r, c) for c in range(3)], [r.edc(c) for c in range(3)])
    finally:
        r.close()
    g = RenderGroup(RenderSettings(**C1), devices=[0, 0], scene=c1_scene, receiver=receiver_local())
    try:
        g.setEmitterPosInOptix(C1_EMITTER)
        g.setSphereCenterInOptix(C1_LISTENER, 0.0)
        g.render()
        m = g.member(0)
        m.analyze_ir()
        got = ([raw(m, c) for c in range(3)], [m.edc(c) for c in range(3)])
        # auto-analysis on a member rides behind arx_group_render's finalize
        m.set_auto_analyze(True)
        g.render()
        auto = ([raw(m, c) for c in range(3)], [m.edc(c) for c in range(3)])
    finally:
        g.close()
    for res in (got, auto):
        for c in range(3):
            assert res[1][c].tobytes() == want[1][c].tobytes(), c
        assert res[0] == want[0]
    assert want[1][2][0] > 0


def test_first_render_writes_the_parameters_once(c1_scene, tmp_path):
    """The app's --acoustics option: the flag makes the next render() analyse its histogram and write
    the three channels' parameters next to the IR dump; off by default, and cleared by the write."""
    import json

    r = c1_renderer(c1_scene)
    try:
        r.output_dir = str(tmp_path)
        r.render()
        assert not (tmp_path / "output_acoustics.json").exists() and raw(r, 0)[0] == 4
        r.set_write_acoustics_to_file_flag(True)
        r.render()
        doc = json.loads((tmp_path / "output_acoustics.json").read_text())
        assert sorted(doc) == ["left", "right", "sum"]
        for ch in CHANNELS:
            a = r.acoustics(ch)
            assert doc[ch]["total"] == a["total"] > 0 and doc[ch]["valid"] == sorted(a["valid"])
            assert doc[ch]["t30_bins"] == list(a["t30_bins"]) and doc[ch]["edt_s"] == a["edt_s"]
        (tmp_path / "output_acoustics.json").unlink()
        r.render()
        assert not (tmp_path / "output_acoustics.json").exists()
    finally:
        r.close()
