#!/usr/bin/env python3
"""What band synthesis costs on the device (arx_combine_bands) against the host round trip it replaces.

    python tools/band_synth_time.py [--out FILE] [--commit TEXT]

The workload is C3 (1M rays x 16 bounces, 48 kHz x 2 s, the conference stand-in) with 8 bands: the table is
PCG64(7)'s uniform(0.05, 0.9, (8, T)) as f32 and the scene's absorption its column minimum, as in
tools/bands_time.py.  The band IRs are arx_render_bands' own, left in device memory; the filters are
arx_band_filters' octave bank at 48 kHz (crossovers 88.4 ... 5656.9 Hz) with 2047 and with 4095 taps, in
device memory too, and so are the outputs.  ROUNDS alternating rounds of REPS calls each, after one discarded
round, of
  (C2047) arx_combine_bands with 2047 taps: the call's device time (*ms: its copies and the kernel);
  (C4095) the same with 4095 taps;
  (D)     the chain on the device, 4095 taps: render_bands into device buffers, combine_bands on them,
          set_ir_device and a synchronise -- on the host clock;
  (H)     the chain through the host, 4095 taps: render_bands(irs=True), every band filtered with numpy's
          rfft / irfft and summed, set_ir and a synchronise -- on the host clock.
Beside them: the fmas the arithmetic needs (2 x 8 x (ir_len x taps - c (c + 1)), the clipped terms at both ends
taken out) and the achieved fma/s; arx_render_bands' device time of round 15 (profiles/r15/bands.json) for
scale; and how far the host leg's FFT result lies from the device's.  Nothing is asserted about the times.
Writes profiles/r16/band_synth.json by default."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, REPS, BANDS = 3, 10, 8
TAPS = (2047, 4095)
SETTINGS = dict(rays=(100, 100, 100), sample_rate=48000, base_power=3.62, max_bounces=16, hrtf_absorption_rate=1.0,
                ir_length_in_seconds=2)


def tree_id():
    """HEAD, marked when the working tree differs from it; "unknown" outside a git checkout."""
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode != 0:
        return "unknown"
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    return head.stdout.strip() + (" + uncommitted changes" if dirty else "")


def fma_count(ir_len, taps):
    c = (taps - 1) // 2
    return 2 * BANDS * (ir_len * taps - c * (c + 1))


def fft_combine(irs, g):
    """The host's way: each band zero-phase filtered with rfft / irfft, the bands summed, f32."""
    n, taps = irs.shape[1], g.shape[1]
    c = (taps - 1) // 2
    size = 1
    while size < n + taps:
        size *= 2
    y = np.fft.irfft(np.fft.rfft(irs.astype(np.float64), size, axis=1) * np.fft.rfft(g, size, axis=1), size, axis=1)
    return y[:, c:c + n].sum(axis=0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "band_synth.json"))
    ap.add_argument("--commit", help="what to record as the measured tree where git cannot say (a copy without .git)")
    a = ap.parse_args()

    from audiorenderingv2_amd import (AudioRenderer, DeviceBuffer, RenderSettings, band_filters, conference_standin,
                                      octave_crossovers, receiver_local)
    from audiorenderingv2_amd._lib import lib
    from audiorenderingv2_amd.scene import CONFERENCE_EMITTER, CONFERENCE_LISTENER, Scene

    conf = conference_standin()
    table = np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.9, (BANDS, conf.n_tris)).astype(np.float32)
    scene = Scene(conf.tri_v, table.min(axis=0), conf.names, table)
    r = AudioRenderer(RenderSettings(**SETTINGS), scene=scene, receiver=receiver_local())
    n = r.ir_length
    sr = SETTINGS["sample_rate"]
    xs = octave_crossovers([62.5 * 2.0 ** i for i in range(BANDS)])
    g = {t: band_filters(sr, xs, t) for t in TAPS}
    bufs = [DeviceBuffer(0, BANDS * n * 4) for _ in range(2)] + [DeviceBuffer(0, n * 4) for _ in range(2)]
    d_g = {t: DeviceBuffer.from_numpy(0, g[t]) for t in TAPS}
    try:
        r.setEmitterPosInOptix(CONFERENCE_EMITTER)
        r.setSphereCenterInOptix(CONFERENCE_LISTENER, 0.0)
        first = r.render_bands(irs=tuple(bufs[:2]), acoustics=False)
        assert r.render_bands(irs=False, acoustics=False)["stats"]["warm_launches"].tolist() == [0] * BANDS

        def combine(t):
            return r.combine_bands(tuple(bufs[:2]), d_g[t], n_bands=BANDS, ir_len=n, out=tuple(bufs[2:]), taps=t)["ms"]

        def sync():
            assert lib().arx_copy_ir(r.handle, None, None, n) == 0

        def chain_device():
            t0 = time.perf_counter()
            r.render_bands(irs=tuple(bufs[:2]), acoustics=False)
            combine(TAPS[-1])
            r.set_ir_device(bufs[2].ptr, bufs[3].ptr)
            sync()
            return (time.perf_counter() - t0) * 1e3

        def chain_host():
            t0 = time.perf_counter()
            L, R = r.render_bands(irs=True, acoustics=False)["ir"]
            r.set_ir(fft_combine(L, g[TAPS[-1]]), fft_combine(R, g[TAPS[-1]]))
            sync()
            return (time.perf_counter() - t0) * 1e3

        legs = {f"C{t}_combine_device_ms": (lambda t=t: combine(t)) for t in TAPS}
        legs["D_chain_on_device_host_ms"] = chain_device
        legs["H_chain_through_host_host_ms"] = chain_host
        rounds = {name: [] for name in legs}
        for rnd in range(ROUNDS + 1):
            for name, fn in legs.items():
                ms = [fn() for _ in range(REPS)]
                if rnd:
                    rounds[name].append(round(float(np.median(ms)), 4))
        med = {name: float(np.median(v)) for name, v in rounds.items()}
        # the device's result against the host leg's, for scale (the FFT route rounds differently)
        combine(TAPS[-1])
        dev = bufs[2].to_numpy(np.float32, n)
        host = fft_combine(bufs[0].to_numpy(np.float32, BANDS * n).reshape(BANDS, n), g[TAPS[-1]])
        st = r.stats()
        with open(os.path.join(ROOT, "profiles", "r15", "bands.json")) as fh:
            r15 = json.load(fh)
        doc = {"tool": "tools/band_synth_time.py",
               "commit": a.commit or tree_id(),
               "method": f"C legs: the call's device time (event pair around its copies and kernel), every buffer device-resident; "
                         f"D and H: host clock around the chain, ending in a synchronise; one discarded round, then {ROUNDS} "
                         f"alternating rounds, each the median of {REPS} calls",
               "workload": {"shape": "c3", "rays": int(np.prod(SETTINGS["rays"])), "max_bounces": SETTINGS["max_bounces"],
                            "bands": BANDS, "ir_len": int(n), "sample_rate": sr, "crossovers_hz": [round(float(x), 2) for x in xs],
                            "triangles": int(conf.n_tris)},
               "guard": {"tree_hash": f"{int(st['tree_hash']):016x}",
                         "trace_kernel_id": f"{int(lib().arx_trace_kernel_id()):016x}",
                         "conv_kernel_id": f"{int(lib().arx_conv_kernel_id()):016x}"},
               "band_queries": [int(q) for q in first["stats"]["queries"]],
               "ms": {name: {"rounds": v, "median": med[name]} for name, v in rounds.items()},
               "combine": {str(t): {"fma": fma_count(n, t),
                                    "fma_per_s": round(fma_count(n, t) / (med[f"C{t}_combine_device_ms"] * 1e-3), 1),
                                    "scratch_bytes": int(lib().arx_debug_combine_bytes(n, BANDS, t))} for t in TAPS},
               "host_over_device_chain": round(med["H_chain_through_host_host_ms"] / med["D_chain_on_device_host_ms"], 3),
               "fft_result_vs_device": {"max_abs_diff": float(np.abs(dev.astype(np.float64) - host).max()),
                                        "max_abs": float(np.abs(dev).max())},
               "r15_render_bands_ms": {k: v["median"] for k, v in r15["ms"].items()}}
    finally:
        for b in bufs + list(d_g.values()):
            b.close()
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
