#!/usr/bin/env python3
"""arx_render_listener_bands against the loop it replaces, on the same library.

    python tools/listener_bands_time.py [--shape c3|small|all] [--out FILE] [--once SHAPE] [--commit TEXT]

Two shapes on the conference stand-in, 8 bands (the table is PCG64(7)'s uniform(0.05, 0.9, (8, T)) as f32, the
scene's absorption its column minimum), the poses listener_grid's over the audience plane at 1.2 m:
  c3     64 poses (8 x 8), 1M rays x 16 bounces, 48 kHz x 2 s
  small  256 poses (16 x 16), 36 000 rays x 8 bounces, 16 kHz x 1 s
The path cache is warm with its filter state.  A pass answers every pose once with acoustics and ends
synchronised; it is timed on the host clock.  Legs:
  call        arx_render_listener_bands, acoustics, no IRs
  loop        per pose arx_set_listener + arx_render_bands, acoustics, no IRs
  call_bb     the call with a 255-tap filter bank, the broadband set into device memory
  loop_bb     per pose arx_set_listener + arx_render_bands into device buffers + arx_combine_bands on them
ROUNDS alternating rounds after one discarded; a round's figure is one pass.  Nothing here asserts a speed:
the ratios are reported as measured.  --once SHAPE runs one call and exits (for a kernel trace of its own).
Writes profiles/r17/listener_bands.json by default."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, BANDS, TAPS = 3, 8, 255
SHAPES = {
    "c3": dict(settings=dict(rays=(100, 100, 100), sample_rate=48000, base_power=3.62, max_bounces=16,
                             hrtf_absorption_rate=1.0, ir_length_in_seconds=2), grid=(8, 8)),
    "small": dict(settings=dict(rays=(60, 60, 10), sample_rate=16000, base_power=3.62, max_bounces=8,
                                hrtf_absorption_rate=0.5), grid=(16, 16)),
}


def tree_id():
    """HEAD, marked when the working tree differs from it; "unknown" outside a git checkout."""
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode != 0:
        return "unknown"
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    return head.stdout.strip() + (" + uncommitted changes" if dirty else "")


def setup(shape):
    from audiorenderingv2_amd import AudioRenderer, RenderSettings, conference_standin, listener_grid, receiver_local
    from audiorenderingv2_amd.scene import CONFERENCE_EMITTER, CONFERENCE_LISTENER, Scene

    cfg = SHAPES[shape]
    conf = conference_standin()
    table = np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.9, (BANDS, conf.n_tris)).astype(np.float32)
    scene = Scene(conf.tri_v, table.min(axis=0), conf.names, table)
    r = AudioRenderer(RenderSettings(**cfg["settings"]), scene=scene, receiver=receiver_local())
    r.setEmitterPosInOptix(CONFERENCE_EMITTER)
    r.setSphereCenterInOptix(CONFERENCE_LISTENER, 0.0)
    r.set_timing(False)
    poses = listener_grid((-8.0, 0.0, -4.0), (8.0, 0.0, 4.0), cfg["grid"][0], cfg["grid"][1], 1.2)
    for _ in range(3):
        r.render()
    assert r.path_cache_state()["state"] == "replayed"
    return r, poses, conf


def measure(shape):
    from audiorenderingv2_amd import DeviceBuffer, band_filters, octave_crossovers
    from audiorenderingv2_amd._lib import lib

    r, poses, conf = setup(shape)
    k, n = len(poses), r.ir_length
    sr = SHAPES[shape]["settings"]["sample_rate"]
    g = band_filters(sr, octave_crossovers([63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, sr / 4.0]), TAPS)
    bufs = [DeviceBuffer(0, BANDS * n * 4) for _ in range(2)] + [DeviceBuffer(0, n * 4) for _ in range(2)]
    bb = [DeviceBuffer(0, k * n * 4) for _ in range(2)]
    try:
        first = r.render_listener_bands(poses, acoustics=True)
        assert not first["stats"]["warm_launches"].any()
        routes = first["stats"]["route"][:, 0]

        def loop(combine):
            for p in poses:
                r.setSphereCenterInOptix(p[:3], float(p[3]))
                if combine:
                    r.render_bands(irs=tuple(bufs[:2]), acoustics=True)
                    r.combine_bands(tuple(bufs[:2]), g, n_bands=BANDS, ir_len=n, out=tuple(bufs[2:]))
                else:
                    r.render_bands(irs=False, acoustics=True)

        legs = {"call": lambda: r.render_listener_bands(poses, acoustics=True),
                "loop": lambda: loop(False),
                "call_bb": lambda: r.render_listener_bands(poses, acoustics=True, filters=g, broadband=tuple(bb)),
                "loop_bb": lambda: loop(True)}
        rounds = {name: [] for name in legs}
        for rnd in range(ROUNDS + 1):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()  # every leg ends synchronised: the call once, the loop after every pose
                ms = (time.perf_counter() - t0) * 1e3
                if rnd:
                    rounds[name].append(round(ms, 3))
        med = {name: float(np.median(v)) for name, v in rounds.items()}
        # the loop's own answer is the call's: the figures compare equal work
        r.setSphereCenterInOptix(poses[-1][:3], float(poses[-1][3]))
        last = r.render_bands(irs=False, acoustics=False)["stats"]
        assert [int(q) for q in last["queries"]] == [int(q) for q in first["stats"]["queries"][-1]]
        st = r.stats()
        return {"poses": k, "rays": int(np.prod(SHAPES[shape]["settings"]["rays"])),
                "max_bounces": SHAPES[shape]["settings"]["max_bounces"], "ir_len": n, "bands": BANDS, "taps": TAPS,
                "triangles": int(conf.n_tris),
                "batched_poses": int((routes == 0).sum()), "single_poses": int((routes == 1).sum()),
                "candidate_rays_mean": float(first["stats"]["candidate_rays"][:, 0].mean()),
                "scratch_bytes_per_listener": int(lib().arx_debug_listener_band_bytes(
                    int(np.prod(SHAPES[shape]["settings"]["rays"])), n, 1019, 1020, BANDS, 1)
                    - lib().arx_debug_listener_band_bytes(int(np.prod(SHAPES[shape]["settings"]["rays"])), n, 1019, 1020, BANDS, 0)),
                "call_device_ms": round(first["ms"], 3),
                "guard": {"tree_hash": f"{int(st['tree_hash']):016x}",
                          "trace_kernel_id": f"{int(lib().arx_trace_kernel_id()):016x}"},
                "ms": {name: {"rounds": v, "median": med[name], "per_pose": round(med[name] / k, 4)} for name, v in rounds.items()},
                "loop_over_call": round(med["loop"] / med["call"], 3),
                "loop_bb_over_call_bb": round(med["loop_bb"] / med["call_bb"], 3)}
    finally:
        for b in bufs + bb:
            b.close()
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["c3", "small", "all"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "listener_bands.json"))
    ap.add_argument("--once", choices=list(SHAPES), help="one call of this shape, nothing timed or written")
    ap.add_argument("--commit", help="what to record as the measured tree where git cannot say (a copy without .git)")
    a = ap.parse_args()
    if a.once:
        r, poses, _ = setup(a.once)
        try:
            out = r.render_listener_bands(poses, acoustics=True)
            print(json.dumps({"shape": a.once, "ms": out["ms"]}), flush=True)
        finally:
            r.close()
        return 0
    shapes = list(SHAPES) if a.shape == "all" else [a.shape]
    doc = {"tool": "tools/listener_bands_time.py", "commit": a.commit or tree_id(),
           "method": f"host clock around passes that end synchronised; path cache warm with filter state; one discarded "
                     f"round, then {ROUNDS} alternating rounds of one pass per leg",
           "shapes": {s: measure(s) for s in shapes}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
