#!/usr/bin/env python3
"""What eight frequency bands cost in one call (arx_render_bands) against the frame the kernel extends.

    python tools/bands_time.py [--out FILE] [--no-loop] [--commit TEXT]

The workload is C3 (1M rays x 16 bounces, 48 kHz x 2 s, the conference stand-in) with 8 bands: the table is
PCG64(7)'s uniform(0.05, 0.9, (8, T)) as f32 and the scene's absorption its column minimum.  The path cache is
warm and the path filter is off (arx_debug_set_path_filter 0), so arx_render is the unfiltered replayed frame
-- replay_kernel, the code band_replay_kernel extends.  ROUNDS alternating rounds of REPS calls each, after one
discarded round, of
  (R) arx_render: the device time of the replay launch (its clear included), arx_render's own ms;
  (B) arx_render_bands, no IRs, no acoustics: the call's device time (clear, kernel, counter copy);
  (A) arx_render_bands with acoustics (eight analyses), no IRs;
  (I) arx_render_bands with acoustics and the IRs finalized and copied to device memory.
The call must cost less than 8 x (R), or the kernel shares nothing: the tool exits 1 otherwise.  Reported
beside it: B / R and the per-band increment (B - R) / 7.  As context only, once, on the host clock: the loop
the call replaces, 8 x (arx_set_scene with the band's absorption + arx_render), every one a host SBVH build.
Writes profiles/r15/bands.json by default."""
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
SETTINGS = dict(rays=(100, 100, 100), sample_rate=48000, base_power=3.62, max_bounces=16, hrtf_absorption_rate=1.0,
                ir_length_in_seconds=2)


def tree_id():
    """HEAD, marked when the working tree differs from it; "unknown" outside a git checkout."""
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode != 0:
        return "unknown"
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    return head.stdout.strip() + (" + uncommitted changes" if dirty else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "bands.json"))
    ap.add_argument("--no-loop", action="store_true", help="skip the 8 x (arx_set_scene + arx_render) context leg")
    ap.add_argument("--commit", help="what to record as the measured tree where git cannot say (a copy without .git)")
    a = ap.parse_args()

    from audiorenderingv2_amd import AudioRenderer, DeviceBuffer, RenderSettings, conference_standin, receiver_local
    from audiorenderingv2_amd._lib import lib
    from audiorenderingv2_amd.scene import CONFERENCE_EMITTER, CONFERENCE_LISTENER, Scene

    conf = conference_standin()
    table = np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.9, (BANDS, conf.n_tris)).astype(np.float32)
    scene = Scene(conf.tri_v, table.min(axis=0), conf.names, table)
    r = AudioRenderer(RenderSettings(**SETTINGS), scene=scene, receiver=receiver_local())
    n = r.ir_length
    dl, dr = DeviceBuffer(0, BANDS * n * 4), DeviceBuffer(0, BANDS * n * 4)
    try:
        r.setEmitterPosInOptix(CONFERENCE_EMITTER)
        r.setSphereCenterInOptix(CONFERENCE_LISTENER, 0.0)
        r.set_path_filter(False)
        for _ in range(3):
            r.render()
        assert r.path_cache_state()["state"] == "replayed" and not r.path_filter_state()["filtered"]
        first = r.render_bands(irs=False, acoustics=False)
        assert first["stats"]["warm_launches"].tolist() == [0] * BANDS
        legs = {"R_unfiltered_replay_frame": lambda: r.render(),
                "B_bands": lambda: r.render_bands(irs=False, acoustics=False)["ms"],
                "A_bands_acoustics": lambda: r.render_bands(irs=False, acoustics=True)["ms"],
                "I_bands_acoustics_device_irs": lambda: r.render_bands(irs=(dl, dr), acoustics=True)["ms"]}
        rounds = {name: [] for name in legs}
        for rnd in range(ROUNDS + 1):
            for name, fn in legs.items():
                ms = [fn() for _ in range(REPS)]
                if rnd:
                    rounds[name].append(round(float(np.median(ms)), 4))
        med = {name: float(np.median(v)) for name, v in rounds.items()}
        R, B = med["R_unfiltered_replay_frame"], med["B_bands"]
        st = r.stats()
        doc = {"tool": "tools/bands_time.py",
               "commit": a.commit or tree_id(),
               "method": f"device time (event pairs) of each call; path cache warm, path filter off; one discarded round, "
                         f"then {ROUNDS} alternating rounds, each the median of {REPS} calls",
               "workload": {"shape": "c3", "rays": int(np.prod(SETTINGS["rays"])), "max_bounces": SETTINGS["max_bounces"],
                            "bands": BANDS, "triangles": int(conf.n_tris)},
               "guard": {"tree_hash": f"{int(st['tree_hash']):016x}",
                         "trace_kernel_id": f"{int(lib().arx_trace_kernel_id()):016x}",
                         "conv_kernel_id": f"{int(lib().arx_conv_kernel_id()):016x}"},
               "band_queries": [int(q) for q in first["stats"]["queries"]],
               "band_receiver_hits": [int(q) for q in first["stats"]["receiver_hits"]],
               "scene_queries": int(st["queries"]),
               "band_bytes": int(lib().arx_debug_band_bytes(n, conf.n_tris, BANDS)),
               "ms": {name: {"rounds": v, "median": med[name]} for name, v in rounds.items()},
               "bands_over_frame": round(B / R, 4),
               "per_band_increment_ms": round((B - R) / (BANDS - 1), 4),
               "limit_8x_frame_ms": round(8 * R, 4),
               "under_8x": bool(B < 8 * R)}
        if not a.no_loop:
            t0 = time.perf_counter()
            for b in range(BANDS):
                r.set_scene(Scene(conf.tri_v, table[b], conf.names))
                r.render()
            r.stats()
            doc["loop_8x_set_scene_render_host_s"] = round(time.perf_counter() - t0, 3)
    finally:
        dl.close()
        dr.close()
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc), flush=True)
    return 0 if doc["under_8x"] else 1


if __name__ == "__main__":
    sys.exit(main())
