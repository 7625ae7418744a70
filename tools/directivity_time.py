#!/usr/bin/env python3
"""What a directed source costs on the band replays, and what turning it costs.

    python tools/directivity_time.py [--out FILE] [--tree DIR] [--undirected-only] [--no-loop] [--commit TEXT]

The workload is C3 (1M rays x 16 bounces, 48 kHz x 2 s, the conference stand-in) with 8 bands: the table is
PCG64(7)'s uniform(0.05, 0.9, (8, T)) as f32 and the scene's absorption its column minimum (tools/bands_time.py's).
The pattern is cardioid_cube(64, orders 0..7): omnidirectional in the lowest band, narrowing with the band.  The
path cache is warm.  ROUNDS alternating rounds of REPS calls each, after one discarded round, of
  (U) arx_render_bands, no pattern: the call's device time, no IRs, no acoustics;
  (D) the same call with the pattern installed and its gain plane made: the directed kernels alone;
  (T) a turn of the source: arx_set_source_orientation to another yaw, then the call -- the gain kernel and the
      directed replay, in the call's device time;
  (G) the gain kernel alone: after a turn, arx_debug_directivity_plane(0, 0), on the host clock -- one launch
      and one synchronisation, so an upper bound; T - D is the same figure from device times;
  (LU), (LD) arx_render_listener_bands at 64 poses on a grid through the room, undirected and directed, no IRs,
      no acoustics (REPS_L calls a round).
As context, once a round on the host clock: what a turn replaces without this feature, arx_set_scene (a host SBVH
build of an edited scene) and two renders (the second records).  --undirected-only runs (U) and (LU) alone and needs none of the new
entry points: with --tree pointing at a checkout of the parent commit it measures the parent's undirected figures
on the same machine.  Writes profiles/r21/directivity.json by default."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROUNDS, REPS, REPS_L, BANDS, POSES = 3, 10, 3, 8, 64
SETTINGS = dict(rays=(100, 100, 100), sample_rate=48000, base_power=3.62, max_bounces=16, hrtf_absorption_rate=1.0,
                ir_length_in_seconds=2)


def tree_id(root):
    """HEAD, marked when the working tree differs from it; "unknown" outside a git checkout."""
    head = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode != 0:
        return "unknown"
    dirty = subprocess.run(["git", "-C", root, "status", "--porcelain"], capture_output=True, text=True).stdout.strip()
    return head.stdout.strip() + (" + uncommitted changes" if dirty else "")


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r21", "directivity.json"))
    ap.add_argument("--tree", default=here, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--undirected-only", action="store_true", help="legs U and LU alone (runs on the parent commit)")
    ap.add_argument("--no-loop", action="store_true", help="skip the arx_set_scene + two renders context leg")
    ap.add_argument("--commit", help="what to record as the measured tree where git cannot say (a copy without .git)")
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    sys.path.insert(0, root)

    import audiorenderingv2_amd as arx
    from audiorenderingv2_amd import AudioRenderer, RenderSettings, conference_standin, listener_grid, receiver_local
    from audiorenderingv2_amd._lib import lib
    from audiorenderingv2_amd.scene import CONFERENCE_EMITTER, CONFERENCE_LISTENER, Scene

    assert os.path.dirname(os.path.dirname(os.path.abspath(arx.__file__))) == root
    conf = conference_standin()
    table = np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.9, (BANDS, conf.n_tris)).astype(np.float32)
    scene = Scene(conf.tri_v, table.min(axis=0), conf.names, table)
    # a scene edit, as modelling a pattern in the scene would need one: another absorption, so another host build
    edited = Scene(conf.tri_v, table.min(axis=0) * np.float32(0.999), conf.names, table)
    lo, hi = conf.tri_v.reshape(-1, 3).min(axis=0), conf.tri_v.reshape(-1, 3).max(axis=0)
    poses = listener_grid(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), 8, 8, CONFERENCE_LISTENER[1])
    assert len(poses) == POSES
    r = AudioRenderer(RenderSettings(**SETTINGS), scene=scene, receiver=receiver_local())
    try:
        r.setEmitterPosInOptix(CONFERENCE_EMITTER)
        r.setSphereCenterInOptix(CONFERENCE_LISTENER, 0.0)
        for _ in range(3):
            r.render()
        assert r.path_cache_state()["state"] == "replayed"
        first = r.render_bands(irs=False, acoustics=False)
        assert first["stats"]["warm_launches"].tolist() == [0] * BANDS
        directed = not a.undirected_only
        yaw = [0.0]

        installed = [False]

        def set_pattern(on):  # only on a change: installing a pattern makes the next call remake the plane
            if directed and installed[0] != on:
                r.set_source_directivity(cube if on else None)
                installed[0] = on

        def bands(on):
            set_pattern(on)
            return r.render_bands(irs=False, acoustics=False)["ms"]

        def turn():
            yaw[0] = 37.0 if yaw[0] == 0.0 else 0.0
            r.set_source_orientation(yaw[0])

        def turned_bands():
            set_pattern(True)
            turn()
            return r.render_bands(irs=False, acoustics=False)["ms"]

        def gain_alone():
            set_pattern(True)
            turn()
            t0 = time.perf_counter()
            r.directivity_plane(0, 0)
            return (time.perf_counter() - t0) * 1e3

        def listeners(on):
            set_pattern(on)
            return r.render_listener_bands(poses, irs=False, acoustics=False)["ms"]

        legs = {"U_bands_undirected": (lambda: bands(False), REPS), "LU_listener_bands_undirected": (lambda: listeners(False), REPS_L)}
        if directed:
            cube = arx.cardioid_cube(64, np.arange(BANDS))
            made0 = int(lib().arx_debug_directivity_planes_made(r.handle))
            legs.update({"D_bands_directed": (lambda: bands(True), REPS), "T_turn_and_bands_directed": (turned_bands, REPS),
                         "G_gain_kernel_host_clock": (gain_alone, REPS),
                         "LD_listener_bands_directed": (lambda: listeners(True), REPS_L)})
        rounds = {name: [] for name in legs}
        loop_s = []
        for rnd in range(ROUNDS + 1):
            for name, (fn, reps) in legs.items():
                fn()  # the leg's own first call settles what the leg before left (a plane made, a pattern dropped)
                ms = [fn() for _ in range(reps)]
                if rnd:
                    rounds[name].append(round(float(np.median(ms)), 4))
            if rnd and not a.no_loop:  # what a turn replaces: a scene edit, a trace and a recording
                set_pattern(False)
                t0 = time.perf_counter()
                r.set_scene(edited)
                r.render()
                r.render()
                r.stats()
                loop_s.append(round(time.perf_counter() - t0, 4))
                r.set_scene(scene)  # untimed: the legs' own scene again, traced, recorded, replayed
                for _ in range(3):
                    r.render()
                r.render_bands(irs=False, acoustics=False)
        med = {name: float(np.median(v)) for name, v in rounds.items()}
        st = r.stats()
        doc = {"tool": "tools/directivity_time.py",
               "commit": a.commit or tree_id(root),
               "method": f"device time (event pairs) of each call unless named host clock; path cache warm; one discarded "
                         f"round, then {ROUNDS} alternating rounds, each the median of {REPS} calls ({REPS_L} for the "
                         f"listener batch)",
               "workload": {"shape": "c3", "rays": int(np.prod(SETTINGS["rays"])), "max_bounces": SETTINGS["max_bounces"],
                            "bands": BANDS, "triangles": int(conf.n_tris), "listener_poses": POSES,
                            "pattern": "cardioid_cube(64, orders 0..7)" if directed else None},
               "guard": {"tree_hash": f"{int(st['tree_hash']):016x}",
                         "trace_kernel_id": f"{int(lib().arx_trace_kernel_id()):016x}"},
               "ms": {name: {"rounds": v, "median": med[name]} for name, v in rounds.items()}}
        if directed:
            U, D, T = med["U_bands_undirected"], med["D_bands_directed"], med["T_turn_and_bands_directed"]
            after = r.render_bands(irs=False, acoustics=False)
            doc.update({"directed_over_undirected": round(D / U, 4),
                        "gain_kernel_ms_from_device_times": round(T - D, 4),
                        "listener_directed_over_undirected": round(med["LD_listener_bands_directed"] /
                                                                   med["LU_listener_bands_undirected"], 4),
                        "directivity_bytes": int(lib().arx_debug_directivity_bytes(int(np.prod(SETTINGS["rays"])), BANDS, 64)),
                        "planes_made": int(lib().arx_debug_directivity_planes_made(r.handle)) - made0,
                        "pattern_power": [round(float(p), 6) for p in arx.directivity_power(cube)],
                        "undirected_band_queries": [int(q) for q in first["stats"]["queries"]],
                        "directed_band_queries": [int(q) for q in after["stats"]["queries"]]})
        if loop_s:
            doc["turn_replaced_set_scene_two_renders_host_s"] = {"rounds": loop_s, "median": float(np.median(loop_s))}
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
