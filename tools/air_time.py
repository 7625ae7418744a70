#!/usr/bin/env python3
"""What air absorption costs on the band replays.

    python tools/air_time.py [--out FILE] [--tree DIR] [--no-air-only] [--commit TEXT]

The workload is C3 (1M rays x 16 bounces, 48 kHz x 2 s, the conference stand-in) with 8 bands and energy_thres 0:
the table is PCG64(7)'s uniform(0.05, 0.9, (8, T)) as f32 and the scene's absorption its column minimum
(tools/bands_time.py's).  The coefficients are ISO 9613-1's pure-tone values at 20 C, 50 %, 101.325 kPa for the
octave centres 63 Hz .. 8 kHz.  The path cache is warm.  ROUNDS alternating rounds of REPS calls each, after one
discarded round, of
  (P) arx_render_bands, no coefficients: the call's device time, no IRs, no acoustics;
  (A) the same call with the coefficients installed and the attenuation table made: the AIR kernels alone;
  (C) a coefficient change, then the call: the host loop and the blocking upload lie in front of the call's device
      time, so this leg is on the host clock, as is (PH), the plain call on the host clock, for its difference;
  (LP), (LA) arx_render_listener_bands at 64 poses on a grid through the room, without and with air, no IRs, no
      acoustics (REPS_L calls a round).
--no-air-only runs (P), (PH) and (LP) alone and needs none of the new entry points: with --tree pointing at a
checkout of the parent commit it measures the parent's figures on the same machine.  Writes profiles/r23/air.json by
default."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROUNDS, REPS, REPS_L, BANDS, POSES = 3, 10, 3, 8, 64
SETTINGS = dict(rays=(100, 100, 100), sample_rate=48000, base_power=3.62, max_bounces=16, hrtf_absorption_rate=1.0,
                ir_length_in_seconds=2, energy_thres=0.0)
CENTRES = [63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0]


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
    ap.add_argument("--out", default=os.path.join(here, "profiles", "r23", "air.json"))
    ap.add_argument("--tree", default=here, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--no-air-only", action="store_true", help="legs P, PH and LP alone (runs on the parent commit)")
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
        with_air = not a.no_air_only
        installed = [False]
        flip = [False]

        def set_air(on):  # only on a change: new coefficients make the next call remake the table
            if with_air and installed[0] != on:
                r.set_air_absorption(alpha if on else None)
                installed[0] = on

        def bands(on):
            set_air(on)
            return r.render_bands(irs=False, acoustics=False)["ms"]

        def bands_host(on):
            set_air(on)
            t0 = time.perf_counter()
            r.render_bands(irs=False, acoustics=False)
            return (time.perf_counter() - t0) * 1e3

        def changed_bands_host():
            flip[0] = not flip[0]
            r.set_air_absorption(alpha * (1.001 if flip[0] else 1.0))
            installed[0] = True
            t0 = time.perf_counter()
            r.render_bands(irs=False, acoustics=False)
            return (time.perf_counter() - t0) * 1e3

        def listeners(on):
            set_air(on)
            return r.render_listener_bands(poses, irs=False, acoustics=False)["ms"]

        legs = {"P_bands_plain": (lambda: bands(False), REPS), "PH_bands_plain_host_clock": (lambda: bands_host(False), REPS),
                "LP_listener_bands_plain": (lambda: listeners(False), REPS_L)}
        if with_air:
            alpha = arx.air_absorption_iso9613(CENTRES, 20.0, 50.0, 101.325)
            made0 = int(lib().arx_debug_air_tables_made(r.handle))
            legs.update({"A_bands_air": (lambda: bands(True), REPS), "AH_bands_air_host_clock": (lambda: bands_host(True), REPS),
                         "C_change_and_bands_air_host_clock": (changed_bands_host, REPS),
                         "LA_listener_bands_air": (lambda: listeners(True), REPS_L)})
        rounds = {name: [] for name in legs}
        for rnd in range(ROUNDS + 1):
            for name, (fn, reps) in legs.items():
                fn()  # the leg's own first call settles what the leg before left (a table made, coefficients dropped)
                ms = [fn() for _ in range(reps)]
                if rnd:
                    rounds[name].append(round(float(np.median(ms)), 4))
        med = {name: float(np.median(v)) for name, v in rounds.items()}
        st = r.stats()
        doc = {"tool": "tools/air_time.py",
               "commit": a.commit or tree_id(root),
               "method": f"device time (event pairs) of each call unless named host clock; path cache warm; one discarded "
                         f"round, then {ROUNDS} alternating rounds, each the median of {REPS} calls ({REPS_L} for the "
                         f"listener batch)",
               "workload": {"shape": "c3", "rays": int(np.prod(SETTINGS["rays"])), "max_bounces": SETTINGS["max_bounces"],
                            "bands": BANDS, "energy_thres": 0.0, "triangles": int(conf.n_tris), "listener_poses": POSES,
                            "alpha_db_per_m": [float(x) for x in alpha] if with_air else None},
               "guard": {"tree_hash": f"{int(st['tree_hash']):016x}",
                         "trace_kernel_id": f"{int(lib().arx_trace_kernel_id()):016x}"},
               "ms": {name: {"rounds": v, "median": med[name]} for name, v in rounds.items()}}
        if with_air:
            set_air(True)
            after = r.render_bands(irs=False, acoustics=False)
            assert after["stats"]["queries"].tolist() == first["stats"]["queries"].tolist()  # air ends no ray
            doc.update({"air_over_plain": round(med["A_bands_air"] / med["P_bands_plain"], 4),
                        "listener_air_over_plain": round(med["LA_listener_bands_air"] / med["LP_listener_bands_plain"], 4),
                        "table_remake_ms_host_clock": round(med["C_change_and_bands_air_host_clock"] -
                                                            med["AH_bands_air_host_clock"], 4),
                        "air_bytes": int(lib().arx_debug_air_bytes(r.ir_length, BANDS)),
                        "tables_made": int(lib().arx_debug_air_tables_made(r.handle)) - made0,
                        "band_receiver_hits": [int(q) for q in after["stats"]["receiver_hits"]],
                        "band_queries": [int(q) for q in after["stats"]["queries"]]})
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
