#!/usr/bin/env python3
"""What a batch of listeners costs (arx_render_listeners) against today's loops, on the conference stand-in.

    python tools/listeners_time.py [--out FILE] [--shapes c3,small]
    python tools/listeners_time.py --one c3        # warm-up and one call of (C): for a kernel trace

Two shapes: C3 (1M rays x 16 bounces, 48 kHz x 2 s) with K = 64 poses of an 8 x 8 grid over the room, and
SMALL (36 000 rays x 8, 16 kHz) with K = 256 (16 x 16).  The path cache is warm (three plain renders), the
per-launch timing events are off, and every leg is the host clock around one pass over the K poses that
ends synchronised.  ROUNDS alternating rounds, after one discarded round past the clock ramp, of
  (A) the loop with the analysis: set listener, arx_render, arx_analyze_ir, arx_get_acoustics x 3, per pose;
  (B) the loop of set listener + arx_render alone, one synchronisation at the end;
  (C) arx_render_listeners with acoustics, no IR copies;
  (D) the same with the IRs copied to device memory.
Writes medians and spreads (profiles/r12/listeners.json by default).  Nothing here asserts a time."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 3
SHAPES = {
    "c3": dict(settings=dict(rays=(100, 100, 100), sample_rate=48000, base_power=3.62, max_bounces=16,
                             hrtf_absorption_rate=1.0, ir_length_in_seconds=2), grid=(8, 8)),
    "small": dict(settings=dict(rays=(60, 60, 10), sample_rate=16000, base_power=3.62, max_bounces=8,
                                hrtf_absorption_rate=0.5), grid=(16, 16)),
}


def setup(shape):
    from audiorenderingv2_amd import AudioRenderer, RenderSettings, conference_standin, listener_grid, receiver_local
    from audiorenderingv2_amd.scene import CONFERENCE_EMITTER, CONFERENCE_LISTENER

    cfg = SHAPES[shape]
    r = AudioRenderer(RenderSettings(**cfg["settings"]), scene=conference_standin(), receiver=receiver_local())
    r.setEmitterPosInOptix(CONFERENCE_EMITTER)
    r.setSphereCenterInOptix(CONFERENCE_LISTENER, 0.0)
    r.set_timing(False)
    poses = listener_grid((-8.0, 0.0, -4.0), (8.0, 0.0, 4.0), cfg["grid"][0], cfg["grid"][1], 1.2)
    for _ in range(3):
        r.render()
    assert r.path_cache_state()["state"] == "replayed"
    return r, poses


def measure(shape):
    from audiorenderingv2_amd import DeviceBuffer
    from audiorenderingv2_amd._lib import check, lib

    r, poses = setup(shape)
    k, n = len(poses), r.ir_length
    dl, dr = DeviceBuffer(0, k * n * 4), DeviceBuffer(0, k * n * 4)

    def leg_a():
        for p in poses:
            r.setSphereCenterInOptix(p[:3], p[3])
            check(lib().arx_render(r.handle, None))
            r.analyze_ir()
            for ch in ("left", "right", "sum"):
                r.acoustics(ch)

    def leg_b():
        for p in poses:
            r.setSphereCenterInOptix(p[:3], p[3])
            check(lib().arx_render(r.handle, None))
        r.stats()

    last = {}

    def leg_c():
        last["c"] = r.render_listeners(poses, irs=False, acoustics=True)

    def leg_d():
        last["d"] = r.render_listeners(poses, irs=(dl, dr), acoustics=True)

    legs = {"A_loop_with_analysis": leg_a, "B_loop_render_only": leg_b, "C_batch_acoustics": leg_c,
            "D_batch_acoustics_device_irs": leg_d}
    runs = {name: [] for name in legs}
    try:
        t_end = time.perf_counter() + 1.0  # past the clock ramp
        while time.perf_counter() < t_end:
            leg_b()
        for rnd in range(ROUNDS + 1):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                if rnd:
                    runs[name].append(round((time.perf_counter() - t0) * 1e3, 4))
        st = r.stats()
        out = {"listeners": k, "rays": int(np.prod(SHAPES[shape]["settings"]["rays"])),
               "guard": {"workload": shape, "tree_hash": f"{int(st['tree_hash']):016x}", "trace_vgprs": int(st["trace_vgprs"]),
                         "trace_kernel_id": f"{int(lib().arx_trace_kernel_id()):016x}"},
               "routes_batched": int((last["c"]["stats"]["route"] == 0).sum()),
               "candidate_rays_median": int(np.median(last["c"]["stats"]["candidate_rays"])),
               "receiver_hits_median": int(np.median(last["c"]["stats"]["receiver_hits"])),
               "batch_device_ms": {"C": round(last["c"]["ms"], 4), "D": round(last["d"]["ms"], 4)},
               "ms": {name: {"runs": v, "median": float(np.median(v)), "min": min(v), "max": max(v),
                             "per_listener_us": round(float(np.median(v)) / k * 1e3, 2)} for name, v in runs.items()}}
        b, c = out["ms"]["B_loop_render_only"]["median"], out["ms"]["C_batch_acoustics"]["median"]
        out["C_over_B"] = round(c / b, 4)
        out["C_over_A"] = round(c / out["ms"]["A_loop_with_analysis"]["median"], 4)
        return out
    finally:
        dl.close()
        dr.close()
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "listeners.json"))
    ap.add_argument("--shapes", default="c3,small")
    ap.add_argument("--one", help="warm-up and one call of (C) at this shape, nothing written")
    a = ap.parse_args()
    if a.one:
        r, poses = setup(a.one)
        try:
            out = r.render_listeners(poses, irs=False, acoustics=True)
            print(json.dumps({"shape": a.one, "ms": out["ms"], "batched": int((out["stats"]["route"] == 0).sum())}))
        finally:
            r.close()
        return
    g = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    doc = {"tool": "tools/listeners_time.py", "commit": g.stdout.strip() if g.returncode == 0 else "unknown",
           "method": f"host clock around one pass over K poses ending synchronised; path cache warm, per-launch events "
                     f"off; one discarded round, then {ROUNDS} rounds of the legs in turn",
           "legs": {"A": "loop: set listener, arx_render, arx_analyze_ir, arx_get_acoustics x 3",
                    "B": "loop: set listener, arx_render; one synchronisation at the end",
                    "C": "arx_render_listeners, acoustics, no IR copies",
                    "D": "arx_render_listeners, acoustics, IRs to device memory"}}
    for shape in a.shapes.split(","):
        doc[shape] = measure(shape)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
