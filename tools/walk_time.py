#!/usr/bin/env python3
"""What a walk-through convolution costs (arx_convolute_walk) against the loop it stands for.

    python tools/walk_time.py [--out FILE] [--tiles 4,8,16]
    python tools/walk_time.py --one even          # warm-up and one call of a schedule: for a kernel trace

Shape: 48 kHz, 2-s IR, blocks of 4096 frames, 60 s of the clapper recording looped -- 704 input blocks plus
24 tail blocks -- over 64 synthetic IR pairs, everything in device memory.  Schedules:
  one    one IR throughout, no fade;
  even   arx_walk_even_schedule over the 64 IRs, a whole-block fade (63 transition blocks);
  worst  a new IR on every block, a whole-block fade (727 transition blocks).
Per schedule, ROUNDS alternating rounds after one discarded round of
  call   arx_convolute_walk: its device time (*ms) and the host clock around it;
  loop   a fresh stream, then arx_set_ir_device at every change + arx_stream_process_device per block, the
         host clock from the first call to a final synchronisation -- the route a caller has without the call;
and whether the two outputs are equal.  --tiles: the call's device time again with the multiply-accumulate
tile forced to each value (arx_debug_set_walk_tile), ROUNDS alternating rounds.  Writes medians, spreads and
the loop / call ratios (profiles/r13/walk.json by default).  Nothing here asserts a time."""
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
SR, SECS, B, SECONDS, N_IRS = 48000, 2, 4096, 60, 64


def schedules(n_frames, n):
    from audiorenderingv2_amd import walk_blocks, walk_schedule

    nb = walk_blocks(n_frames, B, n)
    return {"one": (np.zeros(nb, np.int32), 0), "even": (walk_schedule(n_frames, B, n, N_IRS), B),
            "worst": ((np.arange(nb) % N_IRS).astype(np.int32), B)}


class Bench:
    def __init__(self):
        from audiorenderingv2_amd import AudioRenderer, DeviceBuffer, RenderSettings
        from audiorenderingv2_amd.scene import reference_audio

        self.r = AudioRenderer(RenderSettings(rays=(1, 1, 1), sample_rate=SR, ir_length_in_seconds=SECS))
        self.r.set_timing(False)
        self.n = n = self.r.ir_length
        clap, sr = reference_audio("clapper")
        assert sr == SR
        x = np.resize(clap.astype(np.float64), SECONDS * SR)
        rng = np.random.default_rng(0)
        irs = np.zeros((2, N_IRS, n), np.float32)
        for ear in range(2):
            for j in range(N_IRS):  # rendered-like sparse IRs, as tools/conv_once.py makes them
                irs[ear, j, rng.integers(0, n, 20000)] = rng.exponential(1e-4, 20000).astype(np.float32)
        self.n_frames = x.size
        self.sched = schedules(x.size, n)
        self.nb = len(self.sched["one"][0])
        self.dl, self.dr = DeviceBuffer.from_numpy(0, irs[0]), DeviceBuffer.from_numpy(0, irs[1])
        self.dx = DeviceBuffer.from_numpy(0, x)
        self.out_call, self.out_loop = (DeviceBuffer(0, 2 * self.nb * B * 8) for _ in range(2))

    def call(self, name):
        sched, fade = self.sched[name]
        t0 = time.perf_counter()
        res = self.r.convolute_walk((self.dl, self.dr), sched, self.dx, B, fade, "hann", n_irs=N_IRS,
                                    n_frames=self.n_frames, out=self.out_call)
        return res["ms"], (time.perf_counter() - t0) * 1e3

    def loop(self, name):
        from audiorenderingv2_amd import LiveStream

        sched, fade = self.sched[name]
        sched = sched.tolist()
        r, n = self.r, self.n
        s = LiveStream(r, B, crossfade_frames=fade, fade="hann")
        r.stats()
        t0 = time.perf_counter()
        for b, j in enumerate(sched):
            if b == 0 or j != sched[b - 1]:
                r.set_ir_device(self.dl.ptr + j * n * 4, self.dr.ptr + j * n * 4)
            m = min(max(self.n_frames - b * B, 0), B)
            s.process_device(self.dx.ptr + b * B * 8 if m else 0, m, self.out_loop.ptr + 2 * b * B * 8)
        r.stats()  # synchronises the renderer's stream
        ms = (time.perf_counter() - t0) * 1e3
        s.close()
        return ms

    def equal(self):
        return bool(np.array_equal(self.out_call.to_numpy(np.float64), self.out_loop.to_numpy(np.float64)))

    def close(self):
        for b in (self.dl, self.dr, self.dx, self.out_call, self.out_loop):
            b.close()
        self.r.close()


def stat(v):
    return {"runs": [round(t, 4) for t in v], "median": round(float(np.median(v)), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


def measure(tiles):
    bench = Bench()
    try:
        t_end = time.perf_counter() + 1.0  # past the clock ramp
        while time.perf_counter() < t_end:
            bench.call("even")
        out = {"blocks": bench.nb, "input_blocks": -(-bench.n_frames // B), "irs": N_IRS, "schedules": {}}
        runs = {name: {"call_device": [], "call_wall": [], "loop_wall": []} for name in bench.sched}
        for rnd in range(ROUNDS + 1):
            for name in bench.sched:
                dev, wall = bench.call(name)
                loop = bench.loop(name)
                if rnd:
                    runs[name]["call_device"].append(dev)
                    runs[name]["call_wall"].append(wall)
                    runs[name]["loop_wall"].append(loop)
        for name in bench.sched:
            bench.call(name)
            st = bench.r.walk_state()
            bench.loop(name)
            leg = {"fade_frames": int(bench.sched[name][1]), "transitions": st["transitions"],
                   "irs_transformed": st["irs_transformed"], "tiles": st["tiles"], "scratch_bytes": st["scratch_bytes"],
                   "equal": bench.equal(), "ms": {k: stat(v) for k, v in runs[name].items()}}
            leg["loop_over_call_wall"] = round(leg["ms"]["loop_wall"]["median"] / leg["ms"]["call_wall"]["median"], 2)
            leg["loop_over_call_device"] = round(leg["ms"]["loop_wall"]["median"] / leg["ms"]["call_device"]["median"], 2)
            leg["loop_min_over_call_wall_max"] = round(leg["ms"]["loop_wall"]["min"] / leg["ms"]["call_wall"]["max"], 2)
            out["schedules"][name] = leg
        if tiles:
            sweep = {name: {t: [] for t in tiles} for name in bench.sched}
            for rnd in range(ROUNDS + 1):
                for t in tiles:
                    bench.r.set_walk_tile(t)
                    for name in bench.sched:
                        dev, _ = bench.call(name)
                        if rnd:
                            sweep[name][t].append(dev)
            bench.r.set_walk_tile(0)
            out["tile_sweep_call_device_ms"] = {name: {str(t): stat(v) for t, v in by.items()} for name, by in sweep.items()}
        return out
    finally:
        bench.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "walk.json"))
    ap.add_argument("--tiles", default="4,8,16", help="forced tiles to sweep ('' for none)")
    ap.add_argument("--one", help="warm-up and one call of this schedule, nothing written")
    a = ap.parse_args()
    if a.one:
        bench = Bench()
        try:
            bench.call(a.one)
            dev, wall = bench.call(a.one)
            print(json.dumps({"schedule": a.one, "device_ms": dev, "wall_ms": wall, **bench.r.walk_state()}))
        finally:
            bench.close()
        return
    g = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    doc = {"tool": "tools/walk_time.py", "commit": g.stdout.strip() if g.returncode == 0 else "unknown",
           "shape": {"sample_rate": SR, "ir_seconds": SECS, "block_frames": B, "seconds": SECONDS},
           "method": f"everything in device memory, per-launch events off; one discarded round, then {ROUNDS} rounds of "
                     "call and loop in turn per schedule; call_device: the call's *ms (a pair of events around its copies "
                     "and launches); call_wall / loop_wall: the host clock around work that ends synchronised",
           "legs": {"call": "arx_convolute_walk",
                    "loop": "fresh stream; arx_set_ir_device at every change + arx_stream_process_device per block; "
                            "one synchronisation at the end"}}
    doc.update(measure([int(t) for t in a.tiles.split(",") if t]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
