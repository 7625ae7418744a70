"""CPU: the host side of arx_render_listeners (include/arx.h) -- where a chunk's receiver slots live, what
a chunk's scratch costs, the two structs' layout, argument checks that need no device, and the Python
helpers around a batch (listener_grid, write_acoustic_map_json)."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from audiorenderingv2_amd import listener_grid, write_acoustic_map_json
from audiorenderingv2_amd._lib import ArxAcoustics, ArxListenerPose, ArxListenerResult, lib
from audiorenderingv2_amd.renderer import LISTENER_RESULT_DTYPE, _acoustics_dict, write_acoustics_json

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # ARX_ERR_INVALID_ARGUMENT
# a 526 K-node / 620 K-triangle scene and the 1 020-triangle head (its refit tree: one node per leaf pair)
SCENE_NODES, SCENE_TRIS, RECV_TRIS = 526_000, 620_000, 1020
RECV_NODES = 1019


def layout(scene_nodes, scene_tris, recv_nodes, recv_tris, listeners, slot):
    out = (C.c_int64 * 5)()
    st = lib().arx_debug_listener_layout(scene_nodes, scene_tris, recv_nodes, recv_tris, listeners, slot, out)
    return st, tuple(out)


@pytest.mark.parametrize("listeners", [1, 2, 8, 64])
def test_slots_are_disjoint_and_behind_the_renderers_own_receiver(listeners):
    own_nodes = 1 + SCENE_NODES + RECV_NODES
    own_tris = SCENE_TRIS + RECV_TRIS
    node_ranges, tri_ranges, tops = [], [], []
    for j in range(listeners):
        st, (n0, n1, t0, t1, top) = layout(SCENE_NODES, SCENE_TRIS, RECV_NODES, RECV_TRIS, listeners, j)
        assert st == 0
        assert n1 - n0 == RECV_NODES and t1 - t0 == RECV_TRIS
        assert n0 >= own_nodes and t0 >= own_tris and top >= own_nodes
        assert top >= 1024  # the LDS node cache holds at most the buffer's 1024 spare nodes (kNodeCache)
        node_ranges.append((n0, n1))
        tri_ranges.append((t0, t1))
        tops.append(top)
    assert len(set(tops)) == listeners
    node_ranges += [(t, t + 1) for t in tops]
    for ranges in (node_ranges, tri_ranges):
        ranges.sort()
        for a, b in zip(ranges, ranges[1:]):
            assert a[1] <= b[0], (a, b)


def test_tops_clear_the_node_cache_even_for_a_tiny_scene():
    st, (n0, n1, t0, t1, top) = layout(5, 12, RECV_NODES, RECV_TRIS, 2, 0)
    assert st == 0 and top >= 1 + 5 + RECV_NODES and n0 > top


def test_a_scene_whose_last_slot_passes_the_offset_limit_is_rejected():
    # triangle records are addressed with 31-bit byte offsets: (2^31 - 1) // 48 records at the most
    limit = (2**31 - 1) // 48
    fits = limit - RECV_TRIS - 8 * RECV_TRIS
    assert layout(1000, fits, RECV_NODES, RECV_TRIS, 8, 7)[0] == 0
    assert layout(1000, fits + 1, RECV_NODES, RECV_TRIS, 8, 7)[0] == INVALID
    assert layout(1000, fits + 1, RECV_NODES, RECV_TRIS, 8, 0)[0] == INVALID  # the chunk, not the slot
    node_limit = (2**31 - 1) // 64
    assert layout(node_limit, 1000, RECV_NODES, RECV_TRIS, 1, 0)[0] == INVALID
    for bad in [(-1, 0), (0, 1), (65, 0), (8, 8), (8, -1)]:
        assert layout(1000, 1000, RECV_NODES, RECV_TRIS, *bad)[0] == INVALID, bad


def documented_bytes(rays, ir_len, recv_nodes, recv_tris, listeners):
    each = (96 * recv_nodes + 48 * recv_tris + 96 + 112 + 16 * ir_len + 128 + 336 + 8 * ir_len + 16 * rays
            + 16 * math.ceil(rays / 1024) + 16 + 64 * math.ceil(rays / 1024))
    return listeners * each


def test_listener_bytes_is_the_documented_formula_and_monotone():
    f = lib().arx_debug_listener_bytes
    prev = -1
    for listeners in [0, 1, 2, 3, 8, 28, 29, 64]:
        got = f(1_000_000, 96_000, RECV_NODES, RECV_TRIS, listeners)
        assert got == documented_bytes(1_000_000, 96_000, RECV_NODES, RECV_TRIS, listeners)
        assert got > prev
        prev = got
    assert f(36_000, 32_000, 7, 12, 5) == documented_bytes(36_000, 32_000, 7, 12, 5)
    assert f(1025, 1, 0, 0, 1) == documented_bytes(1025, 1, 0, 0, 1)
    # the header's figures: 28 listeners fit the 512 MiB budget at 1M rays, 29 do not
    assert f(1_000_000, 96_000, RECV_NODES, RECV_TRIS, 28) <= 512 << 20 < f(1_000_000, 96_000, RECV_NODES, RECV_TRIS, 29)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_structs_have_the_c_layout(tmp_path):
    mirrors = {"arx_listener_pose": ArxListenerPose, "arx_listener_result": ArxListenerResult}
    assert C.sizeof(ArxListenerPose) == 16 and C.sizeof(ArxListenerResult) == 48
    assert LISTENER_RESULT_DTYPE.itemsize == 48
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "arx.h"', "int main(void) {"]
    for cname, py in mirrors.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, field, v = ln.split()
        got[(cname, field)] = int(v)
    for cname, py in mirrors.items():
        assert got[(cname, "sizeof")] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
            if py is ArxListenerResult:
                assert LISTENER_RESULT_DTYPE.fields[f][1] == got[(cname, f)], f


def test_null_renderer_is_an_invalid_argument():
    pose = ArxListenerPose(0.0, 0.0, 0.0, 0.0)
    assert lib().arx_render_listeners(None, C.byref(pose), 1, None, None, None, None, None) == INVALID
    assert lib().arx_render_listeners(None, None, 0, None, None, None, None, None) == INVALID
    assert lib().arx_debug_set_listener_chunk(None, 1) == INVALID


def test_listener_grid_is_cell_centres_x_fastest():
    g = listener_grid((-8, 0, -4), (8, 0, 4), 8, 4, 1.2, yaw_deg=30.0)
    assert g.shape == (32, 4) and g.dtype == np.float32
    assert np.array_equal(g[:8, 0], np.arange(-7, 8, 2, dtype=np.float32))
    assert np.array_equal(g[::8, 2], np.array([-3, -1, 1, 3], np.float32))
    assert np.all(g[:8, 2] == -3) and np.all(g[8:16, 2] == -1)
    assert np.all(g[:, 1] == np.float32(1.2)) and np.all(g[:, 3] == 30)
    assert np.array_equal(listener_grid((0, 0), (1, 3), 1, 3, 0.0)[:, [0, 2]],
                          np.array([[0.5, 0.5], [0.5, 1.5], [0.5, 2.5]], np.float32))


def test_acoustic_map_json_round_trip(tmp_path):
    a = ArxAcoustics()
    a.total, a.unit, a.t30_s, a.c50_db, a.d50 = 12345, 0.5, 1.25, float("inf"), 0.75
    a.edt_s = a.t20_s = a.c80_db = a.ts_s = float("nan")
    a.onset_bin, a.last_bin, a.valid = 3, 99, 0x04 | 0x08 | 0x20
    a.t30_bins[0], a.t30_bins[1] = 5, 60
    empty = ArxAcoustics()
    for k in ("edt_s", "t20_s", "t30_s", "c50_db", "c80_db", "d50", "ts_s"):
        setattr(empty, k, float("nan"))
    chans = [{"left": _acoustics_dict(a), "right": _acoustics_dict(empty), "sum": _acoustics_dict(a)},
             {"left": _acoustics_dict(empty), "right": _acoustics_dict(a), "sum": _acoustics_dict(empty)}]
    poses = [(5.0, 1.2, 2.0, 0.0), (4.0, 1.2, 1.0, 15.0)]
    path = tmp_path / "map.json"
    write_acoustic_map_json(str(path), poses, chans)
    got = json.loads(path.read_text())
    assert [e["pose"] for e in got] == [[float(np.float32(v)) for v in p] for p in poses]  # the f32 the call takes
    # the channels are write_acoustics_json's, entry by entry
    for j, e in enumerate(got):
        one = tmp_path / f"one{j}.json"
        write_acoustics_json(str(one), chans[j])
        assert {k: v for k, v in e.items() if k != "pose"} == json.loads(one.read_text())
    left = got[0]["left"]
    assert left["edt_s"] is None and left["c50_db"] == "inf" and left["t30_s"] == 1.25 and left["d50"] == 0.75
    assert left["t30_bins"] == [5, 60] and left["valid"] == ["c50", "d50", "t30"] and left["total"] == 12345
    with pytest.raises(ValueError):
        write_acoustic_map_json(str(path), poses[:1], chans)
