"""CPU: the host side of frequency-band absorption (arx_set_band_absorption / arx_render_bands, include/arx.h)
-- the result struct's layout, the rule for a band table, what the table and the scratch cost, argument
checks that need no device, and the Python scenes whose absorption is the minimum over their bands."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from audiorenderingv2_amd import conference_standin, scene_from_meshes, write_band_acoustics_json
from audiorenderingv2_amd._lib import MAX_BANDS, ArxAcoustics, ArxBandResult, lib
from audiorenderingv2_amd.renderer import BAND_RESULT_DTYPE, _acoustics_dict, write_acoustics_json
from audiorenderingv2_amd.scene import Mesh, Scene, material_bands

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, 1
_F = C.POINTER(C.c_float)


def band_table(n_bands, n_tris):
    """The suite's band table (tests/test_gpu_bands.py uses the same)."""
    return np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.9, (n_bands, n_tris)).astype(np.float32)


def table_check(scene, table):
    scene = np.ascontiguousarray(scene, np.float32)
    table = np.ascontiguousarray(table, np.float32)
    band, tri = C.c_int32(-7), C.c_int64(-7)
    st = lib().arx_band_table_check(scene.ctypes.data_as(_F), table.ctypes.data_as(_F), table.shape[0], scene.shape[0],
                                    C.byref(band), C.byref(tri))
    return st, band.value, tri.value, lib().arx_last_error().decode()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_band_result_has_the_c_layout(tmp_path):
    assert C.sizeof(ArxBandResult) == 40 and BAND_RESULT_DTYPE.itemsize == 40 and MAX_BANDS == 8
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "arx.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(arx_band_result));', '  printf("max_bands %d\\n", ARX_MAX_BANDS);']
    for f, _ in ArxBandResult._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(arx_band_result, {f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(ArxBandResult) and int(got["max_bands"]) == MAX_BANDS
    for f, _ in ArxBandResult._fields_:
        assert int(got[f]) == getattr(ArxBandResult, f).offset == BAND_RESULT_DTYPE.fields[f][1], f


@pytest.mark.parametrize("n_bands,n_tris", [(4, 12), (8, 14), (1, 1), (3, 331_000)])
def test_the_column_minimum_scene_satisfies_the_rule(n_bands, n_tris):
    t = band_table(n_bands, n_tris)
    st, band, tri, _ = table_check(t.min(axis=0), t)
    assert (st, band, tri) == (OK, -1, -1)


def test_a_table_equal_to_the_scene_and_marks_kept_are_accepted():
    scene = np.array([0.25, 0.0, 1.0, -1.0, -2.0], np.float32)
    assert table_check(scene, np.stack([scene, scene]))[0] == OK
    up = np.array([0.5, 0.0, 1.0, -1.0, -2.0], np.float32)
    assert table_check(scene, np.stack([scene, up]))[0] == OK
    assert table_check(scene, np.zeros((0, 5), np.float32))[0] == OK  # no bands: nothing to break


@pytest.mark.parametrize("what,band,tri,value", [
    ("below the scene", 2, 7, None), ("above one", 1, 3, 1.0000001), ("nan", 3, 11, float("nan")),
    ("negative", 0, 5, -0.25), ("a changed -1 mark", 1, 12, 0.3), ("-1 turned -2", 2, 12, -2.0),
    ("a mark where the scene has none", 0, 2, -1.0)])
def test_the_first_offender_is_named(what, band, tri, value):
    t = band_table(4, 14)
    scene = t.min(axis=0)
    scene[12], scene[13] = -1.0, -2.0
    t[:, 12], t[:, 13] = -1.0, -2.0
    assert table_check(scene, t)[0] == OK
    t[band, tri] = np.nextafter(scene[tri], np.float32(-1.0)) if value is None else value
    st, b, i, msg = table_check(scene, t)
    assert (st, b, i) == (INVALID, band, tri), (what, msg)
    assert f"band {band}" in msg and f"triangle {tri}" in msg, msg
    # a second, later offender does not change the answer
    t[3, 13] = 0.5
    assert table_check(scene, t)[1:3] == (band, tri)


def test_bad_check_arguments():
    scene = np.full(4, 0.25, np.float32)
    t = np.full((2, 4), 0.5, np.float32)
    f = lib().arx_band_table_check
    assert f(scene.ctypes.data_as(_F), t.ctypes.data_as(_F), 9, 4, None, None) == INVALID
    assert f(scene.ctypes.data_as(_F), t.ctypes.data_as(_F), -1, 4, None, None) == INVALID
    assert f(None, t.ctypes.data_as(_F), 2, 4, None, None) == INVALID
    assert f(scene.ctypes.data_as(_F), None, 2, 4, None, None) == INVALID
    assert f(scene.ctypes.data_as(_F), t.ctypes.data_as(_F), 2, 4, None, None) == OK  # outputs may be NULL
    bad_scene = np.array([0.25, 1.5, 0.25, 0.25], np.float32)
    st, band, tri, msg = table_check(bad_scene, t)
    assert (st, band, tri) == (INVALID, -1, 1) and "triangle 1" in msg


def test_null_renderer_is_an_invalid_argument():
    t = np.full((2, 4), 0.5, np.float32)
    assert lib().arx_set_band_absorption(None, t.ctypes.data_as(_F), 2, 4) == INVALID
    assert lib().arx_render_bands(None, None, None, None, None, None) == INVALID
    assert lib().arx_band_count(None) == 0


def documented_bytes(ir_len, n_tris, n_bands):
    analysis = lib().arx_debug_band_bytes(0, 0, 1) - 400  # the header's definition of the analysis scratch
    width = 4 if n_bands <= 4 else 8
    return n_tris * width * 4 + n_bands * (16 * ir_len + 64 + 336 + 8 * ir_len) + 24 * ir_len + analysis


def test_band_bytes_is_the_documented_sum():
    f = lib().arx_debug_band_bytes
    assert f(0, 0, 1) > 400 and (f(0, 0, 1) - 400) % 16 == 0
    prev = 0
    for n_bands in range(1, 9):
        got = f(96_000, 331_000, n_bands)
        assert got == documented_bytes(96_000, 331_000, n_bands), n_bands
        assert got > prev
        prev = got
    assert f(32_000, 12, 3) == documented_bytes(32_000, 12, 3)
    assert f(2, 1, 5) == documented_bytes(2, 1, 5)  # every region is a multiple of 16 B for an even ir_len
    assert f(96_000, 331_000, 0) == 0 and f(96_000, 331_000, 9) == 0 and f(-1, 1, 1) == 0 and f(1, -1, 1) == 0
    # C3 with eight bands: the table 10.6 MB, the scratch 20.7 MB
    assert 30e6 < f(96_000, 331_000, 8) < 33e6


def square(name, x):
    v = np.array([[x, 0, 0], [x + 1, 0, 0], [x + 1, 1, 0], [x, 1, 0]], np.float32)
    return Mesh(name, v, np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def test_scene_from_meshes_takes_the_minimum_over_bands():
    meshes = [square("wood", 0), square("glass", 2), square("unknown", 4), square("receiver_left", 6), square("plain", 8)]
    materials = [("wood", [0.10, 0.30, 0.05]), ("glass", (0.9, 0.2, 0.4)), ("plain", 0.75)]
    assert material_bands(materials) == 3 and material_bands([("plain", 0.75)]) == 0 and material_bands(()) == 0
    s = scene_from_meshes(meshes, materials)
    assert s.band_abs.shape == (3, 10) and s.band_abs.dtype == np.float32 and s.tri_abs.dtype == np.float32
    want = np.array([[0.10, 0.9, 0.5, -1.0, 0.75], [0.30, 0.2, 0.5, -1.0, 0.75], [0.05, 0.4, 0.5, -1.0, 0.75]], np.float32)
    assert np.array_equal(s.band_abs, np.repeat(want, 2, axis=1))
    assert np.array_equal(s.tri_abs, np.repeat(np.array([0.05, 0.2, 0.5, -1.0, 0.75], np.float32), 2))
    assert table_check(s.tri_abs, s.band_abs)[0] == OK
    # scalar materials: as before, no table
    plain = scene_from_meshes(meshes, [("wood", 0.1)])
    assert plain.band_abs is None and plain.tri_abs[0] == np.float32(0.1)
    assert Scene(s.tri_v, s.tri_abs, s.names).band_abs is None
    with pytest.raises(ValueError):
        scene_from_meshes(meshes, [("wood", [0.1, 0.2]), ("glass", [0.1, 0.2, 0.3])])


def test_conference_standin_with_band_materials():
    with open(os.path.join(REPO, "tests", "golden", "conference_materials.json")) as fh:
        names = json.load(fh)
    rng = np.random.Generator(np.random.PCG64(11))
    materials = [(n, rng.uniform(0.05, 0.9, 4).astype(np.float32)) for n in names[:-1]]  # the last: the 0.5 default
    s = conference_standin(n_boxes=10, n_cylinders=10, materials=materials)
    plain = conference_standin(n_boxes=10, n_cylinders=10)
    assert np.array_equal(s.tri_v, plain.tri_v) and s.names == plain.names and plain.band_abs is None
    assert s.band_abs.shape == (4, s.n_tris)
    assert np.array_equal(s.tri_abs, s.band_abs.min(axis=0))
    lut = dict(materials)
    for t in (0, 12, 12 + 12 * 10, s.n_tris - 1):
        assert np.array_equal(s.band_abs[:, t], lut.get(s.names[t], np.full(4, 0.5, np.float32))), t
    assert table_check(s.tri_abs, s.band_abs)[0] == OK


def test_band_acoustics_json(tmp_path):
    a = ArxAcoustics()
    a.total, a.unit, a.t30_s, a.c50_db = 99, 0.5, 1.25, float("inf")
    a.edt_s = a.t20_s = a.c80_db = a.ts_s = a.d50 = float("nan")
    a.valid = 0x04 | 0x08
    chans = {"left": _acoustics_dict(a), "right": _acoustics_dict(a), "sum": _acoustics_dict(a)}
    path = tmp_path / "bands.json"
    write_band_acoustics_json(str(path), [125, 250.0], [chans, chans])
    got = json.loads(path.read_text())
    one = tmp_path / "one.json"
    write_acoustics_json(str(one), chans)
    assert [e["band_hz"] for e in got] == [125.0, 250.0]
    for e in got:
        assert {k: v for k, v in e.items() if k != "band_hz"} == json.loads(one.read_text())
    with pytest.raises(ValueError):
        write_band_acoustics_json(str(path), [125], [chans, chans])
