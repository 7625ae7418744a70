"""Python host mirror of the reference's AudioRenderer (R/prebuild/obj_raytracer/AudioRenderer.h:16-152).

Method names follow the reference so callers and tests read like the original:
render(), convoluteAudioFile(), setEmitterPosInOptix(), setSphereCenterInOptix(),
setThresholds(), set_hrtf_absorption_rate(), setBasePower(), setMonoOutput().  Every
call goes through libarx.so's C ABI (include/arx.h); there is no CPU fallback.
"""
from __future__ import annotations

import atexit
import ctypes as C
import dataclasses
import json
import os
import time
import weakref
from dataclasses import dataclass

import numpy as np

from ._lib import ACOUSTICS_VALID, MAX_BANDS, ArxAcoustics, ArxBandResult, ArxConfig, ArxListenerBandResult, ArxListenerPose, ArxListenerResult, ArxStats, check, fptr, lib
from .formats import write_float_lines
from .scene import Scene

# Every live native object, released at interpreter exit (streams, then buffers, groups and
# renderers), while the HIP and RCCL runtimes are still whole: objects the interpreter would finalize
# only during its own teardown -- or never -- otherwise reach the runtimes' exit-time destructors
# still allocated (a double free inside HIP 7.2's teardown was the result).
_LIVE: "dict[str, weakref.WeakSet]" = {k: weakref.WeakSet() for k in ("stream", "buffer", "group", "renderer")}


@atexit.register
def _release_all() -> None:
    for kind in ("stream", "buffer", "group", "renderer"):
        for obj in list(_LIVE[kind]):
            try:
                obj.close()
            except Exception:
                pass


@dataclass
class RenderSettings:
    rays: tuple = (100, 100, 100)          # pathtracer_parameters.rays (Context.cpp:125-133)
    ir_length_in_seconds: int = 2          # renderer_parameters.ir_length_in_seconds
    sample_rate: int = 44100               # audio file rate (Context.cpp:197-224)
    base_power: float = 100.0
    energy_thres: float = 0.0
    max_bounces: int = 10
    hrtf_absorption_rate: float = 1.0      # round(0.9), Context.cpp:145
    mono: bool = False
    seed: int = 1
    device: int = 0

    def to_c(self) -> ArxConfig:
        c = ArxConfig()
        c.rays_x, c.rays_y, c.rays_z = (int(v) for v in self.rays)
        c.ir_length_in_seconds = int(self.ir_length_in_seconds)
        c.sample_rate = int(self.sample_rate)
        c.base_power = float(self.base_power)
        c.energy_thres = float(self.energy_thres)
        c.max_bounces = int(self.max_bounces)
        c.hrtf_absorption_rate = float(self.hrtf_absorption_rate)
        c.is_mono = 1 if self.mono else 0
        c.seed = int(self.seed)
        c.device = int(self.device)
        return c


class AudioRenderer:
    """AudioRenderer(model, ir_length_in_seconds, sample_rate, materials, rays) (AudioRenderer.h:24)."""

    def __init__(self, settings: RenderSettings, scene: Scene | None = None,
                 receiver: tuple[np.ndarray, np.ndarray] | None = None, _borrowed: C.c_void_p | None = None):
        self.settings = settings
        self._owned = _borrowed is None
        self._h = C.c_void_p()
        if _borrowed is not None:  # a RenderGroup member: the group owns the handle
            self._h = _borrowed
        else:
            cfg = settings.to_c()
            check(lib().arx_create(C.byref(cfg), C.byref(self._h)))
            _LIVE["renderer"].add(self)
        self.ir_length = settings.ir_length_in_seconds * settings.sample_rate
        if receiver is not None:
            self.set_receiver_model(*receiver)
        if scene is not None:
            self.set_scene(scene)

    # -- lifecycle ---------------------------------------------------------------
    def close(self) -> None:
        if self._h and self._owned:
            lib().arx_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # -- scene -------------------------------------------------------------------
    def set_scene(self, scene: Scene) -> None:
        self._scene_v = np.ascontiguousarray(scene.tri_v, np.float32)
        self._scene_a = np.ascontiguousarray(scene.tri_abs, np.float32)
        check(lib().arx_set_scene(self._h, fptr(self._scene_v), fptr(self._scene_a), scene.n_tris))
        if getattr(scene, "band_abs", None) is not None:
            self.set_band_absorption(scene.band_abs)

    def set_band_absorption(self, table) -> None:
        """arx_set_band_absorption: table (B, T) f32, band b's absorption of scene triangle t -- at least the
        scene's own on every triangle, in [0, 1], a receiver mark kept; None or B == 0 drops it."""
        if table is None:
            check(lib().arx_set_band_absorption(self._h, None, 0, 0))
            return
        t = np.ascontiguousarray(table, np.float32)
        if t.ndim != 2:
            raise ValueError("band table: (bands, triangles)")
        check(lib().arx_set_band_absorption(self._h, fptr(t), t.shape[0], t.shape[1]))

    @property
    def n_bands(self) -> int:
        """arx_band_count: the bands of the installed table, 0 without one -- what render_bands returns."""
        return int(lib().arx_band_count(self._h))

    def set_source_directivity(self, cube) -> None:
        """arx_set_source_directivity: cube (B, 6, res, res) f32 gains in [0, 1] (or (6, res, res): one band,
        which serves every band of the table); None drops the pattern.  render_bands and
        render_listener_bands then start ray r's band b from e0 * cube[b][texel of r's direction]; render and
        render_listeners stay omnidirectional.  The engine does not renormalise: scale base_power by
        1 / directivity_power(cube) for the omnidirectional source's radiated power."""
        if cube is None:
            check(lib().arx_set_source_directivity(self._h, None, 0, 0))
            return
        c = _cube_array(cube)
        check(lib().arx_set_source_directivity(self._h, fptr(c), c.shape[0], c.shape[2]))

    def set_source_orientation(self, yaw_deg=0.0, pitch_deg: float = 0.0, roll_deg: float = 0.0) -> None:
        """arx_set_source_orientation: the source's local axes in world coordinates -- a 3 x 3 matrix whose
        rows are the local x, y, z axes, or yaw / pitch / roll in degrees (source_rotation).  Turning costs
        the gain kernel and a replay, never a trace."""
        m = np.asarray(yaw_deg, np.float64)
        m = source_rotation(float(yaw_deg), pitch_deg, roll_deg) if m.ndim == 0 else m
        m = np.ascontiguousarray(m, np.float32).reshape(-1)
        if m.size != 9:
            raise ValueError("source orientation: a 3 x 3 matrix, or yaw, pitch, roll in degrees")
        check(lib().arx_set_source_orientation(self._h, fptr(m)))

    @property
    def n_directivity_bands(self) -> int:
        """arx_source_directivity_bands: the bands of the installed pattern, 0 without one."""
        return int(lib().arx_source_directivity_bands(self._h))

    def directivity_plane(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """arx_debug_directivity_plane: rows [first, first + count) of the device gain plane, (count, W) f32,
        indexed like the path cache's direction copy; made from the current recording if it is stale."""
        bands = self.n_bands or self.n_directivity_bands
        n = int(self.settings.rays[0]) * int(self.settings.rays[1]) * int(self.settings.rays[2])
        count = n - first if count is None else count
        out = np.zeros((count, 4 if bands <= 4 else 8), np.float32)
        check(lib().arx_debug_directivity_plane(self._h, first, count, fptr(out)))
        return out

    def set_air_absorption(self, alpha_db_per_m) -> None:
        """arx_set_air_absorption: the air's loss in dB per metre per band, finite and >= 0 -- one value
        (serves every band of the table) or one per band; None drops it.  render_bands and
        render_listener_bands then weight a receiver deposit of band b in bin k by
        exp(-alpha[b] ln(10) / 10 * k * 343 / sample_rate) (air_attenuation is the table); the energy a
        ray carries, and so every counter, is unchanged.  air_absorption_iso9613 gives pure-tone values."""
        if alpha_db_per_m is None:
            check(lib().arx_set_air_absorption(self._h, None, 0))
            return
        a = np.ascontiguousarray(np.atleast_1d(alpha_db_per_m), np.float64)
        if a.ndim != 1 or a.size < 1:
            raise ValueError("air absorption: one coefficient, or one per band")
        check(lib().arx_set_air_absorption(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size))

    @property
    def n_air_bands(self) -> int:
        """arx_air_absorption_bands: the coefficients installed, 0 without any."""
        return int(lib().arx_air_absorption_bands(self._h))

    def air_table(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """arx_debug_air_table: rows [first, first + count) of the device attenuation table, (count, W) f32,
        a row per IR bin; made now if it is stale.  It needs coefficients, and no recording."""
        bands = self.n_bands or self.n_air_bands
        count = self.ir_length - first if count is None else count
        out = np.zeros((max(count, 0), 4 if bands <= 4 else 8), np.float32)
        check(lib().arx_debug_air_table(self._h, first, count, fptr(out)))
        return out

    def band_histograms(self) -> np.ndarray:
        """arx_debug_band_histograms: the last render_bands call's raw int64 histograms, (B, 2, ir_len):
        band b's left and right, before finalize."""
        out = np.zeros((self.n_bands, 2, self.ir_length), np.int64)
        check(lib().arx_debug_band_histograms(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), out.size))
        return out

    def set_receiver_model(self, left: np.ndarray, right: np.ndarray) -> None:
        for side, t in enumerate((left, right)):
            t = np.ascontiguousarray(t, np.float32).reshape(-1, 9)
            check(lib().arx_set_receiver_model(self._h, side, fptr(t), t.shape[0]))

    def setEmitterPosInOptix(self, pos) -> None:  # AudioRenderer.cpp:752-756
        check(lib().arx_set_emitter(self._h, *(float(v) for v in pos)))

    def setSphereCenterInOptix(self, pos, yaw_deg: float = 0.0) -> None:
        """placeReceiver(...) + setSphereCenterInOptix (AudioRenderer.cpp:758-762)."""
        check(lib().arx_set_listener(self._h, *(float(v) for v in pos), float(yaw_deg)))

    place_listener = setSphereCenterInOptix

    def setThresholds(self, energy: float, max_bounces: int) -> None:
        check(lib().arx_set_thresholds(self._h, float(energy), int(max_bounces)))

    def set_hrtf_absorption_rate(self, rate: float) -> None:
        check(lib().arx_set_hrtf_absorption_rate(self._h, float(rate)))

    def setBasePower(self, p: float) -> None:
        check(lib().arx_set_base_power(self._h, float(p)))

    def setMonoOutput(self, mono: bool) -> None:
        check(lib().arx_set_mono_output(self._h, 1 if mono else 0))

    def normalizeAndMergeStereoOutput(self, left, right, mono_len: int, out) -> None:
        """Declared by the reference with an empty body (AudioRenderer.cpp:574-576): a no-op,
        kept so callers of that API keep working (the live path zips L/R on the device)."""

    def set_frames_in_flight(self, n: int) -> None:
        """1 to 3 (arx_set_frames_in_flight): with n > 1, consecutive render() calls rotate over n
        streams and buffer sets, so a render / convolute loop keeps the GPU full; every getter and
        convolution refers to the last frame started."""
        check(lib().arx_set_frames_in_flight(self._h, int(n)))

    def set_timing(self, on: bool) -> None:
        """arx_set_timing: per-launch timing events (trace_times / conv_times) on or off; a render()
        still times its trace."""
        check(lib().arx_set_timing(self._h, 1 if on else 0))

    def set_seed(self, seed: int) -> None:
        check(lib().arx_set_seed(self._h, int(seed)))

    def set_stream(self, stream_ptr: int | None) -> None:
        """Issue work on this hipStream_t (e.g. torch.cuda.Stream().cuda_stream); 0/None = null stream."""
        check(lib().arx_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def get_stream(self) -> int:
        return int(lib().arx_get_stream(self._h) or 0)

    # -- render ------------------------------------------------------------------
    def render(self) -> float:
        """AudioRenderer::render (AudioRenderer.cpp:489-523); returns the trace kernel's ms.
        With the write-IR flag set, dumps the IR once like :525-567 and clears the flag."""
        ms = C.c_double()
        check(lib().arx_render(self._h, C.byref(ms)))
        if self.write_ir_to_file_flag:
            L, R = self.get_ir()
            lp, rp = "output_ir_left.txt", "output_ir_right.txt"
            if self.experimentation:
                stamp = time.time_ns()
                lp = os.path.join("experimentation", f"output_ir_left_{stamp}.txt")
                rp = os.path.join("experimentation", f"output_ir_right_{stamp}.txt")
            write_float_lines(os.path.join(self.output_dir, lp), L)
            write_float_lines(os.path.join(self.output_dir, rp), R)
            self.write_ir_to_file_flag = False
        if self.write_acoustics_to_file_flag:  # next to the IR dump; no reference counterpart
            self.analyze_ir()
            name = "output_acoustics.json"
            if self.experimentation:
                name = os.path.join("experimentation", f"output_acoustics_{time.time_ns()}.json")
            write_acoustics_json(os.path.join(self.output_dir, name), {ch: self.acoustics(ch) for ch in ACOUSTICS_CHANNELS})
            self.write_acoustics_to_file_flag = False
        return ms.value

    # -- text dumps (AudioRenderer.cpp:525-567, 720-744; setters :780-788) -----------
    write_ir_to_file_flag = False
    write_output_to_file_flag = False
    write_acoustics_to_file_flag = False
    experimentation = False
    output_dir = "."

    def set_write_ir_to_file_flag(self, value: bool) -> None:
        self.write_ir_to_file_flag = bool(value)

    def set_write_output_to_file_flag(self, value: bool) -> None:
        self.write_output_to_file_flag = bool(value)

    def set_write_acoustics_to_file_flag(self, value: bool) -> None:
        """The next render() analyses its histogram and writes the three channels' room-acoustic
        parameters to output_acoustics.json, next to the IR dump; then the flag clears."""
        self.write_acoustics_to_file_flag = bool(value)

    def enable_experimentation(self) -> None:
        self.experimentation = True

    def set_trace_path(self, path: int) -> None:
        """Parity hook (arx_debug_set_trace_path): bit 0 forces the f32 nodes, bit 1 the
        global-memory traversal stack; 0 = automatic."""
        check(lib().arx_debug_set_trace_path(self.handle, int(path)))

    def set_ray_order(self, mode: int) -> None:
        """arx_debug_set_ray_order: 0 directions kept in ray order, 1 (default) the ray pool's slots
        longest ray first, 2 directions re-made by every launch."""
        check(lib().arx_debug_set_ray_order(self.handle, int(mode)))

    PATH_CACHE_STATES = ("off", "traced", "recorded", "replayed", "not-cacheable", "over-cap")

    def set_path_cache(self, mode: int, max_bytes: int = 1 << 30) -> None:
        """arx_debug_set_path_cache: 0 off, 1 (default) a repeated key replays its cached scene-only
        hits against the receiver; max_bytes caps the records."""
        check(lib().arx_debug_set_path_cache(self.handle, int(mode), int(max_bytes)))

    def path_cache_state(self, queries: bool = False) -> dict:
        """arx_debug_path_cache_state: what the last trace launch did (PATH_CACHE_STATES), the bytes of
        records held and, when asked for (synchronises), the queries the recording ran."""
        st, nb, nq = C.c_int32(), C.c_uint64(), C.c_uint64()
        check(lib().arx_debug_path_cache_state(self.handle, C.byref(st), C.byref(nb), C.byref(nq) if queries else None))
        return {"state": self.PATH_CACHE_STATES[st.value], "bytes": int(nb.value), "queries_recorded": int(nq.value)}

    def set_path_filter(self, on: bool) -> None:
        """arx_debug_set_path_filter: on (default) a replayed frame runs only the queries whose segment
        crosses the receiver's box; off, every cached query as before."""
        check(lib().arx_debug_set_path_filter(self.handle, 1 if on else 0))

    def path_filter_state(self, candidates: bool = False) -> dict:
        """arx_debug_path_filter_state: whether the last trace launch was a filtered replay, the bytes held
        for the filter and, when asked for (synchronises), its candidate rays and queries."""
        fl, nb, cr, cq = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().arx_debug_path_filter_state(self.handle, C.byref(fl), C.byref(nb),
                                                C.byref(cr) if candidates else None, C.byref(cq) if candidates else None))
        return {"filtered": bool(fl.value), "bytes": int(nb.value), "candidate_rays": int(cr.value),
                "candidate_queries": int(cq.value)}

    def set_listener_chunk(self, n: int) -> None:
        """arx_debug_set_listener_chunk: listeners per chunk of render_listeners (0: automatic, else 1..64)."""
        check(lib().arx_debug_set_listener_chunk(self.handle, int(n)))

    def render_listeners(self, poses, irs: bool | tuple = False, acoustics: bool = True) -> dict:
        """arx_render_listeners: a batch of listeners (x, y, z, yaw_deg) rendered from one recorded path
        set, bit for bit the loop of setSphereCenterInOptix + render (+ analyze_ir) over them; the
        listener set before stays.  irs: False, True (host arrays) or a pair of DeviceBuffers / device
        pointers of K * ir_len floats each (returned as given).  Returns {"ir": (L[K, ir_len],
        R[K, ir_len]) | None, "acoustics": [{"left", "right", "sum"}] * K | None, "stats": a structured
        array of arx_listener_result's fields, "ms": the call's device time}."""
        P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 4))
        k = P.shape[0]
        ir, pl, pr = _ir_pair(irs, (k, self.ir_length))
        ac = (ArxAcoustics * (3 * max(k, 1)))() if acoustics else None
        res = (ArxListenerResult * max(k, 1))()
        ms = C.c_double(0.0)
        check(lib().arx_render_listeners(self.handle, P.ctypes.data_as(C.POINTER(ArxListenerPose)), k, pl, pr, ac, res,
                                         C.byref(ms)))
        stats = np.frombuffer(res, dtype=LISTENER_RESULT_DTYPE, count=k).copy() if k else np.zeros(0, LISTENER_RESULT_DTYPE)
        return {"ir": ir, "acoustics": _acoustics_list(ac, k) if acoustics else None, "stats": stats, "ms": float(ms.value)}

    def render_bands(self, irs: bool | tuple = False, acoustics: bool = True) -> dict:
        """arx_render_bands: every band of set_band_absorption's table from one walk over the recorded
        paths, band b bit for bit the frame of a renderer whose scene carries table[b].  irs: False, True
        (host arrays) or a pair of DeviceBuffers / device pointers of B * ir_len floats each (returned as
        given).  Returns {"ir": (L[B, ir_len], R[B, ir_len]) | None, "acoustics": [{"left", "right",
        "sum"}] * B | None, "stats": a structured array of arx_band_result's fields, "ms": the call's
        device time}."""
        k = self.n_bands  # the library's own count: the output buffers are sized from it
        ir, pl, pr = _ir_pair(irs, (k, self.ir_length))
        ac = (ArxAcoustics * (3 * MAX_BANDS))() if acoustics else None
        res = (ArxBandResult * MAX_BANDS)()
        ms = C.c_double(0.0)
        check(lib().arx_render_bands(self.handle, pl, pr, ac, res, C.byref(ms)))
        stats = np.frombuffer(res, dtype=BAND_RESULT_DTYPE, count=k).copy()
        return {"ir": ir, "acoustics": _acoustics_list(ac, k) if acoustics else None, "stats": stats, "ms": float(ms.value)}

    def combine_bands(self, irs, filters, n_bands: int | None = None, ir_len: int | None = None, out=None,
                      taps: int | None = None) -> dict:
        """arx_combine_bands: one broadband IR pair from band IRs -- out = sum over the bands of filter b
        convolved with IR b, zero-phase, in include/arx.h's f64 arithmetic, rounded once to f32.  irs: a
        pair of [B, ir_len] float32 arrays, or a pair of DeviceBuffers / device pointers of B * ir_len floats
        each with n_bands=B and ir_len (render_bands' irs).  filters: a [B, taps] array (converted to f64;
        band_filters' result), or a DeviceBuffer / device pointer of B * taps doubles with taps.  out: None
        (host arrays are returned) or a pair of DeviceBuffers / device pointers of ir_len floats each
        (returned as given).  Needs no scene and leaves the renderer's own IR alone.  Returns {"ir": (L, R),
        "ms": the call's device time}."""
        keep = []  # host arrays the call reads
        if n_bands is None:
            L, R = (np.ascontiguousarray(a, np.float32) for a in irs)
            if L.shape != R.shape or L.ndim != 2:
                raise ValueError("irs: a pair of [B, ir_len] arrays")
            keep += [L, R]
            k, n, pl, pr = L.shape[0], L.shape[1], L.ctypes.data, R.ctypes.data
        else:
            if ir_len is None:
                raise ValueError("device IRs need n_bands and ir_len")
            k, n = int(n_bands), int(ir_len)
            pl, pr = (int(getattr(b, "ptr", b)) for b in irs)
        if taps is None:
            g = np.ascontiguousarray(filters, np.float64)
            if g.ndim != 2 or g.shape[0] != k:
                raise ValueError(f"filters: a [{k}, taps] array")
            keep.append(g)
            t, pg = g.shape[1], g.ctypes.data
        else:
            t, pg = int(taps), int(getattr(filters, "ptr", filters))
        host_out = None
        if out is None:
            host_out = (np.empty(n, np.float32), np.empty(n, np.float32))
            ol, or_ = host_out[0].ctypes.data, host_out[1].ctypes.data
        else:
            out = tuple(out)
            ol, or_ = (int(getattr(b, "ptr", b)) for b in out)
        ms = C.c_double(0.0)
        check(lib().arx_combine_bands(self.handle, pl or None, pr or None, k, n, pg or None, t, ol or None, or_ or None,
                                      C.byref(ms)))
        del keep
        return {"ir": host_out if out is None else out, "ms": float(ms.value)}

    def render_broadband(self, filters, set_ir: bool = False) -> dict:
        """Frequency-dependent absorption made audible on the device: render_bands into device buffers, then
        combine_bands on them with `filters` ([n_bands, taps], band_filters' result) -- the band IRs never
        visit the host.  set_ir: the broadband IR becomes the renderer's IR (set_ir_device), so the next
        convolution or stream block uses it.  Returns {"ir": (L, R) host arrays, "acoustics" and "stats":
        render_bands', "render_ms": render_bands' device time, "ms": the combine's}."""
        k, n = self.n_bands, self.ir_length
        dev = self.settings.device
        bufs = [DeviceBuffer(dev, max(k * n * 4, 4)) for _ in range(2)] + [DeviceBuffer(dev, max(n * 4, 4)) for _ in range(2)]
        try:
            rb = self.render_bands(irs=tuple(bufs[:2]), acoustics=True)
            cb = self.combine_bands(tuple(bufs[:2]), filters, n_bands=k, ir_len=n, out=tuple(bufs[2:]))
            ir = tuple(b.to_numpy(np.float32, n) for b in bufs[2:])
            if set_ir:
                self.set_ir_device(bufs[2].ptr, bufs[3].ptr)
                check(lib().arx_copy_ir(self._h, None, None, n))  # the copy has left the buffers before they go
        finally:
            for b in bufs:
                b.close()
        return {"ir": ir, "acoustics": rb["acoustics"], "stats": rb["stats"], "render_ms": rb["ms"], "ms": cb["ms"]}

    def render_listener_bands(self, poses, irs: bool | tuple = False, acoustics: bool = True, filters=None,
                              broadband: tuple | None = None) -> dict:
        """arx_render_listener_bands: every band of set_band_absorption's table for a batch of listeners
        (x, y, z, yaw_deg) from one recorded path set -- entry (j, b) bit for bit the loop of
        setSphereCenterInOptix + render_bands (+ combine_bands) over the poses; the listener set before
        stays.  irs: False, True (host arrays) or a pair of DeviceBuffers / device pointers of K * B * ir_len
        floats each (returned as given).  filters: None, or a [B, taps] array (band_filters' result): then
        every listener's bands are also combined into one broadband pair, into host arrays or, with
        broadband=(left, right), into DeviceBuffers / device pointers of K * ir_len floats each
        (convolute_walk's layout; returned as given).  Returns {"ir": (L[K, B, ir_len], R[K, B, ir_len]) |
        None, "broadband": (L[K, ir_len], R[K, ir_len]) | None, "acoustics": [[{"left", "right", "sum"}] * B]
        * K | None, "stats": a [K, B] structured array of arx_listener_band_result's fields, "ms": the
        call's device time}."""
        P = np.ascontiguousarray(poses, np.float32)
        if P.ndim != 2 or P.shape[1] != 4:
            raise ValueError("poses: a [K, 4] array of (x, y, z, yaw_deg)")
        nb = self.n_bands  # the library's own count: the output buffers are sized from it
        if broadband is not None and filters is None:
            raise ValueError("broadband buffers need filters")
        g = None
        if filters is not None:
            if nb < 1:
                raise ValueError("filters need a band table (set_band_absorption)")
            g = np.ascontiguousarray(filters, np.float64)
            if g.ndim != 2 or g.shape[0] != nb:
                raise ValueError(f"filters: a [{nb}, taps] array")
        k, n = P.shape[0], self.ir_length
        ir, pl, pr = _ir_pair(irs, (k, nb, n))
        bb, bl, br = _ir_pair(g is not None and (True if broadband is None else broadband), (k, n))
        cells = max(k * nb, 1)
        ac = (ArxAcoustics * (3 * cells))() if acoustics else None
        res = (ArxListenerBandResult * cells)()
        ms = C.c_double(0.0)
        check(lib().arx_render_listener_bands(self.handle, P.ctypes.data_as(C.POINTER(ArxListenerPose)), k, pl or None,
                                              pr or None, g.ctypes.data if g is not None else None,
                                              g.shape[1] if g is not None else 0, bl or None, br or None, ac, res,
                                              C.byref(ms)))
        stats = np.frombuffer(res, dtype=LISTENER_BAND_RESULT_DTYPE, count=k * nb).copy().reshape(k, nb)
        out_ac = None
        if acoustics:
            flat = _acoustics_list(ac, k * nb)
            out_ac = [flat[j * nb:(j + 1) * nb] for j in range(k)]
        return {"ir": ir, "broadband": bb, "acoustics": out_ac, "stats": stats, "ms": float(ms.value)}

    def auralise_walk_bands(self, poses, samples, filters, block_frames: int = 4096, crossfade_frames: int | None = None,
                            fade: str | int = "hann") -> dict:
        """auralise_walk with frequency-dependent absorption: render_listener_bands over the poses with the
        broadband set in device buffers, the poses spread evenly over the input's blocks, then convolute_walk
        on those buffers -- neither the band IRs nor the broadband IRs visit the host.  Returns
        auralise_walk's dict."""
        P = np.ascontiguousarray(poses, np.float32)
        if P.ndim != 2 or P.shape[1] != 4:
            raise ValueError("poses: a [K, 4] array of (x, y, z, yaw_deg)")
        return self._auralise(lambda bufs: self.render_listener_bands(P, irs=False, acoustics=False, filters=filters,
                                                                      broadband=bufs),
                              P.shape[0], samples, block_frames, crossfade_frames, fade)

    def set_walk_tile(self, items: int) -> None:
        """arx_debug_set_walk_tile: items per multiply-accumulate workgroup of convolute_walk (0: the
        product's tile, else 1..64); the same bits either way."""
        check(lib().arx_debug_set_walk_tile(self.handle, int(items)))

    def walk_state(self) -> dict:
        """arx_debug_walk_state: the last convolute_walk's blocks, transition blocks, distinct IRs
        transformed, tiles launched and scratch bytes."""
        out = (C.c_uint64 * 5)()
        check(lib().arx_debug_walk_state(self.handle, out))
        return dict(zip(("blocks", "transitions", "irs_transformed", "tiles", "scratch_bytes"), (int(v) for v in out)))

    def convolute_walk(self, irs, ir_of_block, samples, block_frames: int = 4096, crossfade_frames: int = 0,
                       fade: str | int = "hann", n_irs: int | None = None, n_frames: int | None = None, out=None) -> dict:
        """arx_convolute_walk: `samples` convolved with the IR ir_of_block[b] on output block b, crossfaded
        over the first crossfade_frames frames of every block whose IR differs from the block before -- bit
        for bit the loop of set_ir_device + LiveStream.process_device over the blocks, in one call that
        leaves the renderer's IR and streams alone.  irs: a pair of [K, ir_len] float32 arrays, or a pair of
        DeviceBuffers / device pointers of K * ir_len floats each with n_irs=K (render_listeners' irs).
        samples: an array (converted to f64), or a DeviceBuffer / device pointer of f64 frames with
        n_frames.  out: None (a host array is returned) or a DeviceBuffer / device pointer of
        2 * len(ir_of_block) * block_frames doubles (returned as given).  Returns {"out": the frames as
        [len(ir_of_block) * block_frames, 2] L/R, "ms": the call's device time}."""
        sched = np.ascontiguousarray(ir_of_block, np.int32).reshape(-1)
        nb, B = sched.size, int(block_frames)
        keep = []  # host arrays the call reads
        if n_irs is None:
            L, R = (np.ascontiguousarray(a, np.float32) for a in irs)
            if L.shape != R.shape or L.ndim != 2 or L.shape[1] != self.ir_length:
                raise ValueError("irs: a pair of [K, ir_len] arrays")
            keep += [L, R]
            k, pl, pr = L.shape[0], L.ctypes.data, R.ctypes.data
        else:
            k = int(n_irs)
            pl, pr = (int(getattr(b, "ptr", b)) for b in irs)
        if n_frames is None:
            x = np.ascontiguousarray(samples, np.float64).reshape(-1)
            keep.append(x)
            nf, px = x.size, x.ctypes.data
        else:
            nf, px = int(n_frames), int(getattr(samples, "ptr", samples))
        host_out = None
        if out is None:
            host_out = np.empty((nb * max(B, 0), 2), np.float64)
            po_ = host_out.ctypes.data
        else:
            po_ = int(getattr(out, "ptr", out))
        ms = C.c_double(0.0)
        check(lib().arx_convolute_walk(self.handle, pl or None, pr or None, k, sched.ctypes.data_as(C.POINTER(C.c_int32)), nb,
                                       px or None, nf, B, int(crossfade_frames), _fade_shape(fade), po_ or None,
                                       C.byref(ms)))
        del keep
        return {"out": host_out if out is None else out, "ms": float(ms.value)}

    def auralise_walk(self, poses, samples, block_frames: int = 4096, crossfade_frames: int | None = None,
                      fade: str | int = "hann") -> dict:
        """A walk made audible on the device: render_listeners over the poses into device buffers, the
        poses spread evenly over the input's blocks (walk_schedule over walk_blocks, the last pose ringing
        out the tail), then convolute_walk on those buffers -- the IRs never visit the host.
        crossfade_frames=None: a whole block.  Returns {"out": [n_blocks * block_frames, 2] L/R frames,
        "ir_of_block", "render_ms", "ms": the convolution's device time}."""
        P = np.asarray(poses, np.float32).reshape(-1, 4)
        return self._auralise(lambda bufs: self.render_listeners(P, irs=bufs, acoustics=False), P.shape[0], samples,
                              block_frames, crossfade_frames, fade)

    def _auralise(self, render, k: int, samples, block_frames: int, crossfade_frames: int | None, fade: str | int) -> dict:
        """Both auralise_walk methods: render(a pair of device buffers of k * ir_len floats each) fills them with
        the k poses' IRs, then convolute_walk runs on them with the poses spread evenly over the input's blocks."""
        x = np.ascontiguousarray(samples, np.float64).reshape(-1)
        B = int(block_frames)
        F = B if crossfade_frames is None else int(crossfade_frames)
        sched = walk_schedule(x.size, B, self.ir_length, k)
        dev = self.settings.device
        bufs = [DeviceBuffer(dev, max(k * self.ir_length * 4, 4)) for _ in range(2)]
        try:
            rl = render(tuple(bufs))
            res = self.convolute_walk(tuple(bufs), sched, x, B, F, fade, n_irs=k)
        finally:
            for b in bufs:
                b.close()
        return {"out": res["out"], "ir_of_block": sched, "render_ms": rl["ms"], "ms": res["ms"]}

    def ray_order_buffer(self, count: int) -> dict:
        """arx_debug_ray_order_buffer: the first count slots (count x 4 floats) of the current frame
        set's direction buffer, the ray id of slot 0, the leading slots still in ray order and whether
        the pool's slots are sorted."""
        out = np.empty((int(count), 4), np.float32)
        first, n_static, srt = C.c_uint64(), C.c_uint64(), C.c_int32()
        check(lib().arx_debug_ray_order_buffer(self.handle, fptr(out), int(count), C.byref(first), C.byref(n_static),
                                               C.byref(srt)))
        return {"dirs": out, "first_ray": int(first.value), "n_static": int(n_static.value), "sorted": bool(srt.value)}

    def node_images(self) -> dict:
        """Parity hook (arx_debug_node_images): the device's coded f32 nodes (n x 16 words), their
        device-made 16-bit quantized copy (n x 8 words), the grid and the re-quantization count."""
        n = int(self.stats()["n_nodes"])
        cn = np.empty((n, 16), np.uint32)
        qn = np.empty((n, 8), np.uint32)
        grid = np.empty(6, np.float32)
        rq = C.c_uint64()
        check(lib().arx_debug_node_images(self._h, cn.ctypes.data_as(C.c_void_p), qn.ctypes.data_as(C.c_void_p), n,
                                          fptr(grid), C.byref(rq)))
        return {"cnodes": cn, "qnodes": qn, "origin": grid[:3], "scale": grid[3:], "requants": int(rq.value)}

    def clear_histogram(self) -> None:
        check(lib().arx_clear_histogram(self._h))

    def trace_rays(self, ray_begin: int, ray_end: int) -> None:
        check(lib().arx_trace_rays(self._h, int(ray_begin), int(ray_end)))

    def finalize_ir(self) -> None:
        check(lib().arx_finalize_ir(self._h))

    def histogram_device_ptr(self) -> tuple[int, int]:
        p = C.c_void_p()
        n = C.c_size_t()
        check(lib().arx_histogram_device(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def attach_histogram(self, d_ptr: int | None, n_elems: int = 0) -> None:
        check(lib().arx_attach_histogram(self._h, C.c_void_p(d_ptr or 0), int(n_elems)))

    def ir_device_ptrs(self) -> tuple[int, int, int]:
        l, r, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        check(lib().arx_ir_device(self._h, C.byref(l), C.byref(r), C.byref(n)))
        return int(l.value), int(r.value), int(n.value)

    def get_ir(self) -> tuple[np.ndarray, np.ndarray]:
        L = np.empty(self.ir_length, np.float32)
        R = np.empty(self.ir_length, np.float32)
        check(lib().arx_copy_ir(self._h, fptr(L), fptr(R), self.ir_length))
        return L, R

    def set_ir(self, left: np.ndarray, right: np.ndarray) -> None:
        L = np.ascontiguousarray(left, np.float32)
        R = np.ascontiguousarray(right, np.float32)
        check(lib().arx_set_ir(self._h, fptr(L), fptr(R), L.size))

    def trace_times(self, n: int = 64) -> np.ndarray:
        """Device ms of the last min(n, ring) trace launches, oldest first (arx_trace_times)."""
        out = np.zeros(n, np.float64)
        k = C.c_size_t()
        check(lib().arx_trace_times(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(k)))
        return out[:k.value]

    def conv_times(self, n: int = 64) -> np.ndarray:
        """Device ms of the last min(n, ring) file convolutions, oldest first (arx_conv_times)."""
        out = np.zeros(n, np.float64)
        k = C.c_size_t()
        check(lib().arx_conv_times(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(k)))
        return out[:k.value]

    def live_times(self, n: int = 64) -> np.ndarray:
        """Device ms of the last min(n, ring) live / streaming convolution blocks (arx_live_times)."""
        out = np.zeros(n, np.float64)
        k = C.c_size_t()
        check(lib().arx_live_times(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(k)))
        return out[:k.value]

    def stats(self) -> dict:
        s = ArxStats()
        check(lib().arx_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in ArxStats._fields_}

    # -- room-acoustic parameters (no reference counterpart) ------------------------
    def analyze_ir(self) -> None:
        """arx_analyze_ir: queue the decay curves and ISO 3382-1 parameters of the last started
        frame's histogram on its stream (asynchronous)."""
        check(lib().arx_analyze_ir(self._h))

    def set_auto_analyze(self, on: bool) -> None:
        """arx_set_auto_analyze: every render() queues the analysis behind its IR finalize."""
        check(lib().arx_set_auto_analyze(self._h, 1 if on else 0))

    def acoustics(self, channel: str | int = "sum") -> dict:
        """arx_get_acoustics of "left", "right" or "sum" (synchronises): total, unit, edt_s, t20_s,
        t30_s, c50_db, c80_db, d50, ts_s (NaN where invalid), onset_bin, last_bin, the fit ranges
        edt_bins / t20_bins / t30_bins, valid (the set of valid quantities' names) and valid_mask."""
        a = ArxAcoustics()
        check(lib().arx_get_acoustics(self._h, _channel(channel), C.byref(a)))
        return _acoustics_dict(a)

    def edc(self, channel: str | int = "sum") -> np.ndarray:
        """arx_copy_edc: Schroeder's decay curve E[k] = sum of the histogram from bin k on, exact
        int64 in fixed-point units (times acoustics()["unit"] = energy)."""
        out = np.empty(self.ir_length, np.int64)
        check(lib().arx_copy_edc(self._h, _channel(channel), out.ctypes.data_as(C.POINTER(C.c_int64)), out.size))
        return out

    def analysis_times(self, n: int = 64) -> np.ndarray:
        """Device ms of the last min(n, ring) analyses, oldest first (arx_analysis_times)."""
        out = np.zeros(n, np.float64)
        k = C.c_size_t()
        check(lib().arx_analysis_times(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), n, C.byref(k)))
        return out[:k.value]

    def set_scan_shape(self, shape: int) -> None:
        """Measurement hook (arx_debug_set_scan_shape): 1 = one workgroup per channel, 2 = tiled
        two-launch scan, 0 = the product's choice; the same bits either way."""
        check(lib().arx_debug_set_scan_shape(self._h, int(shape)))

    # -- convolution ---------------------------------------------------------------
    def convoluteAudioFile(self, samples: np.ndarray) -> tuple[np.ndarray, np.ndarray, float, float]:
        """AudioRenderer::convoluteAudioFile (AudioRenderer.cpp:663-750): host in, host out."""
        x = np.ascontiguousarray(samples, np.float32)
        L = np.zeros_like(x)
        R = np.zeros_like(x)
        cms, pms = C.c_double(), C.c_double()
        check(lib().arx_convolute_audio_file(self._h, fptr(x), x.nbytes, fptr(L), fptr(R), C.byref(cms),
                                             C.byref(pms)))
        if self.write_output_to_file_flag:
            write_float_lines(os.path.join(self.output_dir, "output_convolute_left.txt"), L)
            write_float_lines(os.path.join(self.output_dir, "output_convolute_right.txt"), R)
            self.write_output_to_file_flag = False
        return L, R, cms.value, pms.value

    def convoluteLiveInput(self, block: np.ndarray, circular_buffer=None) -> np.ndarray:
        """AudioRenderer::convoluteLiveInput (AudioRenderer.cpp:593-661): one f64 mic block ->
        2*ir_len interleaved doubles, added into circular_buffer (CircularBuffer::add) if given."""
        x = np.ascontiguousarray(block, np.float64)
        out = np.empty(2 * self.ir_length, np.float64)
        D = C.POINTER(C.c_double)
        check(lib().arx_convolute_live_block(self._h, x.ctypes.data_as(D), x.nbytes, out.ctypes.data_as(D), out.size))
        if circular_buffer is not None:
            circular_buffer.add(out)
        return out

    def prepare_ir_spectra(self, file: bool = True, live: bool = False) -> None:
        """Recompute the cached IR spectra now (async) rather than in the next convolution."""
        check(lib().arx_prepare_ir_spectra(self._h, (1 if file else 0) | (2 if live else 0)))

    def set_ir_device(self, d_left: int, d_right: int) -> None:
        """Take the IR from device memory (arx_set_ir_device), async on this renderer's stream."""
        check(lib().arx_set_ir_device(self._h, C.c_void_p(d_left), C.c_void_p(d_right), self.ir_length))

    def conv_plan(self, live: bool = False) -> str:
        """The convolution plan in use (arx_conv_describe): direct mixed-radix or power-of-two."""
        buf = C.create_string_buffer(256)
        check(lib().arx_conv_describe(self._h, 2 if live else 1, buf, len(buf)))
        return buf.value.decode()

    def convolute_live_device(self, d_in: int, n_in: int, d_out: int) -> None:
        check(lib().arx_convolute_live_device(self._h, C.c_void_p(d_in), n_in, C.c_void_p(d_out)))

    def convolute_device(self, d_in: int, n_frames: int, d_out_left: int, d_out_right: int) -> None:
        check(lib().arx_convolute_device(self._h, C.c_void_p(d_in), n_frames, C.c_void_p(d_out_left),
                                         C.c_void_p(d_out_right)))

    def convolute_prepare_input(self, d_in: int, n_frames: int) -> None:
        """arx_convolute_prepare_input: the file's blocks transformed once, for convolute_prepared
        (the reference re-convolves the same file with every new IR, AudioRenderer.cpp:790-798)."""
        check(lib().arx_convolute_prepare_input(self._h, C.c_void_p(d_in), n_frames))

    def convolute_prepared(self, d_out_left: int, d_out_right: int) -> int:
        """arx_convolute_prepared: the prepared file convolved with the current IR (bit-identical to
        convolute_device on the same input); returns the frame count."""
        n = C.c_size_t()
        check(lib().arx_convolute_prepared(self._h, C.c_void_p(d_out_left), C.c_void_p(d_out_right), C.byref(n)))
        return int(n.value)


ACOUSTICS_CHANNELS = ("left", "right", "sum")


def _channel(channel: str | int) -> int:
    """A channel's number; an unknown name goes to the library as -1 (rejected)."""
    if isinstance(channel, str):
        return ACOUSTICS_CHANNELS.index(channel) if channel in ACOUSTICS_CHANNELS else -1
    return int(channel)


def _acoustics_dict(a: ArxAcoustics) -> dict:
    d = {}
    for k, _ in ArxAcoustics._fields_[:-1]:  # not the reserved word
        v = getattr(a, k)
        d[k] = tuple(v) if k.endswith("_bins") else v
    d["valid_mask"] = int(a.valid)
    d["valid"] = {name for bit, name in enumerate(ACOUSTICS_VALID) if a.valid >> bit & 1}
    return d


def _acoustics_list(ac, cells: int) -> list:
    """cells x 3 arx_acoustics as [{"left", "right", "sum"}] * cells."""
    return [{name: _acoustics_dict(ac[3 * j + c]) for c, name in enumerate(ACOUSTICS_CHANNELS)} for j in range(cells)]


def _ir_pair(irs, shape) -> tuple:
    """A method's irs argument -- False, True (host arrays of `shape`) or a pair of DeviceBuffers / device
    pointers -- as (what the method returns, the left pointer, the right pointer)."""
    if irs is True:
        ir = (np.zeros(shape, np.float32), np.zeros(shape, np.float32))
        return ir, ir[0].ctypes.data, ir[1].ctypes.data
    if irs:
        ir = tuple(irs)
        pl, pr = (int(getattr(b, "ptr", b)) for b in ir)
        return ir, pl, pr
    return None, None, None


def acoustics_from_histogram(left, right, sample_rate: int, unit: float = 1.0) -> dict:
    """arx_acoustics_from_histogram (host only, no device): the parameters of an int64 histogram
    pair by the definitions of include/arx.h, as {"left": ..., "right": ..., "sum": ...}."""
    L = np.ascontiguousarray(left, np.int64)
    R = np.ascontiguousarray(right, np.int64)
    if L.shape != R.shape or L.ndim != 1:
        raise ValueError("left and right must be one-dimensional and of one length")
    out = (ArxAcoustics * 3)()
    P = C.POINTER(C.c_int64)
    check(lib().arx_acoustics_from_histogram(L.ctypes.data_as(P), R.ctypes.data_as(P), L.size, int(sample_rate),
                                             float(unit), out))
    return _acoustics_list(out, 1)[0]


def write_acoustics_json(path: str, channels: dict) -> None:
    """{"left" | "right" | "sum": acoustics()} as JSON: invalid quantities (NaN) as null, an infinite
    clarity as the string "inf", valid as a sorted list."""
    _dump_json(path, _channels_plain(channels))


def _json_plain(v):
    """write_acoustics_json's number formatting."""
    if isinstance(v, (set, frozenset)):
        return sorted(v)
    if isinstance(v, float) and not np.isfinite(v):
        return None if np.isnan(v) else ("inf" if v > 0 else "-inf")
    return list(v) if isinstance(v, tuple) else v


def _channels_plain(channels: dict) -> dict:
    return {ch: {k: _json_plain(v) for k, v in a.items()} for ch, a in channels.items()}


def _dump_json(path: str, obj) -> None:
    with open(path, "w") as fh:
        json.dump(obj, fh, indent=1)
        fh.write("\n")


LISTENER_RESULT_DTYPE = np.dtype([("queries", "<u8"), ("receiver_hits", "<u8"), ("misses", "<u8"), ("candidate_rays", "<u8"),
                                  ("route", "<i4"), ("reserved", "<i4"), ("reserved2", "<u8")])


BAND_RESULT_DTYPE = np.dtype([("queries", "<u8"), ("receiver_hits", "<u8"), ("misses", "<u8"), ("warm_launches", "<i4"),
                              ("reserved", "<i4"), ("reserved2", "<u8")])  # arx_band_result


LISTENER_BAND_RESULT_DTYPE = np.dtype([("queries", "<u8"), ("receiver_hits", "<u8"), ("misses", "<u8"),
                                       ("candidate_rays", "<u8"), ("route", "<i4"), ("warm_launches", "<i4"),
                                       ("reserved2", "<u8")])  # arx_listener_band_result


def write_band_acoustic_map_json(path: str, poses, bands_hz, acoustics: list) -> None:
    """render_listener_bands' acoustics as JSON: [{"pose": [x, y, z, yaw_deg], "bands": [{"band_hz", "left",
    "right", "sum"}]}] in pose order, each pose's bands as write_band_acoustics_json writes them."""
    P = np.asarray(poses, np.float32).reshape(-1, 4)
    if P.shape[0] != len(acoustics):
        raise ValueError("one acoustics entry per pose")
    out = []
    for p, per_band in zip(P, acoustics):
        if len(bands_hz) != len(per_band):
            raise ValueError(f"{len(bands_hz)} bands, {len(per_band)} results")
        out.append({"pose": [float(v) for v in p],
                    "bands": [{"band_hz": float(hz), **_channels_plain(a)} for hz, a in zip(bands_hz, per_band)]})
    _dump_json(path, out)


def write_band_acoustics_json(path: str, bands_hz, acoustics: list) -> None:
    """render_bands' acoustics as JSON: a list of {"band_hz", "left", "right", "sum"}, the channels as
    write_acoustics_json writes them."""
    if len(bands_hz) != len(acoustics):
        raise ValueError(f"{len(bands_hz)} bands, {len(acoustics)} results")
    _dump_json(path, [{"band_hz": float(hz), **_channels_plain(a)} for hz, a in zip(bands_hz, acoustics)])


def octave_crossovers(centres_hz) -> np.ndarray:
    """The crossover frequencies between neighbouring band centres: their geometric means (one fewer than
    the centres), as band_filters takes them."""
    f = np.asarray(centres_hz, np.float64).reshape(-1)
    return np.sqrt(f[:-1] * f[1:])


def band_filters(sample_rate: int, crossovers_hz, taps: int) -> np.ndarray:
    """arx_band_filters (host only): the float64 [B, taps] linear-phase filter bank of B = len(crossovers_hz)
    + 1 bands -- raised-cosine band edges one octave wide in log-frequency, Hann-windowed, symmetric on bits,
    summing to a unit impulse at (taps - 1) / 2 -- that combine_bands and render_broadband take."""
    x = np.ascontiguousarray(crossovers_hz, np.float64).reshape(-1)
    g = np.zeros((x.size + 1, max(int(taps), 0)), np.float64)
    D = C.POINTER(C.c_double)
    check(lib().arx_band_filters(int(sample_rate), x.ctypes.data_as(D) if x.size else None, x.size + 1, int(taps),
                                 g.ctypes.data_as(D)))
    return g


def listener_grid(lo, hi, nx: int, nz: int, y: float, yaw_deg: float = 0.0) -> np.ndarray:
    """(nx * nz, 4) float32 poses (x, y, z, yaw_deg) for render_listeners: the centres of an nx x nz grid of
    cells over [lo, hi] in x and z (lo / hi: (x, z) pairs or (x, y, z) triples whose y is ignored) at height
    y, x fastest."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    x0, z0, x1, z1 = lo[0], lo[-1], hi[0], hi[-1]
    xs = x0 + (np.arange(nx) + 0.5) * (x1 - x0) / nx
    zs = z0 + (np.arange(nz) + 0.5) * (z1 - z0) / nz
    out = np.empty((nx * nz, 4), np.float32)
    out[:, 0] = np.tile(xs, nz)
    out[:, 1] = y
    out[:, 2] = np.repeat(zs, nx)
    out[:, 3] = yaw_deg
    return out


def write_acoustic_map_json(path: str, poses, acoustics: list) -> None:
    """A listener map as JSON: [{"pose": [x, y, z, yaw_deg], "left" | "right" | "sum": ...}] in pose order,
    the channels written as write_acoustics_json writes them (NaN as null, an infinite clarity as "inf")."""
    P = np.asarray(poses, np.float32).reshape(-1, 4)
    if P.shape[0] != len(acoustics):
        raise ValueError("one acoustics entry per pose")
    _dump_json(path, [{"pose": [float(v) for v in p], **_channels_plain(ac)} for p, ac in zip(P, acoustics)])


def edc_from_histogram(hist) -> np.ndarray:
    """arx_edc_from_histogram (host only): the reverse inclusive cumulative sum of int64 bins."""
    h = np.ascontiguousarray(hist, np.int64)
    out = np.empty(h.size, np.int64)
    P = C.POINTER(C.c_int64)
    check(lib().arx_edc_from_histogram(h.ctypes.data_as(P), h.size, out.ctypes.data_as(P)))
    return out


FADE_SHAPES = ("linear", "hann")  # ARX_FADE_LINEAR, ARX_FADE_HANN


def _fade_shape(fade: str | int) -> int:
    """A shape's number; one that is neither a known name nor an int goes to the library as -1 (rejected)."""
    if isinstance(fade, str):
        return FADE_SHAPES.index(fade) if fade in FADE_SHAPES else -1
    return int(fade)


def fade_weights(shape: str | int, n: int) -> np.ndarray:
    """arx_stream_fade_weights (host only): the new IR's weight on each of a transition block's first
    n frames -- the table a LiveStream with that crossfade uses."""
    w = np.empty(max(int(n), 0), np.float64)
    check(lib().arx_stream_fade_weights(_fade_shape(shape), int(n), w.ctypes.data_as(C.POINTER(C.c_double))))
    return w


def walk_blocks(n_frames: int, block_frames: int, ir_len: int) -> int:
    """arx_walk_blocks (host only): ceil(n_frames / block) + ceil((ir_len - 1) / block), the blocks of a
    convolute_walk until the tail has rung out; 0 for invalid arguments."""
    return int(lib().arx_walk_blocks(int(n_frames), int(block_frames), int(ir_len)))


def walk_schedule(n_frames: int, block_frames: int, ir_len: int, n_irs: int) -> np.ndarray:
    """arx_walk_even_schedule over walk_blocks (host only): the int32 ir_of_block of a walk that spreads
    n_irs IRs evenly over the input's ceil(n_frames / block) blocks and rings out the tail with the last."""
    nb = walk_blocks(n_frames, block_frames, ir_len)
    n_in = -(-int(n_frames) // int(block_frames)) if block_frames > 0 else 0
    out = np.zeros(nb, np.int32)
    check(lib().arx_walk_even_schedule(n_in, nb, int(n_irs), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


class LiveStream:
    """Streaming convolution of a renderer's IR (arx_stream_*, uniformly partitioned overlap-save
    in f64): process(block) consumes one block of <= block_frames f64 frames and returns
    block_frames output frames zipped L/R -- the linear convolution of the input stream with the
    current IR at the reference live path's scale (ir_len / (ir_len/2)).  The drop-in successor of
    convoluteLiveInput + CircularBuffer (AudioRenderer.cpp:593-661, main.cpp:99-135), whose
    full-length circular result the reference's buffer wraps onto itself.

    crossfade_frames > 0 (at most block_frames): the first block after an IR change is computed
    with the old and the new IR and blended over its first crossfade_frames frames with
    fade_weights(fade, crossfade_frames), instead of stepping to the new IR at the block boundary
    (arx_stream_set_crossfade)."""

    def __init__(self, renderer: AudioRenderer, block_frames: int = 4096, crossfade_frames: int = 0,
                 fade: str | int = "hann"):
        self.renderer = renderer
        self._s = C.c_void_p()
        check(lib().arx_stream_create(renderer.handle, int(block_frames), C.byref(self._s)))
        _LIVE["stream"].add(self)
        b, p, n = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().arx_stream_info(self._s, C.byref(b), C.byref(p), C.byref(n)))
        self.block_frames, self.partitions, self.fft_size = b.value, p.value, n.value
        if crossfade_frames:
            self.set_crossfade(crossfade_frames, fade)

    def set_crossfade(self, frames: int, fade: str | int = "hann") -> None:
        """Crossfade over the first `frames` frames of a block whose IR is new; 0 = hard switch."""
        check(lib().arx_stream_set_crossfade(self._s, int(frames), _fade_shape(fade)))

    @property
    def crossfade(self) -> tuple[int, str]:
        """(frames, shape name) as set by set_crossfade; (0, "hann") on a fresh stream."""
        f, sh = C.c_int32(), C.c_int32()
        check(lib().arx_stream_get_crossfade(self._s, C.byref(f), C.byref(sh)))
        return f.value, FADE_SHAPES[sh.value]

    @property
    def crossfades(self) -> int:
        """Transition blocks processed since the stream was created."""
        n = C.c_uint64()
        check(lib().arx_stream_crossfades(self._s, C.byref(n)))
        return int(n.value)

    def process(self, block: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(block, np.float64)
        out = np.empty(2 * self.block_frames, np.float64)
        D = C.POINTER(C.c_double)
        check(lib().arx_stream_process(self._s, x.ctypes.data_as(D), x.size, out.ctypes.data_as(D), out.size))
        return out

    def process_device(self, d_in: int, n_frames: int, d_out: int) -> None:
        check(lib().arx_stream_process_device(self._s, C.c_void_p(d_in), int(n_frames), C.c_void_p(d_out)))

    def reset(self) -> None:
        check(lib().arx_stream_reset(self._s))

    def close(self) -> None:
        if self._s:
            lib().arx_stream_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RenderGroup:
    """Ray-sharded multi-GPU rendering through libarx.so's native RCCL groups (arx_group_*).

    RenderGroup(settings, devices=[0, 1, ...]) drives several GPUs from this process
    (ncclCommInitAll); RenderGroup.rank(settings, n_ranks, rank, uid) joins a one-GPU-per-process
    group (ncclCommInitRank) with the id rank 0 got from RenderGroup.unique_id().  render() =
    every shard traced + one int64 all-reduce + the IR finalised on every member; member(i) is
    that member's AudioRenderer (convolution, IR access).  The reference has no equivalent (it
    renders on device 0, AudioRenderer.cpp:252)."""

    def __init__(self, settings: RenderSettings, devices=None, scene: Scene | None = None,
                 receiver: tuple[np.ndarray, np.ndarray] | None = None, _rank=None):
        self.settings = settings
        self._g = C.c_void_p()
        cfg = settings.to_c()
        if _rank is not None:
            n_ranks, rank, uid = _rank
            check(lib().arx_group_create_rank(C.byref(cfg), int(n_ranks), int(rank), uid, len(uid) if uid else 0,
                                              C.byref(self._g)))
        else:
            devs = list(devices if devices is not None else [settings.device])
            arr = (C.c_int32 * len(devs))(*devs)
            check(lib().arx_group_create(C.byref(cfg), arr, len(devs), C.byref(self._g)))
        _LIVE["group"].add(self)
        self.ir_length = settings.ir_length_in_seconds * settings.sample_rate
        self.members = []
        for i in range(lib().arx_group_members(self._g)):
            h = C.c_void_p(lib().arx_group_member(self._g, i))
            cfg = ArxConfig()
            check(lib().arx_get_config(h, C.byref(cfg)))
            self.members.append(AudioRenderer(dataclasses.replace(settings, device=int(cfg.device)), _borrowed=h))
        if receiver is not None:
            self.set_receiver_model(*receiver)
        if scene is not None:
            self.set_scene(scene)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(lib().arx_group_unique_id(buf, 128))
        return buf.raw

    @classmethod
    def rank(cls, settings: RenderSettings, n_ranks: int, rank: int, uid: bytes | None, **kw) -> "RenderGroup":
        return cls(settings, _rank=(n_ranks, rank, uid), **kw)

    def close(self) -> None:
        for m in getattr(self, "members", []):
            m._h = C.c_void_p()
        if self._g:
            lib().arx_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._g

    def member(self, i: int = 0) -> AudioRenderer:
        return self.members[i]

    @property
    def n_ranks(self) -> int:
        return int(lib().arx_group_ranks(self._g))

    def set_scene(self, scene: Scene) -> None:
        self._scene_v = np.ascontiguousarray(scene.tri_v, np.float32)
        self._scene_a = np.ascontiguousarray(scene.tri_abs, np.float32)
        check(lib().arx_group_set_scene(self._g, fptr(self._scene_v), fptr(self._scene_a), scene.n_tris))

    def set_receiver_model(self, left: np.ndarray, right: np.ndarray) -> None:
        for side, t in enumerate((left, right)):
            t = np.ascontiguousarray(t, np.float32).reshape(-1, 9)
            check(lib().arx_group_set_receiver_model(self._g, side, fptr(t), t.shape[0]))

    def setEmitterPosInOptix(self, pos) -> None:
        check(lib().arx_group_set_emitter(self._g, *(float(v) for v in pos)))

    def setSphereCenterInOptix(self, pos, yaw_deg: float = 0.0) -> None:
        check(lib().arx_group_set_listener(self._g, *(float(v) for v in pos), float(yaw_deg)))

    def setThresholds(self, energy: float, max_bounces: int) -> None:
        check(lib().arx_group_set_thresholds(self._g, float(energy), int(max_bounces)))

    def set_hrtf_absorption_rate(self, rate: float) -> None:
        check(lib().arx_group_set_hrtf_absorption_rate(self._g, float(rate)))

    def setBasePower(self, p: float) -> None:
        check(lib().arx_group_set_base_power(self._g, float(p)))

    def setMonoOutput(self, mono: bool) -> None:
        check(lib().arx_group_set_mono_output(self._g, 1 if mono else 0))

    def set_frames_in_flight(self, n: int) -> None:
        """arx_group_set_frames_in_flight: AudioRenderer.set_frames_in_flight on every member."""
        check(lib().arx_group_set_frames_in_flight(self._g, int(n)))

    def set_timing(self, on: bool) -> None:
        """arx_group_set_timing: AudioRenderer.set_timing on every member."""
        check(lib().arx_group_set_timing(self._g, 1 if on else 0))

    def set_seed(self, seed: int) -> None:
        check(lib().arx_group_set_seed(self._g, int(seed)))

    def render(self, timed: bool = True) -> float:
        """Trace all shards + all-reduce + finalize; returns the longest shard's trace ms (timed)
        or 0.0 without synchronising (timed=False)."""
        ms = C.c_double()
        check(lib().arx_group_render(self._g, C.byref(ms) if timed else None))
        return ms.value

    def synchronize(self) -> None:
        check(lib().arx_group_synchronize(self._g))

    def get_ir(self) -> tuple[np.ndarray, np.ndarray]:
        L = np.empty(self.ir_length, np.float32)
        R = np.empty(self.ir_length, np.float32)
        check(lib().arx_group_copy_ir(self._g, fptr(L), fptr(R), self.ir_length))
        return L, R

    def stats(self) -> dict:
        s = ArxStats()
        check(lib().arx_group_get_stats(self._g, C.byref(s)))
        return {k: getattr(s, k) for k, _ in ArxStats._fields_}

    def allreduce(self, values, op: str = "sum") -> np.ndarray:
        """This process's values combined over every process of the group (one RCCL all-reduce,
        synchronising: also a barrier); a group living in one process returns them unchanged."""
        v = np.ascontiguousarray(np.atleast_1d(values), np.float64).copy()
        check(lib().arx_group_allreduce_f64(self._g, v.ctypes.data_as(C.POINTER(C.c_double)), v.size,
                                            {"sum": 0, "max": 1}[op]))
        return v

    def allreduce_times(self, n: int = 64, member: int = 0) -> np.ndarray:
        """Device ms of member `member`'s last min(n, 256) timed histogram all-reduces, oldest first
        (arx_group_allreduce_times; recorded while the members' timing is on)."""
        out = np.zeros(n, np.float64)
        k = C.c_size_t()
        check(lib().arx_group_allreduce_times(self._g, int(member), out.ctypes.data_as(C.POINTER(C.c_double)), n,
                                              C.byref(k)))
        return out[:k.value]

    def convolute_device(self, d_in, n_frames: int, d_out_left, d_out_right) -> None:
        """Time-block sharded file convolution (arx_group_convolute_device): per local member i, the
        whole file at d_in[i] and full-length outputs d_out_left[i] / d_out_right[i] on its device; rank
        g writes the output frames conv_shard(g) owns."""
        k = len(self.members)
        P = C.c_void_p * k
        check(lib().arx_group_convolute_device(self._g, P(*d_in), int(n_frames), P(*d_out_left), P(*d_out_right)))

    def convoluteAudioFile(self, samples: np.ndarray) -> tuple[np.ndarray, np.ndarray, float, float]:
        """AudioRenderer::convoluteAudioFile over the group (arx_group_convolute_audio_file): host in,
        host out, every GPU of this process convolving its time-block shard; bit-identical to one
        renderer's convoluteAudioFile.  Returns (L, R, convolute_ms, process_ms)."""
        x = np.ascontiguousarray(samples, np.float32)
        L = np.zeros_like(x)
        R = np.zeros_like(x)
        cms, pms = C.c_double(), C.c_double()
        check(lib().arx_group_convolute_audio_file(self._g, fptr(x), x.nbytes, fptr(L), fptr(R), C.byref(cms),
                                                   C.byref(pms)))
        return L, R, cms.value, pms.value

    def conv_shard(self, n_frames: int, rank: int, n_ranks: int | None = None) -> tuple[int, int]:
        """Output frames [begin, end) rank `rank` owns in a sharded convolution (arx_group_conv_shard)."""
        b, e = C.c_uint64(), C.c_uint64()
        lib().arx_group_conv_shard(int(self.settings.sample_rate), int(n_frames), int(rank),
                                   int(self.n_ranks if n_ranks is None else n_ranks), C.byref(b), C.byref(e))
        return int(b.value), int(e.value)

    @property
    def conv_sharded(self) -> bool:
        """Whether the convolution plan shards by time blocks (else every rank convolves the whole file)."""
        v = int(lib().arx_group_conv_sharded(self._g))
        if v < 0:
            check(6)
        return v == 1

    def debug_force_collectives(self, on: bool = True, out_of_place: bool = False) -> None:
        """Tests only (arx_debug_group_force_collectives): every collective issued at one rank too,
        out of place into 0xFF-filled receive buffers if asked."""
        check(lib().arx_debug_group_force_collectives(self._g, 1 if on else 0, 1 if out_of_place else 0))

    def debug_collectives(self) -> dict:
        """Collectives the group has issued (arx_debug_group_collectives)."""
        out = (C.c_uint64 * 3)()
        check(lib().arx_debug_group_collectives(self._g, out))
        return {"histogram_allreduce": int(out[0]), "f64_allreduce": int(out[1]), "scene_broadcast": int(out[2])}


class DeviceBuffer:
    """Device memory allocated through libarx (arx_device_alloc), so that a caller such as
    bench.py needs no other GPU framework (and libarx runs on the HIP runtime it was built with)."""

    def __init__(self, device: int, nbytes: int):
        self.device = int(device)
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().arx_device_alloc(self.device, self.nbytes, C.byref(p)))
        self.ptr = int(p.value)
        _LIVE["buffer"].add(self)

    @classmethod
    def from_numpy(cls, device: int, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(device, a.nbytes)
        check(lib().arx_memcpy(b.device, C.c_void_p(b.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return b

    def to_numpy(self, dtype, count: int | None = None) -> np.ndarray:
        dt = np.dtype(dtype)
        n = self.nbytes // dt.itemsize if count is None else int(count)
        out = np.empty(n, dt)
        check(lib().arx_memcpy(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), out.nbytes))
        return out

    def close(self) -> None:
        if self.ptr:
            lib().arx_device_free(self.device, C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    """HIP devices visible to this process (arx_device_count)."""
    return int(lib().arx_device_count())


def runtime_info() -> str:
    """Paths and versions of the HIP and RCCL runtimes libarx resolved (arx_runtime_info)."""
    buf = C.create_string_buffer(2048)
    check(lib().arx_runtime_info(buf, len(buf)))
    return buf.value.decode()


def scene_build_count() -> int:
    return int(lib().arx_scene_build_count())


def place_receiver_vertices(local_xyz: np.ndarray, pos, yaw_deg: float) -> np.ndarray:
    """place_receiver_half's transform (OptixModel.cpp:178-193), host-only."""
    v = np.ascontiguousarray(local_xyz, np.float32).reshape(-1, 3)
    out = np.empty_like(v)
    check(lib().arx_place_receiver_vertices(fptr(v), v.shape[0], *(float(p) for p in pos), float(yaw_deg),
                                            fptr(out)))
    return out


def debug_ray_directions(seed: int, first: int, count: int, device: int = 0) -> np.ndarray:
    out = np.empty((count, 3), np.float32)
    check(lib().arx_debug_ray_directions(seed, first, count, fptr(out), device))
    return out


def frac_bits(n_rays: int) -> int:
    return int(lib().arx_frac_bits(n_rays))


# -- source directivity (include/arx.h, "Directional sources") ---------------------------------------------
def _cube_array(cube) -> np.ndarray:
    """A pattern as (B, 6, res, res) contiguous f32; (6, res, res) is one band."""
    c = np.ascontiguousarray(cube, np.float32)
    if c.ndim == 3:
        c = c[None]
    if c.ndim != 4 or c.shape[1] != 6 or c.shape[2] != c.shape[3]:
        raise ValueError("directivity cube: (bands, 6, res, res)")
    return np.ascontiguousarray(c)


def source_rotation(yaw_deg: float = 0.0, pitch_deg: float = 0.0, roll_deg: float = 0.0) -> np.ndarray:
    """The orientation matrix of set_source_orientation, f64 (3, 3): row i is the source's local axis i in
    world coordinates.  y is up: yaw turns the source about world +y (counter-clockwise seen from above, so
    local +x goes from world +x towards world -z), pitch then lifts local +x towards +y about the turned z
    axis, roll turns about local +x.  All zero is the identity."""
    y, p, r = np.radians([yaw_deg, pitch_deg, roll_deg])
    ry = np.array([[np.cos(y), 0.0, np.sin(y)], [0.0, 1.0, 0.0], [-np.sin(y), 0.0, np.cos(y)]])
    rz = np.array([[np.cos(p), -np.sin(p), 0.0], [np.sin(p), np.cos(p), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(r), -np.sin(r)], [0.0, np.sin(r), np.cos(r)]])
    return (ry @ rz @ rx).T  # the columns of the rotation are the local axes: as rows


def cube_texel_directions(res: int) -> np.ndarray:
    """Unit vectors (6, res, res, 3) f64 through the texel centres, in the source's local frame, by the
    lookup's convention: faces +x, -x, +y, -y, +z, -z; u and v run along the two remaining coordinates in
    x, y, z order, with no per-face flips."""
    c = (np.arange(res) + 0.5) * (2.0 / res) - 1.0
    v, u = np.meshgrid(c, c, indexing="ij")
    one = np.ones_like(u)
    faces = [(one, u, v), (-one, u, v), (u, one, v), (u, -one, v), (u, v, one), (u, v, -one)]
    d = np.stack([np.stack(f, axis=-1) for f in faces])
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def directivity_cube(fn, res: int, n_bands: int) -> np.ndarray:
    """A pattern (n_bands, 6, res, res) f32 sampled at the texel centres: fn(d, band) -> gains for unit
    vectors d (..., 3) in the source's local frame (+x is the source's front)."""
    d = cube_texel_directions(res)
    return np.stack([np.asarray(fn(d, b), np.float64) * np.ones(d.shape[:-1]) for b in range(n_bands)]).astype(np.float32)


def cardioid_cube(res: int, orders) -> np.ndarray:
    """Per band ((1 + cos theta) / 2) ** order about local +x: order 0 is omnidirectional, 1 a cardioid,
    higher orders narrower -- a pattern that narrows with frequency takes ascending orders."""
    orders = [float(o) for o in np.atleast_1d(orders)]
    return directivity_cube(lambda d, b: (0.5 * (1.0 + d[..., 0])) ** orders[b], res, len(orders))


def directivity_power(cube) -> np.ndarray:
    """Per band the pattern's mean gain over the sphere, each texel weighted with its exact solid angle:
    the directed source's radiated power relative to the omnidirectional source's.  The engine does not
    renormalise; base_power / directivity_power(cube)[b] gives band b the omnidirectional power back."""
    c = _cube_array(cube).astype(np.float64)
    res = c.shape[2]
    e = np.arange(res + 1) * (2.0 / res) - 1.0
    y, x = np.meshgrid(e, e, indexing="ij")
    a = np.arctan2(x * y, np.sqrt(x * x + y * y + 1.0))  # the solid angle of [0, x] x [0, y] on the plane z = 1
    w = a[1:, 1:] - a[:-1, 1:] - a[1:, :-1] + a[:-1, :-1]
    return (c * w).sum(axis=(1, 2, 3)) / (6.0 * w.sum())


def directivity_gains(cube, dirs, orientation=None, width: int | None = None) -> np.ndarray:
    """arx_directivity_gains_host, the lookup's definition: (n, width) f32 gains of the directions (n, 3)."""
    c = _cube_array(cube)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    w = (4 if c.shape[0] <= 4 else 8) if width is None else int(width)
    m = None if orientation is None else np.ascontiguousarray(orientation, np.float32).reshape(-1)
    out = np.zeros((d.shape[0], max(w, 1)), np.float32)
    check(lib().arx_directivity_gains_host(fptr(c), c.shape[0], c.shape[2], None if m is None else fptr(m), fptr(d),
                                           d.shape[0], w, fptr(out)))
    return out


# -- air absorption (include/arx.h, "Air absorption") -------------------------------------------------------
def air_absorption_iso9613(freqs_hz, temperature_c: float = 20.0, relative_humidity: float = 50.0,
                           pressure_kpa: float = 101.325) -> np.ndarray:
    """arx_air_absorption_iso9613: ISO 9613-1's pure-tone attenuation in dB per metre at each frequency (Hz),
    for a temperature in [-20, 50] C, a relative humidity in [0, 100] % and a pressure in (0, 200] kPa.  A
    band takes its centre frequency's value; band-integrated coefficients are the caller's business."""
    f = np.ascontiguousarray(np.atleast_1d(freqs_hz), np.float64).reshape(-1)
    out = np.zeros(f.size, np.float64)
    dp = C.POINTER(C.c_double)
    check(lib().arx_air_absorption_iso9613(float(temperature_c), float(relative_humidity), float(pressure_kpa),
                                           f.ctypes.data_as(dp), f.size, out.ctypes.data_as(dp)))
    return out


def air_attenuation(alpha_db_per_m, sample_rate: int, ir_len: int, width: int | None = None) -> np.ndarray:
    """arx_air_attenuation_host, the table's definition: (ir_len, width) f32 factors, a row per IR bin; one
    coefficient fills every column, else the columns past the coefficients are 0."""
    a = np.ascontiguousarray(np.atleast_1d(alpha_db_per_m), np.float64).reshape(-1)
    w = (4 if a.size <= 4 else 8) if width is None else int(width)
    out = np.zeros((max(int(ir_len), 0), max(w, 1)), np.float32)
    check(lib().arx_air_attenuation_host(a.ctypes.data_as(C.POINTER(C.c_double)), a.size, int(sample_rate), int(ir_len), w,
                                         fptr(out)))
    return out
