"""MI355X-native acoustic impulse-response engine (drop-in for AudioRenderingV2's GPU path).

libarx.so (HIP kernels + C ABI, include/arx.h) does the work; this package is the thin
Python host mirror of the reference's AudioRenderer plus scene/IO helpers.
"""
from ._lib import ArxError, LIB_PATH  # noqa: F401
from .renderer import AudioRenderer, DeviceBuffer, LiveStream, RenderGroup, RenderSettings, acoustics_from_histogram, air_absorption_iso9613, air_attenuation, band_filters, cardioid_cube, cube_texel_directions, debug_ray_directions, directivity_cube, directivity_gains, directivity_power, source_rotation, device_count, edc_from_histogram, fade_weights, frac_bits, listener_grid, octave_crossovers, place_receiver_vertices, runtime_info, scene_build_count, walk_blocks, walk_schedule, write_acoustic_map_json, write_band_acoustic_map_json, write_band_acoustics_json  # noqa: F401
from .scene import Mesh, Scene, conference_standin, receiver_local, scene_from_meshes, test_obj_scene  # noqa: F401

__all__ = [
    "ArxError", "AudioRenderer", "DeviceBuffer", "LiveStream", "device_count", "runtime_info", "scene_build_count", "RenderGroup", "RenderSettings", "Scene", "Mesh", "conference_standin", "receiver_local",
    "scene_from_meshes", "test_obj_scene", "place_receiver_vertices", "debug_ray_directions", "frac_bits", "fade_weights",
    "acoustics_from_histogram", "edc_from_histogram", "listener_grid", "write_acoustic_map_json", "write_band_acoustic_map_json", "write_band_acoustics_json", "walk_blocks", "walk_schedule",
    "band_filters", "octave_crossovers",
    "cardioid_cube", "cube_texel_directions", "directivity_cube", "directivity_gains", "directivity_power", "source_rotation",
    "air_absorption_iso9613", "air_attenuation",
]
