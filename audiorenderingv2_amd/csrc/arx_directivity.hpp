// arx_directivity.hpp -- source directivity (arx_set_source_directivity, include/arx.h): the cube-map lookup,
// written once for the host (arx_directivity_gains_host, the definition) and the device (source_gain_kernel,
// arx_directivity.hip), and the gain plane's launcher.
//
// A pattern only changes the energy a ray starts with, e[b] = e0 * g[ray][b]: the plane g[slot][W] is made
// once per (pattern, orientation, band count, recording) from the path cache's direction copy and read by the
// directed instantiations of the band replays (arx_replay.hip), one or two 16-B loads per ray.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "arx_layout.hpp"

namespace arx {

constexpr int32_t kDirectivityMaxRes = 256;
constexpr int32_t kDirectivityFaces = 6;

// The texel of direction d for the orientation m (rows: the source's local axes in world coordinates), as an
// index into one band's [face][v][u] block; -1: the direction has no major axis (the zero vector, a NaN), gain 0.
// IEEE f32 add, mul, div and comparisons only, in this order, uncontracted (build.py: -ffp-contract=off).
// For finite d the two clamps are min(res - 1, (int)t): t lies in [0, res].
ARX_HOST_DEVICE inline int32_t directivity_texel(const float* m, float dx, float dy, float dz, int32_t res) {
    const float lx = (m[0] * dx + m[1] * dy) + m[2] * dz;
    const float ly = (m[3] * dx + m[4] * dy) + m[5] * dz;
    const float lz = (m[6] * dx + m[7] * dy) + m[8] * dz;
    const float ax = lx < 0.0f ? -lx : lx, ay = ly < 0.0f ? -ly : ly, az = lz < 0.0f ? -lz : lz;
    int32_t face;
    float sc, tc, ma;
    if (ax >= ay && ax >= az) {
        face = lx >= 0.0f ? 0 : 1;
        sc = ly; tc = lz; ma = ax;
    } else if (ay >= az) {
        face = ly >= 0.0f ? 2 : 3;
        sc = lx; tc = lz; ma = ay;
    } else {
        face = lz >= 0.0f ? 4 : 5;
        sc = lx; tc = ly; ma = az;
    }
    if (!(ma > 0.0f)) return -1;
    const float u = sc / ma, v = tc / ma;
    const float half = 0.5f * (float)res;
    const float tu = (u + 1.0f) * half, tv = (v + 1.0f) * half;
    const int32_t iu = tu >= 0.0f ? (tu < (float)res ? (int32_t)tu : res - 1) : 0;  // a NaN: 0
    const int32_t iv = tv >= 0.0f ? (tv < (float)res ? (int32_t)tv : res - 1) : 0;
    return (face * res + iv) * res + iu;
}

struct GainArgs {
    const float* dirs;   // the cache's direction copy, 16 B per slot
    const float* cube;   // [cube_bands][6][res][res] f32 in [0, 1]
    float* plane;        // [slot][band_width(n_bands)] f32; the padding 0
    uint64_t n;          // slots
    float m[9];
    int32_t res;         // 1 .. kDirectivityMaxRes
    int32_t cube_bands;  // 1 (serves every band) or n_bands
    int32_t n_bands;     // 1 .. kMaxBands
};

// The plane for a recording of a.n rays, a lane per slot.
hipError_t launch_source_gain(const GainArgs& a, hipStream_t s);

}  // namespace arx
