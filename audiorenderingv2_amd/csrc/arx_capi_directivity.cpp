// arx_capi_directivity.cpp -- source directivity behind the C ABI (include/arx.h): the pattern (a cube map per
// band) and its rule, the orientation, the lookup's host definition (arx_directivity_gains_host, on
// arx_directivity.hpp's one function), and the gain plane the directed band replays start from
// (source_gain_kernel, arx_directivity.hip) with the generation words that say when it must be remade.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "arx_directivity.hpp"
#include "arx_internal.hpp"

using namespace arx;

namespace {

const float kIdentity[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};

uint64_t cube_floats(int32_t n_bands, int32_t res) {
    return (uint64_t)n_bands * kDirectivityFaces * (uint64_t)res * (uint64_t)res;
}

// The rule for a pattern: 1..kMaxBands bands, res in [1, 256], every value in [0, 1] (false for a NaN).
arx_status check_cube(const float* cube, int32_t n_bands, int32_t res) {
    if (n_bands < 1 || n_bands > kMaxBands) return fail(ARX_ERR_INVALID_ARGUMENT, "directivity: n_bands %d: 1..%d", n_bands, kMaxBands);
    if (res < 1 || res > kDirectivityMaxRes) return fail(ARX_ERR_INVALID_ARGUMENT, "directivity: res %d: 1..%d", res, kDirectivityMaxRes);
    if (!cube) return fail(ARX_ERR_INVALID_ARGUMENT, "directivity: cube is NULL");
    const uint64_t per_face = (uint64_t)res * (uint64_t)res, per_band = kDirectivityFaces * per_face;
    for (uint64_t i = 0; i < cube_floats(n_bands, res); ++i) {
        const float g = cube[i];
        if (!(g >= 0.0f && g <= 1.0f)) {
            const uint64_t t = i % per_band;
            return fail(ARX_ERR_INVALID_ARGUMENT, "directivity: band %d, texel (face %d, v %d, u %d): gain %.9g is not in [0, 1]",
                        (int)(i / per_band), (int)(t / per_face), (int)(t % per_face / (uint64_t)res), (int)(t % (uint64_t)res),
                        (double)g);
        }
    }
    return ARX_OK;
}

// Rows orthonormal to 1e-5, in f64.
arx_status check_orientation(const float* m) {
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double dot = 0.0;
            for (int k = 0; k < 3; ++k) dot += (double)m[3 * i + k] * (double)m[3 * j + k];
            if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-5))  // a NaN fails
                return fail(ARX_ERR_INVALID_ARGUMENT, "source orientation: rows %d and %d have dot product %.9g: not orthonormal to 1e-5",
                            i, j, dot);
        }
    return ARX_OK;
}

}  // namespace

arx_status arx::directivity_check_bands(const arx_renderer* r, int32_t n_bands) {
    const int32_t p = r->directivity.n_bands;
    if (p > 1 && p != n_bands)
        return fail(ARX_ERR_INVALID_ARGUMENT, "the source pattern has %d bands and the band table %d: one band, or as many", p, n_bands);
    return ARX_OK;
}

arx_status arx::directivity_plane(arx_renderer* r, const void* dirs, uint64_t n, int32_t n_bands, const float** plane) {
    DirectivityState& d = r->directivity;
    *plane = nullptr;
    if (d.n_bands < 1) return ARX_OK;
    if (const arx_status st = directivity_check_bands(r, n_bands); st != ARX_OK) return st;
    if (!dirs || n < 1 || n_bands < 1 || n_bands > kMaxBands) return fail(ARX_ERR_INTERNAL, "directivity plane: no recording");
    const uint64_t rec = r->path_cache.rec_gen;
    const uint64_t need = n * (uint64_t)band_width(n_bands);  // floats
    if (need > d.d_plane.cap) {
        d.plane_valid = false;
        if (const arx_status st = d.d_plane.reserve(need); st != ARX_OK) return st;
    }
    if (!d.plane_valid || d.made_pattern != d.pattern_gen || d.made_orient != d.orient_gen || d.made_rec != rec ||
        d.made_rays != n || d.made_bands != n_bands) {
        d.plane_valid = false;
        GainArgs g;
        std::memset(&g, 0, sizeof(g));
        g.dirs = static_cast<const float*>(dirs);
        g.cube = d.d_cube.p;
        g.plane = d.d_plane.p;
        g.n = n;
        std::memcpy(g.m, d.m, sizeof(g.m));
        g.res = d.res;
        g.cube_bands = d.n_bands;
        g.n_bands = n_bands;
        ARX_HIP(launch_source_gain(g, r->stream));
        d.made_pattern = d.pattern_gen;
        d.made_orient = d.orient_gen;
        d.made_rec = rec;
        d.made_rays = n;
        d.made_bands = n_bands;
        d.plane_valid = true;
        ++d.planes_made;
    }
    *plane = d.d_plane.p;
    return ARX_OK;
}

extern "C" {

arx_status arx_set_source_directivity(arx_renderer* r, const float* cube, int32_t n_bands, int32_t res) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    DirectivityState& d = r->directivity;
    if (n_bands == 0) {
        d.n_bands = 0;
        ++d.pattern_gen;
        return ARX_OK;
    }
    if (const arx_status st = check_cube(cube, n_bands, res); st != ARX_OK) return st;
    ARX_HIP(hipSetDevice(r->cfg.device));
    d.n_bands = 0;  // a device error below drops the pattern
    ++d.pattern_gen;
    const uint64_t need = cube_floats(n_bands, res);
    // no call is in flight: every band call ends synchronised
    if (const arx_status st = d.d_cube.reserve(need); st != ARX_OK) return st;
    ARX_HIP(hipMemcpy(d.d_cube.p, cube, need * sizeof(float), hipMemcpyHostToDevice));
    d.n_bands = n_bands;
    d.res = res;
    return ARX_OK;
}

arx_status arx_set_source_orientation(arx_renderer* r, const float* m9) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (!m9) return fail(ARX_ERR_INVALID_ARGUMENT, "source orientation: m9 is NULL");
    if (const arx_status st = check_orientation(m9); st != ARX_OK) return st;
    DirectivityState& d = r->directivity;
    if (std::memcmp(d.m, m9, sizeof(d.m)) != 0) {
        std::memcpy(d.m, m9, sizeof(d.m));
        ++d.orient_gen;
    }
    return ARX_OK;
}

int32_t arx_source_directivity_bands(const arx_renderer* r) { return r ? r->directivity.n_bands : 0; }

arx_status arx_directivity_gains_host(const float* cube, int32_t n_bands, int32_t res, const float* m9, const float* dirs_xyz,
                                      uint64_t n, int32_t width, float* out) {
    if (const arx_status st = check_cube(cube, n_bands, res); st != ARX_OK) return st;
    if (width != 4 && width != 8) return fail(ARX_ERR_INVALID_ARGUMENT, "directivity: width %d: 4 or 8", width);
    if (n_bands > width) return fail(ARX_ERR_INVALID_ARGUMENT, "directivity: %d bands do not fit a row of %d", n_bands, width);
    const float* m = m9 ? m9 : kIdentity;
    if (const arx_status st = check_orientation(m); st != ARX_OK) return st;
    if (n > 0 && (!dirs_xyz || !out)) return fail(ARX_ERR_INVALID_ARGUMENT, "directivity: NULL directions or output");
    const uint64_t per_band = cube_floats(1, res);
    const int32_t filled = n_bands == 1 ? width : n_bands;  // a one-band cube serves every band
    for (uint64_t i = 0; i < n; ++i) {
        const float* d = dirs_xyz + 3 * i;
        const int32_t texel = directivity_texel(m, d[0], d[1], d[2], res);
        float* row = out + (uint64_t)width * i;
        for (int32_t b = 0; b < width; ++b)
            row[b] = (b < filled && texel >= 0) ? cube[(uint64_t)(n_bands == 1 ? 0 : b) * per_band + (uint64_t)texel] : 0.0f;
    }
    return ARX_OK;
}

arx_status arx_debug_directivity_plane(arx_renderer* r, uint64_t first_ray, uint64_t count, float* h_out) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (count > 0 && !h_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL output");
    DirectivityState& d = r->directivity;
    const PathCache& pc = r->path_cache;
    if (d.n_bands < 1) return fail(ARX_ERR_NOT_READY, "arx_set_source_directivity has not been called");
    if (!pc.recorded || !pc.d_dirs.p || pc.rec_rays == 0) return fail(ARX_ERR_NOT_READY, "the path cache holds no recording to make a plane from");
    if (r->stream != r->cur().stream) return fail(ARX_ERR_INVALID_ARGUMENT, "the plane is made on the renderer's own stream");
    // the band count the next band call will run with: the table's, or without a table the pattern's
    const int32_t B = r->bands.n_bands >= 1 ? r->bands.n_bands : d.n_bands;
    if (const arx_status st = directivity_check_bands(r, B); st != ARX_OK) return st;
    if (first_ray > pc.rec_rays || count > pc.rec_rays - first_ray)
        return fail(ARX_ERR_INVALID_ARGUMENT, "the plane holds %llu rays", (unsigned long long)pc.rec_rays);
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (pc.rec_stream != r->stream) ARX_HIP(hipStreamWaitEvent(r->stream, pc.ev_recorded, 0));
    const float* plane = nullptr;
    if (const arx_status st = directivity_plane(r, pc.d_dirs.p, pc.rec_rays, B, &plane); st != ARX_OK) return st;
    const uint64_t W = (uint64_t)band_width(B);
    if (count > 0)
        ARX_HIP(hipMemcpyAsync(h_out, plane + first_ray * W, count * W * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

uint64_t arx_debug_directivity_bytes(uint64_t n_rays, int32_t n_bands, int32_t res) {
    if (n_bands < 1 || n_bands > kMaxBands || res < 1 || res > kDirectivityMaxRes) return 0;
    return n_rays * (uint64_t)band_width(n_bands) * sizeof(float) + cube_floats(n_bands, res) * sizeof(float);
}

uint64_t arx_debug_directivity_planes_made(const arx_renderer* r) { return r ? r->directivity.planes_made : 0; }

}  // extern "C"
