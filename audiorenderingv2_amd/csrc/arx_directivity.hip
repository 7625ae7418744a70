// arx_directivity.hip -- source_gain_kernel: the gain plane of a source pattern (arx_set_source_directivity,
// include/arx.h) for the path cache's recorded rays.  The lookup itself is arx_directivity.hpp's, the same
// function the host definition (arx_directivity_gains_host) runs.
#include <hip/hip_runtime.h>

#include "arx_bands.hpp"
#include "arx_directivity.hpp"

namespace arx {
namespace {

// A lane per recorded slot: the slot's direction (16 B of the cache's copy), its texel, and per band that
// texel's gain -- W floats in one or two 16-B stores, the bands past n_bands 0.  The texel index is below
// 6 * res * res by construction (directivity_texel clamps both coordinates), the band below cube_bands.
template <int W>
__global__ __launch_bounds__(256) void source_gain_kernel(GainArgs a) {
    static_assert(W == 4 || W == 8, "a plane row is one or two 16-B stores");
    const uint64_t slot = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= a.n) return;
    const float4 d = reinterpret_cast<const float4*>(a.dirs)[slot];
    const int32_t texel = directivity_texel(a.m, d.x, d.y, d.z, a.res);
    const uint64_t band_texels = (uint64_t)kDirectivityFaces * (uint64_t)a.res * (uint64_t)a.res;
    float g[W];
#pragma unroll
    for (int b = 0; b < W; ++b) {
        g[b] = 0.0f;
        if (b < a.n_bands && texel >= 0) g[b] = a.cube[(uint64_t)(a.cube_bands == 1 ? 0 : b) * band_texels + (uint64_t)texel];
    }
    float4* row = reinterpret_cast<float4*>(a.plane) + slot * (W / 4);
#pragma unroll
    for (int q = 0; q < W / 4; ++q) row[q] = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
}

}  // namespace

hipError_t launch_source_gain(const GainArgs& a, hipStream_t s) {
    (void)hipGetLastError();
    if (!a.dirs || !a.cube || !a.plane || a.n < 1 || a.res < 1 || a.res > kDirectivityMaxRes || a.n_bands < 1 ||
        a.n_bands > kMaxBands || (a.cube_bands != 1 && a.cube_bands != a.n_bands) || (a.n + 255) / 256 > 0x7fffffffull)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n + 255) / 256));
    if (band_width(a.n_bands) == 4)
        hipLaunchKernelGGL(source_gain_kernel<4>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(source_gain_kernel<8>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace arx
