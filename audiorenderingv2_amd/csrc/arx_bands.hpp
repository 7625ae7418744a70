// arx_bands.hpp -- frequency-band absorption (arx_render_bands, include/arx.h): the arguments of
// band_replay_kernel (arx_replay.hip) and the layout of the call's scratch.
//
// A band is the scene with another absorption per triangle.  A specular ray's geometry does not depend on
// absorption, so one walk over a ray's recorded hits carries every band's energy into that band's own
// histogram: the band arguments ride beside the TraceArgs of the replay as a second kernel parameter.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "arx_batch_plan.hpp"  // kMaxBands, kBandCounterWords
#include "arx_layout.hpp"

namespace arx {

// The compiled width that serves n_bands: the device table's row, so a hit fetches its bands in one or
// two 16-B loads.
ARX_HOST_DEVICE inline int32_t band_width(int32_t n_bands) { return n_bands <= 4 ? 4 : 8; }

struct BandArgs {
    const float* table;            // [triangle][band_width(n_bands)] f32 absorption, by global triangle id; padding 0
    unsigned long long* hist;      // band b's [L | R] histogram at hist + b * 2 * ir_len
    unsigned long long* counters;  // band b's block at counters + b * kBandCounterWords
    int64_t n_tris;                // rows of the table (the scene's input triangles), >= 1
    int32_t n_bands;               // 1 .. kMaxBands
    int32_t pad;
    // Source directivity (arx_directivity.hpp): the gain plane [slot][band_width(n_bands)] of the recording's
    // rays, or null.  With a plane the launchers take the kernels' DIRECTED instantiations, in which a ray's
    // band b starts from e0 * gain[slot][b]; without one, the instantiations that never read this field.
    const float* gain;
    // Air absorption (include/arx.h): the attenuation table [bin][band_width(n_bands)], ir_len rows, or null.
    // Padding columns are 0; a one-coefficient install fills every column.  With a table the launchers take the
    // depositing kernels' AIR instantiations, in which a receiver deposit of band b in bin k is weighted by
    // air[k][b]; without one, the instantiations that never read this field.
    const float* air;
};
static_assert(sizeof(BandArgs) == 56, "BandArgs: a kernel parameter behind TraceArgs");

// The scratch of a call for n_bands bands, as byte offsets (every region 16-B aligned): per band a
// histogram, a counter block, three arx_acoustics and an f32 IR pair (the lefts, then the rights); then one
// decay-curve buffer and the analysis kernels' scratch.
struct BandScratchLayout {
    uint64_t hist, counters, res, ir, edc, acou, total;
};
BandScratchLayout band_scratch_layout(int32_t ir_len, int32_t n_bands);

// The frame of every band from launch_path_record's records (band_replay_kernel): a is the replay's
// arguments (dirs and rec the cache's; its hist and counters are not used), with the clear of the bands'
// histograms and counter blocks in front.  Band b's histogram and counters are those of
// launch_path_replay on a scene whose triangles carry table[.][b].
hipError_t launch_band_replay(const TraceArgs& a, const BandArgs& b, hipStream_t s);

// A batch of listeners per band (arx_render_listener_bands; band_base_kernel / band_cand_multi_kernel).
// A listener's bands' block is BandArgs' layout behind its ListenerEntry: entry.hist the bands' histograms,
// entry.counters the bands' counter blocks; entry.cand lies behind them.
// launch_band_base, once per call: per ray the queries each band makes along the scene-only recording, a
// byte per band packed into `counts` (8 B per ray), and their sums in b.counters (cleared first; band b's at
// b.counters + b * kBandCounterWords).  f.planes is the recording's filter state; b.hist is not used.
hipError_t launch_band_base(const TraceArgs& a, const FilterArgs& f, const BandArgs& b, void* counts, hipStream_t s);
// launch_listeners_replay for every band at once: the same filter pass and work items, then the band chain
// over the candidates and the chunk's query counts from b.counters (launch_band_base's block) and `counts`.
// Per listener and band the results are launch_band_replay's at that listener.  No clear: the caller clears
// the chunk's blocks.
hipError_t launch_listener_bands_replay(const TraceArgs& a, const FilterArgs& f, const ListenerEntry* d_table,
                                        int32_t listeners, const BandArgs& b, const void* counts, hipStream_t s);

}  // namespace arx
