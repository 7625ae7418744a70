// arx_capi_listener_bands.cpp -- band IRs for a batch of listeners behind the C ABI
// (arx_render_listener_bands, include/arx.h): the listener batch's driver and chunks of receiver slots
// (run_listener_call, arx_capi_listeners.cpp) answered by the band chain (band_base_kernel /
// band_cand_multi_kernel, arx_replay.hip), every (listener, band) finalized and analysed as arx_render_bands
// does it and, with a filter bank, every listener's bands summed into one broadband pair (band_synth_kernel);
// the poses the batch cannot take go through arx_set_listener + arx_render_bands (+ arx_combine_bands) one by
// one.  What is here is what differs from arx_render_listeners.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

namespace {

struct BandCall : ListenerCall {
    const double* filters;
    int32_t taps;
    float* bb_left;
    float* bb_right;
    arx_listener_band_result* results;
    std::vector<arx_band_result> single;  // per (pose, band) of the one-listener route
    std::vector<float> tmp_ir;            // that route's band IRs when the caller takes only the broadband pair
    const float* gain = nullptr;          // begin_chunks: the gain plane of a source pattern for this call, or null
    const float* air = nullptr;           // begin_chunks: air absorption's table for this call, or null
};

// The one-listener route: the loop's own step, straight into the caller's arrays; it ends synchronised.
arx_status render_single(ListenerCall& lc, size_t j) {
    BandCall& c = static_cast<BandCall&>(lc);
    arx_renderer* r = c.r;
    const arx_listener_pose& p = c.poses[j];
    const size_t B = (size_t)c.bands, set = B * c.ir_len;
    float* il = c.ir_left ? c.ir_left + j * set : nullptr;
    float* irr = c.ir_right ? c.ir_right + j * set : nullptr;
    if (c.filters && !il) {
        c.tmp_ir.resize(2 * set);
        il = c.tmp_ir.data();
        irr = il + set;
    }
    arx_status st = arx_set_listener(r, p.x, p.y, p.z, p.yaw_deg);
    if (st == ARX_OK)
        st = arx_render_bands(r, il, irr, c.acoustics ? c.acoustics + j * B * 3 : nullptr, c.single.data() + j * B, nullptr);
    if (st == ARX_OK && c.filters)
        st = arx_combine_bands(r, il, irr, c.bands, c.ir_len, c.filters, c.taps, c.bb_left + j * c.ir_len,
                               c.bb_right + j * c.ir_len, nullptr);
    if (st != ARX_OK) return st;
    c.warm += c.single[j * B].warm_launches;
    c.route[j] = ARX_LISTENER_SINGLE;
    return ARX_OK;
}

// 1. the recording: ordinary launches at the first pose until the cache holds the key's records
arx_status warm_up(ListenerCall& c) { return record_for_bands(c.r, c.N, &c.poses[0], &c.probe, &c.warm); }

BandArgs band_args(const ListenerCall& lc) {
    const BandCall& c = static_cast<const BandCall&>(lc);
    BandArgs ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.table = c.r->bands.d_table.p;
    ba.counters = c.at<unsigned long long>(c.sc.base);
    ba.n_tris = c.r->bands.n_tris;
    ba.n_bands = c.bands;
    // a source pattern's plane and air absorption's table, as begin_chunks got them for this call
    ba.gain = c.gain;
    ba.air = c.air;
    return ba;
}

// In front of the chunks, once: the call's filter bank, while the stream is still idle (the copy reads pageable
// memory), and the bands' base counts.
arx_status begin_chunks(ListenerCall& lc) {
    BandCall& c = static_cast<BandCall&>(lc);
    arx_renderer* r = c.r;
    if (c.filters)
        ARX_HIP(hipMemcpyAsync(c.own->d_filters.p, c.filters, (size_t)c.bands * (size_t)c.taps * sizeof(double), hipMemcpyDefault,
                               r->stream));
    // the gain plane of a source pattern and air absorption's table, each remade only when stale (band_args hands them on)
    if (const arx_status st = directivity_plane(r, c.probe.args.dirs, c.N, c.bands, &c.gain); st != ARX_OK) return st;
    if (const arx_status st = air_table(r, c.bands, &c.air); st != ARX_OK) return st;
    ARX_HIP(launch_band_base(c.probe.args, filter_args(c.probe, c.fgrow), band_args(c), c.at<char>(c.sc.counts), r->stream));
    return ARX_OK;
}

// The chunk's replay for every band.
arx_status replay(ListenerCall& c, const ListenerEntry* d_table, size_t, int32_t J) {
    ARX_HIP(launch_listener_bands_replay(c.probe.args, filter_args(c.probe, c.fgrow), d_table, J, band_args(c),
                                         c.at<char>(c.sc.counts), c.r->stream));
    return ARX_OK;
}

// Chunk slot i's bands summed into its broadband pair, and that pair queued for pose j.
arx_status combine(ListenerCall& lc, int32_t i, size_t j) {
    BandCall& c = static_cast<BandCall&>(lc);
    const size_t L = c.ir_len, set = (size_t)c.bands * L;
    BandSynthArgs a{};
    a.ir_left = c.at<float>(c.sc.ir) + (size_t)i * set;
    a.ir_right = a.ir_left + (size_t)c.chunk * set;
    a.filters = c.own->d_filters.p;
    a.out_left = c.at<float>(c.sc.bb) + (size_t)i * L;
    a.out_right = a.out_left + (size_t)c.chunk * L;
    a.ir_len = (int64_t)L;
    a.n_bands = c.bands;
    a.taps = c.taps;
    ARX_HIP(launch_band_synth(a, c.r->stream));
    ARX_HIP(hipMemcpyAsync(c.bb_left + j * L, a.out_left, L * sizeof(float), hipMemcpyDefault, c.r->stream));
    ARX_HIP(hipMemcpyAsync(c.bb_right + j * L, a.out_right, L * sizeof(float), hipMemcpyDefault, c.r->stream));
    return ARX_OK;
}

void write_outputs(const ListenerCall& lc) {
    const BandCall& c = static_cast<const BandCall&>(lc);
    const size_t B = (size_t)c.bands;
    for (size_t j = 0; j < c.n; ++j) {
        const bool batched = c.route[j] == ARX_LISTENER_BATCHED;
        const unsigned long long* hc = c.h_counters + c.where[j] * batch_counter_words(c.bands);
        for (size_t b = 0; b < B && c.results; ++b) {
            arx_listener_band_result& o = c.results[j * B + b];
            std::memset(&o, 0, sizeof(o));
            const arx_band_result& s = c.single[j * B + b];
            o.queries = batched ? hc[b * kBandCounterWords + 0] : s.queries;
            o.receiver_hits = batched ? hc[b * kBandCounterWords + 1] : s.receiver_hits;
            o.misses = batched ? hc[b * kBandCounterWords + 2] : s.misses;
            o.candidate_rays = batched ? hc[B * kBandCounterWords] : 0;
            o.route = c.route[j];
            o.warm_launches = c.warm;
        }
        if (c.acoustics && batched)
            std::memcpy(c.acoustics + 3 * B * j, c.h_res + 3 * B * c.where[j], 3 * B * sizeof(arx_acoustics));
    }
}

}  // namespace

extern "C" {

arx_status arx_render_listener_bands(arx_renderer* r, const arx_listener_pose* poses, size_t n, float* ir_left, float* ir_right,
                                     const double* filters, int32_t taps, float* bb_left, float* bb_right,
                                     arx_acoustics* acoustics, arx_listener_band_result* results, double* ms) {
    if (const arx_status st = check_batch_args(r, poses, n, ir_left, ir_right, filters, taps, bb_left, bb_right); st != ARX_OK || n == 0)
        return st;
    if (r->bands.n_bands < 1) return fail(ARX_ERR_NOT_READY, "arx_set_band_absorption has not been called for this scene");
    if (r->path_cache.mode != 1) return fail(ARX_ERR_NOT_READY, "a band render replays the path cache, which is off");
    const int32_t B = r->bands.n_bands;
    if (const arx_status st = directivity_check_bands(r, B); st != ARX_OK) return st;
    if (const arx_status st = air_check_bands(r, B); st != ARX_OK) return st;
    BandCall c{{r, &r->listener_bands, poses, n, ir_left, ir_right, acoustics, B, false, ir_left || filters, warm_up, render_single,
                begin_chunks, replay, filters ? combine : nullptr, write_outputs},
               filters, filters ? taps : 0, bb_left, bb_right, results};
    c.N = n_rays(r->cfg);
    if (c.N == 0) return fail(ARX_ERR_NOT_READY, "a launch of no rays is not cacheable");
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (filters)
        if (const arx_status st = r->listener_bands.d_filters.reserve((uint64_t)B * (uint64_t)taps); st != ARX_OK) return st;
    c.single.assign(n * (size_t)B, arx_band_result{});
    return run_listener_call(c, ms != nullptr, ms);  // timed around the whole call, its warm launches included
}

uint64_t arx_debug_listener_band_bytes(uint64_t n_rays, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t n_bands,
                                       int32_t listeners) {
    if (ir_len < 0 || recv_nodes < 0 || recv_tris < 0 || listeners < 0 || n_bands < 1 || n_bands > kMaxBands) return 0;
    return (uint64_t)listeners * batch_bytes_each(n_rays, ir_len, recv_nodes, recv_tris, n_bands) + batch_bytes_fixed(n_rays, n_bands);
}

}  // extern "C"
