// arx_capi_listener_bands.cpp -- band IRs for a batch of listeners behind the C ABI
// (arx_render_listener_bands, include/arx.h): the listener batch's chunks of receiver slots
// (arx_capi_listeners.cpp) answered by the band chain (band_base_kernel / band_cand_multi_kernel,
// arx_replay.hip), every (listener, band) finalized and analysed as arx_render_bands does it and, with a
// filter bank, every listener's bands summed into one broadband pair (band_synth_kernel); the poses the
// batch cannot take go through arx_set_listener + arx_render_bands (+ arx_combine_bands) one by one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

namespace {

// a listener's counter block: a kBandCounterWords block per band, then one for its candidate tally
uint64_t counter_words(int32_t B) { return ((uint64_t)B + 1) * kBandCounterWords; }

// arx_debug_listener_band_bytes' terms (include/arx.h)
uint64_t bytes_each(uint64_t n, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t B) {
    const uint64_t L = (uint64_t)ir_len;
    return listener_slot_bytes(recv_nodes, recv_tris) + sizeof(ListenerEntry) + path_filter_list_bytes(n) +
           4 * listener_work_words(n) + (uint64_t)B * (24 * L + kBandCounterWords * 8 + 3 * sizeof(arx_acoustics)) +
           kBandCounterWords * 8 + 8 * L;
}
uint64_t bytes_fixed(uint64_t n) { return 8 * n + (uint64_t)kMaxBands * kBandCounterWords * 8; }

// The call's scratch as byte offsets, every region 16-B aligned: what does not depend on the chunk first.
struct Scratch {
    uint64_t counts, base, edc, acou, lists, list_stride, work, work_stride, table, hist, counters, res, ir, bb, total;
};
Scratch scratch_layout(uint64_t n, int32_t ir_len, int32_t B, int32_t chunk) {
    Scratch s;
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 15) & ~15ull;
        return o;
    };
    const uint64_t J = (uint64_t)chunk, L = (uint64_t)ir_len;
    s.counts = take(8 * n);
    s.base = take((uint64_t)kMaxBands * kBandCounterWords * 8);
    s.edc = take(24 * L);
    s.acou = take(acoustics_scratch_bytes());
    s.list_stride = path_filter_list_bytes(n);
    s.lists = take(J * s.list_stride);
    s.work_stride = 4 * listener_work_words(n);
    s.work = take(J * s.work_stride);
    s.table = take(J * sizeof(ListenerEntry));
    s.hist = take(J * (uint64_t)B * 16 * L);
    s.counters = take(J * counter_words(B) * 8);
    s.res = take(J * (uint64_t)B * 3 * sizeof(arx_acoustics));
    s.ir = take(J * (uint64_t)B * 8 * L);  // the chunk's left IRs [listener][band], then its right IRs
    s.bb = take(J * 8 * L);                // the chunk's broadband lefts, then its rights
    s.total = at;
    return s;
}

// The pinned block of a call of n listeners and B bands: table entries by batched order, then counter blocks
// and results by batched order, then the tree's off-grid flag as the chunks left it.
struct Pinned {
    ListenerEntry* entries;
    unsigned long long* counters;
    arx_acoustics* res;
    unsigned int* flag;
};
size_t pinned_bytes(size_t n, int32_t B) {
    return n * sizeof(ListenerEntry) + n * counter_words(B) * 8 + n * (size_t)B * 3 * sizeof(arx_acoustics) + 16;
}
Pinned pinned(void* base, size_t n, int32_t B) {
    Pinned p;
    char* c = static_cast<char*>(base);
    p.entries = reinterpret_cast<ListenerEntry*>(c);
    c += n * sizeof(ListenerEntry);
    p.counters = reinterpret_cast<unsigned long long*>(c);
    c += n * counter_words(B) * 8;
    p.res = reinterpret_cast<arx_acoustics*>(c);
    c += n * (size_t)B * 3 * sizeof(arx_acoustics);
    p.flag = reinterpret_cast<unsigned int*>(c);
    return p;
}

// One arx_render_listener_bands call: its arguments, and what its steps hand each other.
struct Call {
    arx_renderer* r;
    const arx_listener_pose* poses;
    size_t n;
    float* ir_left;
    float* ir_right;
    const double* filters;
    int32_t taps;
    float* bb_left;
    float* bb_right;
    arx_acoustics* acoustics;
    arx_listener_band_result* results;
    int32_t B = 0;               // bands of the installed table
    uint64_t N = 0;              // rays of a frame
    size_t ir_len = 0;
    int32_t warm = 0;
    Pinned pin{};
    std::vector<int32_t> route;  // per pose
    std::vector<size_t> batched; // the batched poses, in batched order
    std::vector<arx_band_result> single;  // per (pose, band) of the one-listener route
    std::vector<float> tmp_ir;   // that route's band IRs when the caller takes only the broadband pair
    ReplayProbe probe;
    ListenerSlots sl;
    int32_t chunk = 0;
    Scratch sc{};
    char* d_base = nullptr;
    float fgrow = 0.0f;
};

// The one-listener route: the loop's own step, straight into the caller's arrays.
arx_status render_single(Call& c, size_t j) {
    arx_renderer* r = c.r;
    const arx_listener_pose& p = c.poses[j];
    const size_t set = (size_t)c.B * c.ir_len;
    float* il = c.ir_left ? c.ir_left + j * set : nullptr;
    float* irr = c.ir_right ? c.ir_right + j * set : nullptr;
    if (c.filters && !il) {
        c.tmp_ir.resize(2 * set);
        il = c.tmp_ir.data();
        irr = il + set;
    }
    arx_status st = arx_set_listener(r, p.x, p.y, p.z, p.yaw_deg);
    if (st == ARX_OK)
        st = arx_render_bands(r, il, irr, c.acoustics ? c.acoustics + j * (size_t)c.B * 3 : nullptr,
                              c.single.data() + j * (size_t)c.B, nullptr);
    if (st == ARX_OK && c.filters)
        st = arx_combine_bands(r, il, irr, c.B, c.ir_len, c.filters, c.taps, c.bb_left + j * c.ir_len,
                               c.bb_right + j * c.ir_len, nullptr);
    if (st != ARX_OK) return st;
    c.warm += c.single[j * (size_t)c.B].warm_launches;
    c.route[j] = ARX_LISTENER_SINGLE;
    return ARX_OK;
}

// 1. the recording: ordinary launches at the first pose until the cache holds the key's records, as
// arx_render_bands runs them
arx_status warm_up(Call& c) {
    arx_renderer* r = c.r;
    arx_status st;
    for (;;) {
        if ((st = trace_rays(r, 0, c.N, false, false, &c.probe)) != ARX_OK) return st;
        if (c.probe.recorded) return ARX_OK;
        const int32_t would = c.probe.state;  // what the next launch would do
        if (would == kPathOff) return fail(ARX_ERR_NOT_READY, "a band render replays the path cache, which is off");
        if (would == kPathNotCacheable)
            return fail(ARX_ERR_NOT_READY, "this launch is not cacheable (global stack, CW4 or f32 nodes): no records to replay");
        if (would == kPathOverCap)
            return fail(ARX_ERR_NOT_READY,
                        "the launch's records (%llu B) are over the path cache's cap or do not fit on the device "
                        "(arx_debug_set_path_cache max_bytes)",
                        (unsigned long long)arx_debug_path_cache_bytes(c.N, r->cfg.max_bounces));
        if (c.warm == 3) return fail(ARX_ERR_NOT_READY, "the path cache did not record within three launches");
        if (c.warm == 0 && (st = arx_set_listener(r, c.poses[0].x, c.poses[0].y, c.poses[0].z, c.poses[0].yaw_deg)) != ARX_OK)
            return st;
        if ((st = arx_render(r, nullptr)) != ARX_OK) return st;
        ++c.warm;
    }
}

bool scratch_reserve(arx_renderer* r, uint64_t need) {
    ListenerBandBatch& lb = r->listener_bands;
    if (lb.d_scratch && lb.scratch_bytes >= need) return true;
    if (known_no_room(lb.no_room, need) || sync_renderer(r) != ARX_OK) return false;
    return grow_device_optional(&lb.d_scratch, &lb.scratch_bytes, need, need, &lb.no_room);
}

// 2. the batch: grid, slots and scratch before the first launch; any "no" sends every pose through the loop
arx_status prepare_batch(Call& c, bool* batch) {
    arx_renderer* r = c.r;
    arx_status st;
    *batch = c.probe.ready && r->recv_refit && !r->recv.tris.empty() && !r->use_w4 &&
             r->cfg.max_bounces <= kFilterMaxBounces;
    if (!*batch) return ARX_OK;
    if ((st = listener_grid_for(r, c.poses, 0, c.n)) != ARX_OK) return st;
    c.sl = listener_slots(r);
    const uint64_t each = bytes_each(c.N, r->ir_len, c.sl.recv_nodes, c.sl.recv_tris, c.B), fixed = bytes_fixed(c.N);
    const int32_t forced = r->listeners.forced_chunk;
    c.chunk = forced > 0 ? forced
                         : (int32_t)std::min<uint64_t>(kListenerChunkMax, kListenerBudget > fixed ? (kListenerBudget - fixed) / each : 0);
    c.chunk = (int32_t)std::min<size_t>((size_t)c.chunk, c.n);
    c.sl.chunk = c.chunk;
    if (c.chunk < 1) {
        *batch = false;
        return ARX_OK;
    }
    const ListenerLayout last = c.sl.layout(c.chunk - 1);
    c.sc = scratch_layout(c.N, r->ir_len, c.B, c.chunk);
    *batch = listener_slots_valid(r, c.sl) && widen_tree_arrays(r, (size_t)last.total_nodes, (size_t)last.total_tris) &&
             scratch_reserve(r, c.sc.total);
    if (!*batch) return ARX_OK;
    // the arrays may have moved and the grid grown: the replay's arguments as they stand now
    if ((st = trace_rays(r, 0, c.N, false, false, &c.probe)) != ARX_OK) return st;
    *batch = c.probe.ready;
    c.d_base = static_cast<char*>(r->listener_bands.d_scratch);
    c.fgrow = path_filter_grow(c.probe.args.qgrid);
    return ARX_OK;
}

// Each batched pose's table entry, in batched order, with the slot of its chunk it runs in.
void select_batched(Call& c) {
    const Scratch& sc = c.sc;
    const uint64_t L = (uint64_t)c.ir_len;
    for (size_t j = 0; j < c.n; ++j) {
        if (!listener_pose_batchable(c.r, c.poses[j], c.fgrow)) continue;
        const size_t b = c.batched.size();
        const uint64_t slot = b % (size_t)c.chunk;
        ListenerEntry& e = c.pin.entries[b];
        listener_entry_place(c.r, c.sl, (int32_t)slot, c.poses[j], &e);
        e.hist = reinterpret_cast<unsigned long long*>(c.d_base + sc.hist) + slot * (uint64_t)c.B * 2 * L;
        e.counters = reinterpret_cast<unsigned long long*>(c.d_base + sc.counters) + slot * counter_words(c.B);
        e.cand = e.counters + (uint64_t)c.B * kBandCounterWords;
        e.list = reinterpret_cast<FilterCand*>(c.d_base + sc.lists + slot * sc.list_stride);
        e.heads = e.list + c.N;
        e.work = reinterpret_cast<unsigned int*>(c.d_base + sc.work + slot * sc.work_stride);
        c.route[j] = ARX_LISTENER_BATCHED;
        c.batched.push_back(j);
    }
}

BandArgs band_args(const Call& c) {
    BandArgs ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.table = c.r->bands.d_table;
    ba.counters = reinterpret_cast<unsigned long long*>(c.d_base + c.sc.base);
    ba.n_tris = c.r->bands.n_tris;
    ba.n_bands = c.B;
    return ba;
}

// One chunk, on the one stream: the batched poses [c0, c0 + J) refit into their slots, replayed for every
// band, finalized, analysed and combined, and their outputs queued.
arx_status issue_chunk(Call& c, size_t c0, int32_t J) {
    arx_renderer* r = c.r;
    const Scratch& sc = c.sc;
    const size_t L = c.ir_len, B = (size_t)c.B, set = B * L;
    const double unit = ir_unit(r->cfg);
    ListenerEntry* d_table = reinterpret_cast<ListenerEntry*>(c.d_base + sc.table);
    unsigned long long* d_hist = reinterpret_cast<unsigned long long*>(c.d_base + sc.hist);
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(c.d_base + sc.counters);
    arx_acoustics* d_res = reinterpret_cast<arx_acoustics*>(c.d_base + sc.res);
    float* d_irl = reinterpret_cast<float*>(c.d_base + sc.ir);
    float* d_irr = d_irl + (size_t)c.chunk * set;
    float* d_bbl = reinterpret_cast<float*>(c.d_base + sc.bb);
    float* d_bbr = d_bbl + (size_t)c.chunk * L;
    const bool want_ir = c.ir_left || c.filters;
    ARX_HIP(hipMemcpyAsync(d_table, c.pin.entries + c0, (size_t)J * sizeof(ListenerEntry), hipMemcpyHostToDevice, r->stream));
    ARX_HIP(launch_clear(d_hist, (uint64_t)J * B * 2 * L, d_cnt, (int)((uint64_t)J * counter_words(c.B)), r->stream));
    ARX_HIP(launch_receiver_refit_multi(refit_args(r), d_table, J, r->stream));
    FilterArgs fa;
    fa.planes = c.probe.planes;
    fa.list = nullptr;  // per listener, from the table
    fa.heads = nullptr;
    fa.grow = c.fgrow;
    ARX_HIP(launch_listener_bands_replay(c.probe.args, fa, d_table, J, band_args(c), c.d_base + sc.counts, r->stream));
    for (int32_t i = 0; i < J; ++i) {
        const size_t j = c.batched[c0 + (size_t)i];
        for (size_t b = 0; b < B; ++b) {
            const long long* h = reinterpret_cast<const long long*>(d_hist + ((size_t)i * B + b) * 2 * L);
            if (want_ir)
                ARX_HIP(launch_finalize_ir(h, d_irl + (size_t)i * set + b * L, d_irr + (size_t)i * set + b * L, r->ir_len, unit,
                                           r->cfg.is_mono, r->stream));
            if (c.acoustics)
                ARX_HIP(launch_acoustics(acoustics_args(r, h, reinterpret_cast<long long*>(c.d_base + sc.edc),
                                                        d_res + 3 * ((size_t)i * B + b), c.d_base + sc.acou),
                                         r->stream));
        }
        if (c.ir_left) {
            ARX_HIP(hipMemcpyAsync(c.ir_left + j * set, d_irl + (size_t)i * set, set * sizeof(float), hipMemcpyDefault, r->stream));
            ARX_HIP(hipMemcpyAsync(c.ir_right + j * set, d_irr + (size_t)i * set, set * sizeof(float), hipMemcpyDefault, r->stream));
        }
        if (c.filters) {
            BandSynthArgs a{};
            a.ir_left = d_irl + (size_t)i * set;
            a.ir_right = d_irr + (size_t)i * set;
            a.filters = static_cast<const double*>(r->listener_bands.d_filters);
            a.out_left = d_bbl + (size_t)i * L;
            a.out_right = d_bbr + (size_t)i * L;
            a.ir_len = (int64_t)L;
            a.n_bands = c.B;
            a.taps = c.taps;
            ARX_HIP(launch_band_synth(a, r->stream));
            ARX_HIP(hipMemcpyAsync(c.bb_left + j * L, a.out_left, L * sizeof(float), hipMemcpyDefault, r->stream));
            ARX_HIP(hipMemcpyAsync(c.bb_right + j * L, a.out_right, L * sizeof(float), hipMemcpyDefault, r->stream));
        }
    }
    ARX_HIP(hipMemcpyAsync(c.pin.counters + c0 * counter_words(c.B), d_cnt, (size_t)J * counter_words(c.B) * 8,
                           hipMemcpyDeviceToHost, r->stream));
    if (c.acoustics)
        ARX_HIP(hipMemcpyAsync(c.pin.res + 3 * B * c0, d_res, (size_t)J * B * 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost,
                               r->stream));
    ARX_HIP(hipMemcpyAsync(c.pin.flag, r->d_tree_flag, sizeof(unsigned int), hipMemcpyDeviceToHost, r->stream));
    c.pin.flag[1] = r->tree_gen;
    return ARX_OK;
}

// the host-side outputs, after the call's last synchronisation
void write_outputs(const Call& c) {
    const size_t B = (size_t)c.B;
    std::vector<size_t> where(c.n, 0);
    for (size_t b = 0; b < c.batched.size(); ++b) where[c.batched[b]] = b;
    for (size_t j = 0; j < c.n; ++j) {
        const bool batched = c.route[j] == ARX_LISTENER_BATCHED;
        const unsigned long long* hc = c.pin.counters + where[j] * counter_words(c.B);
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
            std::memcpy(c.acoustics + 3 * B * j, c.pin.res + 3 * B * where[j], 3 * B * sizeof(arx_acoustics));
    }
}

arx_status render_listener_bands(Call& c) {
    arx_renderer* r = c.r;
    arx_status st;
    if ((st = warm_up(c)) != ARX_OK) return st;
    bool batch = false;
    if ((st = prepare_batch(c, &batch)) != ARX_OK) return st;
    if (batch) select_batched(c);
    // 3. the poses that take the one-listener route, each ending synchronised
    for (size_t j = 0; j < c.n; ++j)
        if (c.route[j] == ARX_LISTENER_SINGLE && (st = render_single(c, j)) != ARX_OK) return st;
    if (!c.batched.empty()) {
        // 4. the bands' base counts, once; then the chunks
        if (c.filters)
            ARX_HIP(hipMemcpyAsync(r->listener_bands.d_filters, c.filters, (size_t)c.B * (size_t)c.taps * sizeof(double),
                                   hipMemcpyDefault, r->stream));
        FilterArgs fa;
        fa.planes = c.probe.planes;
        fa.list = nullptr;
        fa.heads = nullptr;
        fa.grow = c.fgrow;
        ARX_HIP(launch_band_base(c.probe.args, fa, band_args(c), c.d_base + c.sc.counts, r->stream));
        for (size_t c0 = 0; c0 < c.batched.size(); c0 += (size_t)c.chunk) {
            const int32_t J = (int32_t)std::min<size_t>((size_t)c.chunk, c.batched.size() - c0);
            if ((st = issue_chunk(c, c0, J)) != ARX_OK) return st;
        }
    }
    // 5. the one synchronisation of the batched route, then the host-side outputs
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (!c.batched.empty() && c.pin.flag[1] != 0 && c.pin.flag[0] == c.pin.flag[1])
        return fail(ARX_ERR_INTERNAL, "receiver refit / re-quantization: a box left the quantization grid");
    write_outputs(c);
    return ARX_OK;
}

}  // namespace

void arx::free_listener_bands(ListenerBandBatch& b) {
    hipFree(b.d_scratch);
    hipFree(b.d_filters);
    if (b.h_pinned) hipHostFree(b.h_pinned);
    if (b.ev0) hipEventDestroy(b.ev0);
    if (b.ev1) hipEventDestroy(b.ev1);
    b = ListenerBandBatch{};
}

extern "C" {

arx_status arx_render_listener_bands(arx_renderer* r, const arx_listener_pose* poses, size_t n, float* ir_left, float* ir_right,
                                     const double* filters, int32_t taps, float* bb_left, float* bb_right,
                                     arx_acoustics* acoustics, arx_listener_band_result* results, double* ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n == 0) return ARX_OK;
    if (!poses) return fail(ARX_ERR_INVALID_ARGUMENT, "poses is NULL");
    if ((ir_left == nullptr) != (ir_right == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ir_left and ir_right: both or neither");
    if ((bb_left == nullptr) != (bb_right == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "bb_left and bb_right: both or neither");
    if ((filters == nullptr) != (bb_left == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "filters and bb_left / bb_right: all or none");
    if (filters && arx_debug_combine_bytes(1, 1, taps) == 0)
        return fail(ARX_ERR_INVALID_ARGUMENT, "taps %d: odd, 1..%d", taps, ARX_BAND_TAPS_MAX);
    for (size_t j = 0; j < n; ++j)
        if (!std::isfinite(poses[j].x) || !std::isfinite(poses[j].y) || !std::isfinite(poses[j].z) ||
            !std::isfinite(poses[j].yaw_deg))
            return fail(ARX_ERR_INVALID_ARGUMENT, "pose %zu is not finite", j);
    if (r->fif != 1) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs one frame in flight");
    if (r->stream != r->cur().stream) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own stream");
    if (r->d_hist_ext) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own histogram");
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    if (r->bands.n_bands < 1) return fail(ARX_ERR_NOT_READY, "arx_set_band_absorption has not been called for this scene");
    if (r->path_cache.mode != 1) return fail(ARX_ERR_NOT_READY, "a band render replays the path cache, which is off");
    Call c{r, poses, n, ir_left, ir_right, filters, filters ? taps : 0, bb_left, bb_right, acoustics, results};
    c.B = r->bands.n_bands;
    c.N = n_rays(r->cfg);
    if (c.N == 0) return fail(ARX_ERR_NOT_READY, "a launch of no rays is not cacheable");
    c.ir_len = (size_t)r->ir_len;
    ARX_HIP(hipSetDevice(r->cfg.device));
    ListenerBandBatch& lb = r->listener_bands;
    const size_t pin_need = pinned_bytes(n, c.B);
    if (pin_need > lb.h_bytes) {  // nothing of an earlier call is in flight: every call ends synchronised
        if (lb.h_pinned) hipHostFree(lb.h_pinned);
        lb.h_pinned = nullptr;
        lb.h_bytes = 0;
        ARX_HIP(hipHostMalloc(&lb.h_pinned, pin_need, hipHostMallocDefault));
        lb.h_bytes = pin_need;
    }
    if (filters) {
        const uint64_t need = (uint64_t)c.B * (uint64_t)taps * sizeof(double);
        if (need > lb.filters_cap)
            if (const arx_status st = grow_device(&lb.d_filters, &lb.filters_cap, need, 0, 1); st != ARX_OK) return st;
    }
    c.pin = pinned(lb.h_pinned, n, c.B);
    c.pin.flag[0] = c.pin.flag[1] = 0u;
    c.route.assign(n, ARX_LISTENER_SINGLE);
    c.single.assign(n * (size_t)c.B, arx_band_result{});
    const bool timed = ms != nullptr;  // around the whole call, its warm launches included
    if (timed) {
        if (!lb.ev0) ARX_HIP(hipEventCreate(&lb.ev0));
        if (!lb.ev1) ARX_HIP(hipEventCreate(&lb.ev1));
        ARX_HIP(hipEventRecord(lb.ev0, r->stream));
    }
    const float saved[4] = {r->center[0], r->center[1], r->center[2], r->yaw};
    const arx_status st = render_listener_bands(c);
    arx_set_listener(r, saved[0], saved[1], saved[2], saved[3]);  // the listener set before the call, refit by the next frame
    if (st != ARX_OK) return st;
    if (timed) {
        ARX_HIP(hipEventRecord(lb.ev1, r->stream));
        ARX_HIP(hipEventSynchronize(lb.ev1));
        float t = 0.0f;
        ARX_HIP(hipEventElapsedTime(&t, lb.ev0, lb.ev1));
        *ms = (double)t;
    }
    return ARX_OK;
}

uint64_t arx_debug_listener_band_bytes(uint64_t n_rays, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t n_bands,
                                       int32_t listeners) {
    if (ir_len < 0 || recv_nodes < 0 || recv_tris < 0 || listeners < 0 || n_bands < 1 || n_bands > kMaxBands) return 0;
    return (uint64_t)listeners * bytes_each(n_rays, ir_len, recv_nodes, recv_tris, n_bands) + bytes_fixed(n_rays);
}

}  // extern "C"
