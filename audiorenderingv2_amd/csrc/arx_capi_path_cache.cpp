// arx_capi_path_cache.cpp -- the path cache and its filter behind the C ABI (include/arx.h): their device
// buffers, and the launches of a frame the cache serves -- record, replay and filtered replay
// (arx_replay.hip) -- with the arx_debug_* entry points of both.  Which of them a launch takes is decided
// in arx_path_plan.hpp; trace_rays (arx_capi_trace.cpp) asks it and calls issue_path_replay.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

static_assert(kPathFrames == arx_renderer::kMaxFrames, "one last-replay event per frame set");

namespace {

// The path filter's planes for a recording of n rays (outside the cap, optional).  False: no room on the
// device (the error cleared; that size is not tried again), and the launch records and replays
// unfiltered.  Called behind path_cache_reserve: a buffer that must grow is freed with every stream idle.
bool path_filter_reserve(arx_renderer* r, uint64_t n, uint32_t max_bounces) {
    PathCache& pc = r->path_cache;
    const uint64_t need = path_filter_plane_bytes(n, max_bounces);
    if (need <= pc.d_filter.cap) return true;
    if (known_no_room(pc.filter_no_room, need) || sync_renderer(r) != ARX_OK) return false;
    return pc.d_filter.try_reserve(need, &pc.filter_no_room);
}

}  // namespace

arx_status arx::path_cache_reserve(arx_renderer* r, uint64_t n, uint64_t need, bool* fits) {
    PathCache& pc = r->path_cache;
    *fits = true;
    if (!pc.ev_recorded) ARX_HIP(hipEventCreateWithFlags(&pc.ev_recorded, hipEventDisableTiming));
    for (hipEvent_t& e : pc.ev_replayed)
        if (!e) ARX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    arx_status st;
    if ((st = pc.d_scratch.reserve(kCursor + 1)) != ARX_OK || (st = pc.h_scratch.reserve(kCounters)) != ARX_OK) return st;
    if (n <= pc.d_dirs.cap && need <= pc.d_hits.cap) return ARX_OK;
    if ((st = sync_renderer(r)) != ARX_OK) return st;
    // the caller marks the records' size as not fitting (PathCache::no_room), whichever buffer it was
    *fits = pc.d_dirs.try_reserve(n, &pc.no_room) && pc.d_hits.try_reserve(need, &pc.no_room);
    return ARX_OK;
}

bool arx::path_filter_list_reserve(arx_renderer* r, uint64_t n) {
    PathCache& pc = r->path_cache;
    arx_renderer::FrameSet& f = r->cur();
    if (n <= f.filter_list_rays) return true;
    const uint64_t need = path_filter_list_bytes(n);
    if (known_no_room(pc.filter_list_no_room, need)) return false;
    // an earlier replay on this set's stream may still write it
    if (f.d_filter_list.p && hipStreamSynchronize(f.stream) != hipSuccess) return false;
    f.filter_list_rays = f.d_filter_list.try_reserve(need, &pc.filter_list_no_room) ? n : 0;
    return f.filter_list_rays > 0;
}

float arx::path_filter_grow(const QGrid& g) {
    float m = 0.0f;
    for (int k = 0; k < 3; ++k)
        m = std::max(m, std::max(std::fabs(g.origin[k]), std::fabs(g.origin[k] + 65536.0f * g.scale[k])));
    return kFilterMargin + std::ldexp(m, -18);
}

namespace {

// The recording: the scene-only hits of every query of the launch into the cache, on a copy of the
// launch's direction buffer; with the filter on, what every query starts from as well (outside the cap;
// without room for it, records alone).
arx_status issue_path_record(arx_renderer* r, const TraceArgs& pa, uint64_t n_launch, int grid_cus) {
    PathCache& pc = r->path_cache;
    // the cache may still be read by the other sets' replays of the key before
    for (int k = 0; k < r->fif; ++k)
        if (pc.replayed[k] && k != r->slot) ARX_HIP(hipStreamWaitEvent(r->stream, pc.ev_replayed[k], 0));
    for (bool& b : pc.replayed) b = false;
    ARX_HIP(hipMemcpyAsync(pc.d_dirs.p, r->cur().d_dirs.p, n_launch * 16, hipMemcpyDeviceToDevice, r->stream));
    TraceArgs ra = pa;
    ra.hist = nullptr;
    ra.counters = pc.d_scratch.p;
    ra.cursor = pc.d_scratch.p + kCursor;
    ra.clear_bins = 0;
    ra.clear_counters = kCounters;
    pc.has_state = pc.filter_on && pa.max_bounces >= 1 && pa.max_bounces <= kFilterMaxBounces &&
                   path_filter_reserve(r, n_launch, pa.max_bounces);
    ra.gstack = pc.has_state ? reinterpret_cast<int32_t*>(pc.d_filter.p) : nullptr;
    ARX_HIP(launch_path_record(ra, grid_cus, r->stream));
    pc.recorded = true;
    pc.bytes = kPathRecordBytes * (uint64_t)pa.max_bounces * n_launch;
    pc.rec_rays = n_launch;
    ++pc.rec_gen;
    pc.rec_stream = r->stream;
    ARX_HIP(hipEventRecord(pc.ev_recorded, r->stream));
    return ARX_OK;
}

}  // namespace

arx_status arx::issue_path_replay(arx_renderer* r, const TraceArgs& a, bool record, uint64_t n_launch, int grid_cus) {
    PathCache& pc = r->path_cache;
    arx_renderer::FrameSet& f = r->cur();
    TraceArgs pa = a;
    pa.dirs = pc.d_dirs.p;
    pa.rec = pc.d_hits.p;
    if (record) {
        if (const arx_status st = issue_path_record(r, pa, n_launch, grid_cus); st != ARX_OK) return st;
    } else if (pc.rec_stream != r->stream) {
        ARX_HIP(hipStreamWaitEvent(r->stream, pc.ev_recorded, 0));
    }
    // Filtered unless the emitter lies inside the receiver's grown box: every ray would be a
    // candidate at bounce 0, and the frame takes the unfiltered kernel, which costs what it did.
    const bool filtered = pc.filter_on && pc.has_state &&
                          !emitter_in_receiver_box(r, r->center, 2.0f * path_filter_grow(a.qgrid)) &&
                          path_filter_list_reserve(r, n_launch);
    if (filtered) {
        FilterArgs fa;
        fa.planes = pc.d_filter.p;
        fa.list = reinterpret_cast<FilterCand*>(f.d_filter_list.p);
        fa.heads = fa.list + f.filter_list_rays;
        fa.grow = path_filter_grow(a.qgrid);
        ARX_HIP(launch_path_replay_filtered(pa, fa, r->stream));
        pc.last_filtered = true;
        pc.filter_slot = r->slot;
        pc.filter_rays = n_launch;
    } else {
        ARX_HIP(launch_path_replay(pa, r->stream));
    }
    if (r->fif > 1) {
        ARX_HIP(hipEventRecord(pc.ev_replayed[r->slot], r->stream));
        pc.replayed[r->slot] = true;
    }
    pc.state = record ? kPathRecorded : kPathReplayed;
    return ARX_OK;
}

extern "C" {

arx_status arx_debug_set_path_cache(arx_renderer* r, int32_t mode, uint64_t max_bytes) {
    if (!r || mode < 0 || mode > 1) return fail(ARX_ERR_INVALID_ARGUMENT, "path cache: mode 0 or 1");
    PathCache& pc = r->path_cache;
    pc.mode = mode;
    pc.max_bytes = max_bytes;
    pc.recorded = pc.last_valid = false;  // the next launch is traced
    pc.no_room = 0;
    pc.state = mode == 1 ? kPathTraced : kPathOff;
    return ARX_OK;
}

arx_status arx_debug_path_cache_state(arx_renderer* r, int32_t* state, uint64_t* bytes, uint64_t* queries_recorded) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const PathCache& pc = r->path_cache;
    if (state) *state = pc.state;
    if (bytes) *bytes = pc.recorded ? pc.bytes : 0;
    if (queries_recorded) {
        *queries_recorded = 0;
        if (pc.recorded) {  // the recording's own query counter (its scratch block)
            ARX_HIP(hipSetDevice(r->cfg.device));
            ARX_HIP(hipMemcpyAsync(pc.h_scratch.p, pc.d_scratch.p, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   pc.rec_stream));
            ARX_HIP(hipStreamSynchronize(pc.rec_stream));
            *queries_recorded = pc.h_scratch.p[0];
        }
    }
    return ARX_OK;
}

arx_status arx_debug_set_path_filter(arx_renderer* r, int32_t on) {
    if (!r || on < 0 || on > 1) return fail(ARX_ERR_INVALID_ARGUMENT, "path filter: 0 or 1");
    PathCache& pc = r->path_cache;
    // switched on over records that came without state: they are forgotten, so the key's next launch
    // records again, once, with it
    if (on && !pc.filter_on && pc.recorded && !pc.has_state) pc.recorded = false;
    if (on && !pc.filter_on) pc.filter_no_room = pc.filter_list_no_room = 0;
    pc.filter_on = on;
    return ARX_OK;
}

arx_status arx_debug_path_filter_state(arx_renderer* r, int32_t* filtered, uint64_t* bytes, uint64_t* candidate_rays,
                                       uint64_t* candidate_queries) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const PathCache& pc = r->path_cache;
    if (filtered) *filtered = pc.last_filtered ? 1 : 0;
    if (bytes) {
        *bytes = pc.d_filter.bytes();
        for (const arx_renderer::FrameSet& f : r->sets)
            *bytes += f.d_filter_list.bytes();
    }
    if (candidate_rays) *candidate_rays = 0;
    if (candidate_queries) *candidate_queries = 0;
    const arx_renderer::FrameSet& f = r->sets[pc.filter_slot];
    if ((candidate_rays || candidate_queries) && pc.last_filtered && f.d_filter_list.p) {
        // the heads the launch's filter blocks left behind the list: {candidate rays, candidate queries, ...}
        std::vector<uint32_t> h(4 * path_filter_heads(pc.filter_rays));
        ARX_HIP(hipSetDevice(r->cfg.device));
        ARX_HIP(hipStreamSynchronize(f.stream));
        ARX_HIP(hipMemcpy(h.data(), reinterpret_cast<const FilterCand*>(f.d_filter_list.p) + f.filter_list_rays,
                          h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t rays = 0, queries = 0;
        for (size_t k = 0; k < h.size(); k += 4) {
            rays += h[k];
            queries += h[k + 1];
        }
        if (candidate_rays) *candidate_rays = rays;
        if (candidate_queries) *candidate_queries = queries;
    }
    return ARX_OK;
}

uint64_t arx_debug_path_filter_bytes(uint64_t n_rays, uint32_t max_bounces, uint32_t n_lists) {
    return path_filter_plane_bytes(n_rays, max_bounces) + (uint64_t)n_lists * path_filter_list_bytes(n_rays);
}

uint64_t arx_debug_path_cache_bytes(uint64_t n_rays, uint32_t max_bounces) {
    return kPathRecordBytes * n_rays * (uint64_t)max_bounces;
}

}  // extern "C"
