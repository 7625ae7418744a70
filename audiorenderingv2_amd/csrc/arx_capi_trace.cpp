// arx_capi_trace.cpp -- one frame behind the C ABI (include/arx.h): the trace launch (trace_rays: its
// arguments, scratch, ray order and the path cache's decision, then the launches), the histogram's clear,
// the IR's finalize and its room-acoustic analysis, and the arx_debug_* entry points of the trace and the
// ray order.  The tree the launch reads is arx_capi_device_scene.cpp's, the cache's launches
// arx_capi_path_cache.cpp's.
//
// Host-side counterpart of R/prebuild/obj_raytracer/AudioRenderer.cpp (render), re-designed for HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "arx_internal.hpp"

using namespace arx;

#ifndef ARX_TRACE_PROF
#define ARX_TRACE_PROF 0  // measurement builds only (build.py --exp TAG -D ARX_TRACE_PROF=1)
#endif
#ifndef ARX_SHARED_GRID_PCT
#define ARX_SHARED_GRID_PCT 50  // design experiments only (build.py --exp): other shares
#endif

float arx::initial_energy(const arx_config& c) {
    // devicePrograms.cu:208 -- (x*y*z) is an int product in the reference
    const int32_t n = c.rays_x * c.rays_y * c.rays_z;
    return (float)((double)c.base_power / ((double)n * 4.18879020478));
}

double arx::ir_unit(const arx_config& c) { return std::ldexp((double)initial_energy(c), -arx_frac_bits(n_rays(c))); }

AcousticsArgs arx::acoustics_args(const arx_renderer* r, const long long* hist, long long* edc, arx_acoustics* out,
                                  void* scratch) {
    AcousticsArgs args{};
    args.hist = hist;
    args.n = r->ir_len;
    args.sample_rate = r->cfg.sample_rate;
    args.unit = ir_unit(r->cfg);
    args.edc = edc;
    args.out = out;
    args.scratch = scratch;
    args.shape = r->scan_shape == 0 ? kScanDefault : r->scan_shape;
    return args;
}

namespace {

// 1. the launch's arguments, all but its scratch (directions, costs, global stack)
TraceArgs make_trace_args(arx_renderer* r, uint64_t ray_begin, uint64_t ray_end, bool clear) {
    const arx_renderer::FrameSet& f = r->cur();
    const arx_config& c = r->cfg;
    TraceArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cnodes = r->d_cnodes.p;
    // quantized nodes only while the emitter (the one ray origin off the geometry) is on the
    // grid: the slab arithmetic's error bound assumes origins within the grid's extent
    const float* em = r->emitter;
    a.qnodes = (r->q_valid && !r->force_f32_nodes && qgrid_contains(r->qgrid, em, em)) ? r->d_qnodes.p : nullptr;
    // the CW4 tree on the same condition when asked for (arx_debug_set_trace_path bit 3; measured
    // 1.9x slower than the BVH2 on C3: DESIGN.md section 6.3)
    a.wbuf = (a.qnodes && r->use_w4 && !r->force_global_stack) ? r->d_wbuf.p : nullptr;
    a.qgrid = r->qgrid;
    a.tris = r->d_tris.p;
    a.hist = r->hist();
    a.counters = f.d_counters.p;
    a.cursor = f.d_counters.p + kCursor;
    a.seed = c.seed;
    a.ray_begin = ray_begin;
    a.ray_end = ray_end;
    for (int k = 0; k < 3; ++k) {
        a.emitter[k] = r->emitter[k];
        a.center[k] = r->center[k];
    }
    a.e0 = initial_energy(c);
    a.inv_unit = (a.e0 != 0.0f) ? std::ldexp(1.0, arx_frac_bits(n_rays(c))) / (double)a.e0 : 0.0;
    a.energy_thres = c.energy_thres;
    a.hrtf = c.hrtf_absorption_rate;
    int32_t secs = r->ir_len / c.sample_rate;  // devicePrograms.cu:227-228
    secs = std::max(1, std::min(secs, 999));
    a.dist_limit = (float)(secs * kSpeedOfSound + 1);
    a.max_bounces = c.max_bounces;
    a.sample_rate = c.sample_rate;
    a.ir_len = r->ir_len;
    a.delay = (int32_t)((double)c.sample_rate * 0.00044);  // devicePrograms.cu:125
    a.is_mono = c.is_mono;
    a.bvh_depth = r->stats.bvh_depth;
    if (clear) {
        a.clear_bins = 2 * (uint64_t)r->ir_len;
        a.clear_counters = kCounters;
    }
    return a;
}

// 2. the launch's scratch: the frame set's direction buffer, and for trees deeper than the LDS stack (and
// the CW4 tree) the renderer's global stack; *gstack: the launch takes it for a deep tree.
arx_status reserve_launch_scratch(arx_renderer* r, TraceArgs& a, uint64_t n_launch, bool* gstack) {
    arx_renderer::FrameSet& f = r->cur();
    if (n_launch > f.d_dirs.cap) {  // direction pre-pass buffer; what the old one held is forgotten
        f.dirs_valid = f.dirs_sorted = false;
        if (const arx_status st = f.d_dirs.reserve(n_launch); st != ARX_OK) return st;
    }
    *gstack = r->force_global_stack || a.bvh_depth + 1 > kLdsStack;
    // CW4: up to three pushes per level; the rows beyond the LDS rows overflow into a global column
    const size_t w4_rows = (size_t)std::max(1, 3 * r->depth4 + 3 - kLdsStack);
    if (*gstack || a.wbuf) {  // one global column of bvh_depth + 1 entries per lane
        const size_t lanes = trace_max_lanes(r->cus);
        const size_t need = (a.wbuf ? w4_rows : (size_t)(a.bvh_depth + 1)) * lanes;
        if (const arx_status st = r->d_gstack.reserve(need); st != ARX_OK) return st;
        a.gstack = r->d_gstack.p;
        a.gstack_lanes = lanes;
        // one global stack per renderer: with frames in flight, after the other frames' traces
        if (const arx_status w = fif_wait_traced(r); w != ARX_OK) return w;
    }
#if ARX_TRACE_PROF  // measurement builds only: per-wave records (arx_debug_trace_profile)
    {
        const size_t words = (size_t)r->cus * 64 * kProfWords;  // >= waves of any trace grid
        if (const arx_status st = r->d_prof.reserve(words); st != ARX_OK) return st;
        ARX_HIP(hipMemsetAsync(r->d_prof.p, 0, words * sizeof(unsigned long long), r->stream));
        a.prof = r->d_prof.p;
    }
#endif
    return ARX_OK;
}

// The launch's key, for the ray order as it is and for the path cache without dyn_share and instance.
OrderKey make_order_key(const arx_renderer* r, const TraceArgs& a, int fmt) {
    OrderKey key;
    std::memset(&key, 0, sizeof(key));
    key.scene_gen = r->scene_gen;
    key.tree_hash = r->stats.tree_hash;
    key.seed = a.seed;
    key.ray_begin = a.ray_begin;
    key.ray_end = a.ray_end;
    for (int k = 0; k < 3; ++k) key.emitter[k] = r->emitter[k];
    key.e0 = a.e0;
    key.energy_thres = a.energy_thres;
    key.hrtf = a.hrtf;
    key.dist_limit = a.dist_limit;
    key.max_bounces = a.max_bounces;
    key.dyn_share = trace_pool_share();
    key.is_mono = a.is_mono;
    key.instance = fmt;
    return key;
}

// 3. the direction buffer across launches (arx_debug_set_ray_order, include/arx.h).  Kept while seed
// and ray range stay (every launch kind); for launches that take the pool on the 16-bit LDS-stack
// instance, the pool's slots ordered longest first: the first launch of a key runs the measuring
// instance on directions in ray order and the sort follows it on the same stream into the set's
// second buffer; the launches after it run the product instance on that buffer as long as the key
// holds.  Per frame set: its own stream and buffers, nothing new crosses streams.
struct RayOrder {
    bool use_sorted;  // the launch runs on the sorted buffer as it is
    bool measure;     // the launch measures the rays' costs and the sort follows it
    bool fill_dirs;   // the launch's pre-pass writes the directions
};
arx_status plan_ray_order(arx_renderer* r, const TraceArgs& a, const OrderKey& key, uint64_t n_launch, RayOrder* o) {
    arx_renderer::FrameSet& f = r->cur();
    // (a caller's other stream, arx_set_stream, is not ordered after the launch that wrote them: re-made)
    const bool kept = r->ray_order != 2 && f.dirs_valid && f.dirs_stream == r->stream && f.dirs_seed == a.seed &&
                      f.dirs_begin == a.ray_begin && f.dirs_count == n_launch;
    const bool ordered = r->ray_order == 1 && trace_can_measure(a, r->cus, r->force_global_stack);
    o->use_sorted = ordered && kept && f.dirs_sorted && same_key(key, f.order_key);
    o->measure = ordered && !o->use_sorted;
    o->fill_dirs = !o->use_sorted && !(kept && !f.dirs_sorted);
    if (o->measure) {  // the two direction buffers swap: always the same size
        arx_status st;
        if ((st = f.d_order_bins.reserve(order_bins_bytes() / sizeof(uint32_t))) != ARX_OK || (st = f.d_dirs_alt.reserve(f.d_dirs.cap)) != ARX_OK ||
            (st = f.d_cost.reserve(f.d_dirs.cap)) != ARX_OK)
            return st;
    }
    return ARX_OK;
}

// 4. the path cache's decision for this launch (arx_path_plan.hpp), from the cache as the launches before
// left it; *need: bytes of the launch's records.
PathPlan plan_launch_cache(const arx_renderer* r, const TraceArgs& a, OrderKey key, const RayOrder& o, uint64_t* need) {
    const PathCache& pc = r->path_cache;
    const bool cacheable = pc.mode == 1 && r->stream == r->cur().stream && trace_can_cache(a, r->force_global_stack);
    key.dyn_share = 0;  // the cache carries its own directions: neither shapes a ray's path
    key.instance = 0;
    *need = arx_debug_path_cache_bytes(a.ray_end - a.ray_begin, a.max_bounces);
    const PathHistory h{pc.recorded, pc.key, pc.last_valid, pc.last_key, pc.max_bytes, pc.no_room};
    return plan_path_cache(pc.mode, cacheable, key, !o.fill_dirs && !o.measure, *need, h);
}

// 5. the traced launch, and behind a measuring one the sort of its pool
arx_status issue_trace(arx_renderer* r, const TraceArgs& a, const OrderKey& key, const RayOrder& o, int grid_cus) {
    arx_renderer::FrameSet& f = r->cur();
    const uint64_t n_launch = a.ray_end - a.ray_begin;
    f.dirs_valid = false;  // until the launches below are issued
    ARX_HIP(launch_trace(a, grid_cus, r->stream, r->force_global_stack, o.fill_dirs));
    f.dirs_stream = r->stream;
    f.dirs_seed = a.seed;
    f.dirs_begin = a.ray_begin;
    f.dirs_count = n_launch;
    f.dirs_sorted = o.use_sorted;
    if (o.measure) {  // inside the launch's timing window: a cost this frame pays
        ARX_HIP(launch_order_pool(f.d_dirs.p, f.d_dirs_alt.p, f.d_cost.p, f.d_order_bins.p, n_launch, r->stream));
        std::swap(f.d_dirs, f.d_dirs_alt);
        f.order_key = key;
        f.dirs_sorted = true;
    }
    f.dirs_valid = true;
    return ARX_OK;
}

}  // namespace

arx_status arx::trace_rays(arx_renderer* r, uint64_t ray_begin, uint64_t ray_end, bool timed, bool clear,
                           ReplayProbe* probe) {
    if (probe) probe->ready = probe->recorded = false;
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (ray_end < ray_begin) return fail(ARX_ERR_INVALID_ARGUMENT, "ray_end < ray_begin");
    // global ray ids index the launch of N = x*y*z rays: energies are normalised by N and the
    // int64 fixed point's headroom (arx_frac_bits) assumes at most N rays per histogram
    if (ray_end > n_rays(r->cfg))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ray_end %llu exceeds the launch's %llu rays", (unsigned long long)ray_end,
                    (unsigned long long)n_rays(r->cfg));
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_status st = ensure_device_scene(r);
    if (st != ARX_OK) return st;
    arx_renderer::FrameSet& f = r->cur();
    TraceArgs a = make_trace_args(r, ray_begin, ray_end, clear);
    if (ray_end == ray_begin) {  // nothing to trace: the clear alone
        if (probe) return ARX_OK;
        if (clear) ARX_HIP(launch_clear(r->hist(), 2 * (uint64_t)r->ir_len, f.d_counters.p, (int)kCounters, r->stream));
        return ARX_OK;
    }
    const uint64_t n_launch = ray_end - ray_begin;
    bool gstack = false;
    if ((st = reserve_launch_scratch(r, a, n_launch, &gstack)) != ARX_OK) return st;
    // frames in flight: after the other frame set's last writes to the tree (its refit, re-gridding
    // or upload), which this launch reads
    if (const arx_status w = fif_wait_scene(r); w != ARX_OK) return w;
    const int fmt = a.wbuf ? kFmtW4 : (a.qnodes ? kFmtQ16 : kFmtF32);
    // the instance launch_trace takes (ray pool or small launch): the profile guard reads these
    const int small = trace_uses_small_block(a, r->cus, r->force_global_stack) ? 1 : 0;
    const OrderKey key = make_order_key(r, a, fmt);
    RayOrder order;
    if ((st = plan_ray_order(r, a, key, n_launch, &order)) != ARX_OK) return st;
    a.dirs = f.d_dirs.p;
    a.cost = order.measure ? f.d_cost.p : nullptr;
    const int inst = order.measure ? kInstMeasure : (small ? kInstSmall : kInstPool);
    r->stats.trace_format = fmt;
    r->stats.trace_vgprs = r->occ[fmt][inst][0];
    r->stats.trace_waves_per_simd = r->occ[fmt][inst][1];
    r->stats.trace_waves_target = r->occ[fmt][inst][2];
    if (timed && !probe && (st = r->trace_ring.begin(r->stream)) != ARX_OK) return st;
    // Frames in flight: a ray-pool launch is sized for half the CUs' wave slots, so the next frame's
    // launch runs beside it for its whole length instead of only in its tail.  A launch of 1M rays
    // gives each lane about three rays; the last of them leave the lanes idle one by one, and a wave
    // holds its slot until its last lane is done (C3 on the full grid: 5.87e9 queries/s at 1M rays
    // against 7.23e9 at 10M).  Two half grids side by side: C3 2.60 -> 2.44 ms per frame (DESIGN.md
    // section 6.3, profiles/r06/grid_ab_*.txt); more than half each makes a launch's last blocks wait
    // for the other's (55 %: 2.9 ms).  One frame in flight keeps the full grid, and so do the traces
    // on the renderer's one global stack (deep trees, CW4): they wait for every other frame's trace
    // above, so they never run beside one.
    const bool shared_grid = r->fif >= 2 && !small && !gstack && !a.wbuf;
    const int grid_cus = shared_grid ? std::max(1, r->cus * ARX_SHARED_GRID_PCT / 100) : r->cus;
    r->stats.trace_grid_cus = grid_cus;
    // The path cache (arx_debug_set_path_cache, include/arx.h).  A launch whose key equals the previous
    // launch's, on a direction buffer in its final state (one this launch would neither fill nor
    // measure), records the scene-only hits and replays them; the launches of that key after it only
    // replay.  Everything else is traced as above and costs what it did.
    PathCache& pc = r->path_cache;
    uint64_t need = 0;
    PathPlan plan = plan_launch_cache(r, a, key, order, &need);
    if (probe) {
        // a probe decides what this launch would do and leaves what the last launch did as it was, but for
        // records of another key: those are dropped now (arx_debug_path_cache_state reports 0 bytes)
        pc.recorded = plan.recorded;
        probe->recorded = plan.replay && !plan.record && pc.rec_stream == r->stream;
        probe->ready = probe->recorded && pc.filter_on && pc.has_state && pc.d_filter.p;
        probe->state = plan.state;
        probe->args = a;
        probe->args.dirs = pc.d_dirs.p;
        probe->args.rec = pc.d_hits.p;
        probe->planes = pc.d_filter.p;
        return ARX_OK;
    }
    pc.last_filtered = false;
    pc.state = plan.state;
    pc.recorded = plan.recorded;
    pc.last_valid = plan.last_valid;
    pc.last_key = plan.last_key;
    if (plan.record) {
        bool fits = true;
        if ((st = path_cache_reserve(r, n_launch, need, &fits)) != ARX_OK) return st;
        if (fits) {
            pc.key = plan.last_key;
        } else {  // no room on the device for an optional cache: this launch is traced like an over-cap one
            plan.record = plan.replay = false;
            pc.state = kPathOverCap;
            pc.no_room = need;  // not tried again per frame (arx_debug_set_path_cache forgets it)
        }
    }
    st = plan.replay ? issue_path_replay(r, a, plan.record, n_launch, grid_cus) : issue_trace(r, a, key, order, grid_cus);
    if (st != ARX_OK) return st;
    if (timed && (st = r->trace_ring.end(r->stream)) != ARX_OK) return st;
    return fif_done_traced(r);
}

extern "C" {

arx_status arx_finalize_ir(arx_renderer* r) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(launch_finalize_ir((const long long*)r->hist(), r->cur().d_ir.p, r->cur().d_ir.p + r->ir_len, r->ir_len,
                               ir_unit(r->cfg), r->cfg.is_mono, r->stream));
    r->conv_ir_dirty = true;
    r->conv_live_ir_dirty = true;
    ++r->ir_generation;
    return ARX_OK;
}

arx_status arx_analyze_ir(arx_renderer* r) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_renderer::Acoustics& a = r->cur().acou;
    if (!a.d_edc.p) {  // this frame set's first analysis
        arx_status st;
        if ((st = a.d_edc.reserve(3 * (size_t)r->ir_len)) != ARX_OK || (st = a.d_res.reserve(3)) != ARX_OK ||
            (st = a.d_scratch.reserve(acoustics_scratch_bytes())) != ARX_OK) {
            a.release();
            return st;
        }
    }
    if (r->timing)
        if (const arx_status st = r->analysis_ring.begin(r->stream); st != ARX_OK) return st;
    ARX_HIP(launch_acoustics(acoustics_args(r, (const long long*)r->hist(), a.d_edc.p, a.d_res.p, a.d_scratch.p), r->stream));
    if (r->timing)
        if (const arx_status st = r->analysis_ring.end(r->stream); st != ARX_OK) return st;
    a.queued = true;
    return ARX_OK;
}

arx_status arx_clear_histogram(arx_renderer* r) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const arx_status st = arx::begin_frame(r);
    if (st != ARX_OK) return st;
    ARX_HIP(launch_clear(r->hist(), 2 * (uint64_t)r->ir_len, r->cur().d_counters.p, (int)kCounters, r->stream));
    return ARX_OK;
}

arx_status arx_trace_rays(arx_renderer* r, uint64_t ray_begin, uint64_t ray_end) {
    return r ? arx::trace_rays(r, ray_begin, ray_end, r->timing) : fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
}


arx_status arx_render(arx_renderer* r, double* render_ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
#ifdef ARX_EXP_SEPARATE_CLEAR  // design experiments only: the clear as a launch of its own (round-5 A/B)
    arx_status st = arx_clear_histogram(r);
    if (st != ARX_OK) return st;
    st = arx::trace_rays(r, 0, n_rays(r->cfg), r->timing || render_ms != nullptr, false);
#else
    arx_status st = arx::begin_frame(r);  // the clear rides on the direction pre-pass
    if (st != ARX_OK) return st;
    st = arx::trace_rays(r, 0, n_rays(r->cfg), r->timing || render_ms != nullptr, true);
#endif
    if (st != ARX_OK) return st;
    st = arx_finalize_ir(r);
    if (st != ARX_OK) return st;
    if (r->auto_analyze && (st = arx_analyze_ir(r)) != ARX_OK) return st;
    if (render_ms) return r->trace_ring.last_ms(true, render_ms);
    return ARX_OK;
}


arx_status arx_set_auto_analyze(arx_renderer* r, int32_t on) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->auto_analyze = on != 0;
    return ARX_OK;
}

arx_status arx_debug_set_scan_shape(arx_renderer* r, int32_t shape) {
    if (!r || shape < 0 || shape > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "scan shape: 0, 1 or 2");
    r->scan_shape = shape;
    return ARX_OK;
}

arx_status arx_get_acoustics(arx_renderer* r, int32_t channel, arx_acoustics* out) {
    if (!r || !out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel < 0 || channel > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "channel %d: 0 left, 1 right, 2 sum", channel);
    if (!r->cur().acou.queued) return fail(ARX_ERR_NOT_READY, "no analysis was queued for the last frame (arx_analyze_ir)");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipMemcpyAsync(out, r->cur().acou.d_res.p + channel, sizeof(arx_acoustics), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

arx_status arx_edc_device(arx_renderer* r, int64_t** d_edc, size_t* n) {
    if (!r || !d_edc) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    *d_edc = (int64_t*)r->cur().acou.d_edc.p;
    if (n) *n = 3 * (size_t)r->ir_len;
    return ARX_OK;
}

arx_status arx_copy_edc(arx_renderer* r, int32_t channel, int64_t* h_edc, size_t ir_len) {
    if (!r || !h_edc) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel < 0 || channel > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "channel %d: 0 left, 1 right, 2 sum", channel);
    if (ir_len != (size_t)r->ir_len) return fail(ARX_ERR_INVALID_ARGUMENT, "ir_len %zu != %d", ir_len, r->ir_len);
    if (!r->cur().acou.queued) return fail(ARX_ERR_NOT_READY, "no analysis was queued for the last frame (arx_analyze_ir)");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipMemcpyAsync(h_edc, r->cur().acou.d_edc.p + (size_t)channel * ir_len, ir_len * sizeof(int64_t),
                           hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

arx_status arx_debug_trace_counters(arx_renderer* r, uint64_t* out, size_t n) {
    if (!r || !out || n > (size_t)kCounters) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    ARX_HIP(hipSetDevice(r->cfg.device));
    const arx_renderer::FrameSet& f = r->cur();
    ARX_HIP(hipMemcpyAsync(f.h_counters.p, f.d_counters.p, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    for (size_t i = 0; i < n; ++i) out[i] = f.h_counters.p[i];
    return ARX_OK;
}


arx_status arx_debug_trace_profile(arx_renderer* r, uint64_t* out, size_t n_words, size_t* n_out) {
    if (!r || (n_words > 0 && !out)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    if (!r->d_prof.p) return fail(ARX_ERR_NOT_READY, "not a profiling build (ARX_TRACE_PROF) or no trace yet");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipStreamSynchronize(r->stream));
    const size_t k = std::min<size_t>(n_words, r->d_prof.cap);
    ARX_HIP(hipMemcpy(out, r->d_prof.p, k * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (n_out) *n_out = k;
    return ARX_OK;
}


arx_status arx_debug_set_trace_path(arx_renderer* r, int path) {
    if (!r || path < 0 || path > 15 || (path & 4)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    r->force_f32_nodes = (path & 1) != 0;
    r->force_global_stack = (path & 2) != 0;
    const bool w4 = (path & 8) != 0;
    if (w4 && !r->use_w4) {  // the opt-in CW4 copy is made and uploaded at the next trace
        r->scene_dirty = true;
        r->recv_model_dirty = true;
    }
    r->use_w4 = w4;
    return ARX_OK;
}

arx_status arx_debug_set_ray_order(arx_renderer* r, int32_t mode) {
    if (!r || mode < 0 || mode > 2) return fail(ARX_ERR_INVALID_ARGUMENT, "ray order: 0, 1 or 2");
    r->ray_order = mode;
    return ARX_OK;
}


arx_status arx_debug_ray_order_buffer(arx_renderer* r, float* h_out_xyzw, uint64_t count, uint64_t* first_ray,
                                      uint64_t* n_static, int32_t* sorted) {
    if (!r || (count > 0 && !h_out_xyzw)) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    const arx_renderer::FrameSet& f = r->cur();
    if (!f.dirs_valid) return fail(ARX_ERR_NOT_READY, "no trace on this frame set yet");
    if (count > f.dirs_count) return fail(ARX_ERR_INVALID_ARGUMENT, "the buffer holds %llu rays", (unsigned long long)f.dirs_count);
    ARX_HIP(hipSetDevice(r->cfg.device));
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (count > 0) ARX_HIP(hipMemcpy(h_out_xyzw, f.d_dirs.p, count * 16, hipMemcpyDeviceToHost));
    if (first_ray) *first_ray = f.dirs_begin;
    if (n_static) *n_static = f.dirs_sorted ? pool_static_rays(f.dirs_count, trace_pool_share()) : f.dirs_count;
    if (sorted) *sorted = f.dirs_sorted ? 1 : 0;
    return ARX_OK;
}

arx_status arx_debug_ray_order_host(uint64_t n, uint32_t dyn_share, uint32_t steps, uint64_t* n_static, uint32_t* cost16,
                                    uint32_t* build_share) {
    if (n_static) *n_static = pool_static_rays(n, dyn_share);
    if (cost16) *cost16 = ray_cost16(steps);
    if (build_share) *build_share = trace_pool_share();
    return ARX_OK;
}

arx_status arx_debug_ray_directions(uint64_t seed, uint64_t first, uint64_t count, float* h_out, int device) {
    if (count > 0 && !h_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL output");
    if (count == 0) return ARX_OK;
    ARX_HIP(hipSetDevice(device));
    float* d = nullptr;
    ARX_HIP(hipMalloc(&d, 3 * count * sizeof(float)));
    hipError_t e = launch_ray_directions(seed, first, count, d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h_out, d, 3 * count * sizeof(float), hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail(ARX_ERR_HIP, "ray directions: %s", hipGetErrorString(e));
    return ARX_OK;
}

}  // extern "C"
