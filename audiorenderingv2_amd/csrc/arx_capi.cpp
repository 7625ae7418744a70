// arx_capi.cpp -- C ABI of libarx.so (include/arx.h): the renderer itself -- the error channel,
// its lifecycle, the frame sets of frames in flight, the timing rings, the simple setters and
// getters and the device helpers.  The scene image is in arx_scene.cpp, the tree on the device in
// arx_capi_device_scene.cpp, a frame in arx_capi_trace.cpp, the path cache in arx_capi_path_cache.cpp, a
// batch of listeners in arx_capi_listeners.cpp, the convolution in arx_capi_conv.cpp.
//
// Host-side counterpart of R/prebuild/obj_raytracer/AudioRenderer.cpp, re-designed for HIP: one
// stream per frame set, persistent device buffers (the reference cudaMallocs and frees inside every
// call, AudioRenderer.cpp:593-750), status codes instead of throw/exit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "arx_internal.hpp"

using namespace arx;

namespace {
thread_local std::string g_last_error;

// The per-launch timing events only time: no system-scope fence when they are recorded (with one,
// each marker wrote back and invalidated the caches, a few microseconds of stream time per event).
constexpr unsigned kTimingEvent = hipEventDisableSystemFence;
}  // namespace

arx_status arx::fail(arx_status s, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return s;
}

// shared with arx_io.cpp so the loaders report through arx_last_error()
void arx_set_last_error(const std::string& m) { g_last_error = m; }

arx_status EventRing::create_all() {
    for (int i = 0; i < kTraceRing; ++i) {
        ARX_HIP(hipEventCreateWithFlags(&e0[i], kTimingEvent));
        ARX_HIP(hipEventCreateWithFlags(&e1[i], kTimingEvent));
    }
    return ARX_OK;
}

void EventRing::destroy() {
    for (int i = 0; i < kTraceRing; ++i) {
        if (e0[i]) hipEventDestroy(e0[i]);
        if (e1[i]) hipEventDestroy(e1[i]);
    }
    *this = EventRing{};
}

arx_status EventRing::begin(hipStream_t s) {
    const int slot = (int)(launches % kTraceRing);
    if (!e0[slot]) ARX_HIP(hipEventCreateWithFlags(&e0[slot], kTimingEvent));
    if (!e1[slot]) ARX_HIP(hipEventCreateWithFlags(&e1[slot], kTimingEvent));
    ARX_HIP(hipEventRecord(e0[slot], s));
    return ARX_OK;
}

arx_status EventRing::end(hipStream_t s) {
    ARX_HIP(hipEventRecord(e1[(int)(launches % kTraceRing)], s));
    ++launches;
    return ARX_OK;
}

arx_status EventRing::last_ms(bool wait, double* ms) const {
    if (launches == 0) return fail(ARX_ERR_NOT_READY, "no timed launch yet");
    const int slot = (int)((launches - 1) % kTraceRing);
    if (wait) ARX_HIP(hipEventSynchronize(e1[slot]));
    float f = 0.f;
    ARX_HIP(hipEventElapsedTime(&f, e0[slot], e1[slot]));
    *ms = f;
    return ARX_OK;
}

arx_status EventRing::times(double* ms, size_t n, size_t* n_out) const {
    const uint64_t have = std::min<uint64_t>(launches, (uint64_t)kTraceRing);
    const uint64_t k = std::min<uint64_t>(have, (uint64_t)n);
    for (uint64_t i = 0; i < k; ++i) {  // oldest of the last k first
        const int slot = (int)((launches - k + i) % kTraceRing);
        ARX_HIP(hipEventSynchronize(e1[slot]));
        float f = 0.f;
        ARX_HIP(hipEventElapsedTime(&f, e0[slot], e1[slot]));
        ms[i] = f;
    }
    if (n_out) *n_out = (size_t)k;
    return ARX_OK;
}

namespace {

arx_status check_config(const arx_config* c) {
    if (!c) return fail(ARX_ERR_INVALID_ARGUMENT, "config is NULL");
    if (c->rays_x <= 0 || c->rays_y <= 0 || c->rays_z <= 0)
        return fail(ARX_ERR_INVALID_ARGUMENT, "rays dims must be positive");
    if ((uint64_t)c->rays_x * (uint64_t)c->rays_y * (uint64_t)c->rays_z > 0x7fffffffull)
        return fail(ARX_ERR_INVALID_ARGUMENT, "x*y*z must fit int32 (devicePrograms.cu:208 int product)");
    if (c->sample_rate <= 0) return fail(ARX_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
    if (!(c->hrtf_absorption_rate >= 0.0f && c->hrtf_absorption_rate <= 1.0f))
        return fail(ARX_ERR_INVALID_ARGUMENT, "hrtf_absorption_rate must be in [0, 1]");
    if (c->ir_length_in_seconds == 0) return fail(ARX_ERR_INVALID_ARGUMENT, "ir_length_in_seconds must be >= 1");
    const uint64_t L = (uint64_t)c->ir_length_in_seconds * (uint64_t)c->sample_rate;
    if (L > 0x7fffffffull) return fail(ARX_ERR_INVALID_ARGUMENT, "ir length too large");
    return ARX_OK;
}

// Frames in flight (no-ops with one): the current set's stream waits for every other set's last
// trace / for the set that did the last step of a chain (convolutions, all-reduces, scene writes),
// and records its own.
using FifEvents = hipEvent_t[arx_renderer::kMaxFrames];
arx_status fif_wait_all(arx_renderer* r, FifEvents& ev) {
    if (r->fif > 1)
        for (int s = 0; s < r->fif; ++s)
            if (s != r->slot) ARX_HIP(hipStreamWaitEvent(r->stream, ev[s], 0));
    return ARX_OK;
}
arx_status fif_done_one(arx_renderer* r, FifEvents& ev) {
    if (r->fif > 1) ARX_HIP(hipEventRecord(ev[r->slot], r->stream));
    return ARX_OK;
}
arx_status fif_wait_last(arx_renderer* r, FifEvents& ev, int32_t last) {
    if (r->fif > 1 && last >= 0 && last != r->slot) ARX_HIP(hipStreamWaitEvent(r->stream, ev[last], 0));
    return ARX_OK;
}
arx_status fif_done_last(arx_renderer* r, FifEvents& ev, int32_t& last) {
    if (r->fif > 1) {
        ARX_HIP(hipEventRecord(ev[r->slot], r->stream));
        last = r->slot;
    }
    return ARX_OK;
}

// A frame set's stream and buffers, zeroed (the analysis buffers come with the set's first analysis).
// On a failure the caller releases what was made.
arx_status alloc_frame_set(int32_t ir_len, arx_renderer::FrameSet& f) {
    const size_t bins = 2 * (size_t)ir_len, words = kCursor + 1;
    arx_status st;
    ARX_HIP(hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
    if ((st = f.d_hist.reserve(bins)) != ARX_OK || (st = f.d_ir.reserve(bins)) != ARX_OK ||
        (st = f.d_counters.reserve(words)) != ARX_OK || (st = f.h_counters.reserve(kCounters)) != ARX_OK)
        return st;
    ARX_HIP(hipMemsetAsync(f.d_hist.p, 0, f.d_hist.bytes(), f.stream));
    ARX_HIP(hipMemsetAsync(f.d_ir.p, 0, f.d_ir.bytes(), f.stream));
    ARX_HIP(hipMemsetAsync(f.d_counters.p, 0, f.d_counters.bytes(), f.stream));
    ARX_HIP(hipStreamSynchronize(f.stream));
    return ARX_OK;
}

arx_status ring_times(arx_renderer* r, const EventRing& ring, double* ms, size_t n, size_t* n_out) {
    if (n > 0 && !ms) return fail(ARX_ERR_INVALID_ARGUMENT, "bad arguments");
    ARX_HIP(hipSetDevice(r->cfg.device));
    return ring.times(ms, n, n_out);
}

}  // namespace

arx_status arx::fif_wait_traced(arx_renderer* r) { return fif_wait_all(r, r->ev_traced); }
arx_status arx::fif_done_traced(arx_renderer* r) { return fif_done_one(r, r->ev_traced); }
arx_status arx::fif_wait_scene(arx_renderer* r) { return fif_wait_last(r, r->ev_scene, r->last_scene); }
arx_status arx::fif_done_scene(arx_renderer* r) { return fif_done_last(r, r->ev_scene, r->last_scene); }
arx_status arx::fif_wait_conv(arx_renderer* r) { return fif_wait_last(r, r->ev_conv, r->last_conv); }
arx_status arx::fif_done_conv(arx_renderer* r) { return fif_done_last(r, r->ev_conv, r->last_conv); }
arx_status arx::fif_wait_reduced(arx_renderer* r) { return fif_wait_last(r, r->ev_reduced, r->last_reduced); }
arx_status arx::fif_done_reduced(arx_renderer* r) { return fif_done_last(r, r->ev_reduced, r->last_reduced); }

arx_status arx::sync_renderer(arx_renderer* r) {
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (r->stream && r->stream != r->cur().stream) ARX_HIP(hipStreamSynchronize(r->stream));  // arx_set_stream's
    for (const auto& f : r->sets)
        if (f.stream) ARX_HIP(hipStreamSynchronize(f.stream));
    return ARX_OK;
}

arx_status arx::begin_frame(arx_renderer* r) {
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (r->fif > 1) {  // a frame starts: it takes the next set (with one, arx_set_stream's stream stays)
        r->slot = (r->slot + 1) % r->fif;
        r->stream = r->cur().stream;
    }
    r->cur().acou.queued = false;  // the new frame has no analysis yet
    return ARX_OK;
}

extern "C" {

arx_status arx_trace_times(arx_renderer* r, double* ms, size_t n, size_t* n_out) {
    return r ? ring_times(r, r->trace_ring, ms, n, n_out) : fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
}

arx_status arx_conv_times(arx_renderer* r, double* ms, size_t n, size_t* n_out) {
    return r ? ring_times(r, r->conv_ring, ms, n, n_out) : fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
}

arx_status arx_live_times(arx_renderer* r, double* ms, size_t n, size_t* n_out) {
    return r ? ring_times(r, r->live_ring, ms, n, n_out) : fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
}

arx_status arx_analysis_times(arx_renderer* r, double* ms, size_t n, size_t* n_out) {
    return r ? ring_times(r, r->analysis_ring, ms, n, n_out) : fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
}

int32_t arx_timing_ring(void) { return kTraceRing; }
uint64_t arx_trace_kernel_id(void) { return trace_kernel_source_id(); }
uint64_t arx_conv_kernel_id(void) { return conv_kernel_source_id(); }

int32_t arx_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? (int32_t)n : -1;
}

arx_status arx_device_alloc(int32_t device, size_t bytes, void** out) {
    if (!out) return fail(ARX_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    ARX_HIP(hipSetDevice(device));
    ARX_HIP(hipMalloc(out, std::max<size_t>(bytes, 1)));
    return ARX_OK;
}

void arx_device_free(int32_t device, void* p) {
    if (!p) return;
    hipSetDevice(device);
    hipFree(p);
}

arx_status arx_memcpy(int32_t device, void* dst, const void* src, size_t bytes) {
    if (bytes > 0 && (!dst || !src)) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    ARX_HIP(hipSetDevice(device));
    if (bytes > 0) ARX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
    return ARX_OK;
}

const char* arx_status_string(arx_status s) {
    switch (s) {
        case ARX_OK: return "ok";
        case ARX_ERR_INVALID_ARGUMENT: return "invalid argument";
        case ARX_ERR_HIP: return "HIP error";
        case ARX_ERR_OUT_OF_MEMORY: return "out of memory";
        case ARX_ERR_NOT_READY: return "not ready";
        case ARX_ERR_IO: return "I/O error";
        case ARX_ERR_INTERNAL: return "internal error";
    }
    return "unknown status";
}

const char* arx_last_error(void) { return g_last_error.c_str(); }

int arx_abi_version(void) { return ARX_ABI_VERSION; }

int arx_frac_bits(uint64_t n) {
    int lg = 0;
    while (((uint64_t)1 << lg) < n && lg < 63) ++lg;
    int fb = 59 - lg;
    return std::min(52, std::max(8, fb));
}

void arx_default_config(arx_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->rays_x = c->rays_y = c->rays_z = 100;  // Context.cpp:114
    c->ir_length_in_seconds = 2;              // :21
    c->sample_rate = 44100;                   // live-mode default (:221)
    c->base_power = 100.0f;                   // :113
    c->energy_thres = 0.0f;                   // :115
    c->max_bounces = 10;                      // :116
    c->hrtf_absorption_rate = 1.0f;           // round(0.9) (:117, :145)
    c->is_mono = 0;
    c->seed = 1;
    c->device = 0;
}

float arx_material_absorption(const char* name, const char* const* names, const float* absorption, size_t n) {
    if (!name) return 0.5f;
    if (std::strcmp(name, "receiver_left") == 0) return -1.0f;
    if (std::strcmp(name, "receiver_right") == 0) return -2.0f;
    for (size_t i = 0; i < n; ++i)
        if (names && names[i] && std::strcmp(names[i], name) == 0) return absorption[i];
    return 0.5f;
}

arx_status arx_create(const arx_config* cfg, arx_renderer** out) {
    if (!out) return fail(ARX_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    arx_status st = check_config(cfg);
    if (st != ARX_OK) return st;
    int ndev = 0;
    ARX_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(ARX_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", cfg->device, ndev);
    ARX_HIP(hipSetDevice(cfg->device));
    arx_renderer* r = new (std::nothrow) arx_renderer();
    if (!r) return fail(ARX_ERR_OUT_OF_MEMORY, "host allocation failed");
    std::memset(&r->stats, 0, sizeof(r->stats));
    r->cfg = *cfg;
    r->ir_len = (int32_t)(cfg->ir_length_in_seconds * (uint32_t)cfg->sample_rate);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) r->cus = prop.multiProcessorCount;
    auto cleanup = [&](arx_status s) {
        arx_destroy(r);
        return s;
    };
    hipError_t e;
    if ((st = alloc_frame_set(r->ir_len, r->sets[0])) != ARX_OK || (st = r->d_tree_flag.reserve(1)) != ARX_OK ||
        (st = r->h_tree_flag.reserve(1)) != ARX_OK)
        return cleanup(st);
    r->stream = r->cur().stream;
    // the analysis ring's events are made by the first analyses
    if ((st = r->trace_ring.create_all()) != ARX_OK || (st = r->conv_ring.create_all()) != ARX_OK ||
        (st = r->live_ring.create_all()) != ARX_OK)
        return cleanup(st);
    // the production trace kernels' register allocation, as the runtime sees it (arx_stats)
    for (int f = 0; f < 3; ++f)
        for (int inst = 0; inst < 3; ++inst)
            if ((e = trace_kernel_occupancy(f, inst, &r->occ[f][inst][0], &r->occ[f][inst][1], &r->occ[f][inst][2])) !=
                hipSuccess)
                return cleanup(fail(ARX_ERR_HIP, "arx_create: trace kernel attributes: %s", hipGetErrorString(e)));
    r->stats.trace_vgprs = r->occ[kFmtQ16][0][0];
    r->stats.trace_waves_per_simd = r->occ[kFmtQ16][0][1];
    r->stats.trace_waves_target = r->occ[kFmtQ16][0][2];
    r->stats.trace_format = kFmtQ16;
    r->stats.trace_grid_cus = r->cus;
    if ((e = hipMemsetAsync(r->d_tree_flag.p, 0, sizeof(unsigned int), r->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(r->stream)) != hipSuccess)
        return cleanup(fail(ARX_ERR_HIP, "arx_create: %s", hipGetErrorString(e)));
    *out = r;
    return ARX_OK;
}

void arx_destroy(arx_renderer* r) {
    if (!r) return;
    hipSetDevice(r->cfg.device);
    sync_renderer(r);
    for (int k = 0; k < arx_renderer::kMaxFrames; ++k)
        for (hipEvent_t e : {r->ev_traced[k], r->ev_conv[k], r->ev_reduced[k], r->ev_scene[k]})
            if (e) hipEventDestroy(e);
    for (arx_stream* s : r->streams) release_stream(s);  // the handles stay valid but detached
    r->streams.clear();
    if (r->conv) conv_plan_destroy(r->conv);
    if (r->conv_live) conv_plan_destroy(r->conv_live);
    r->release_buffers();
    r->path_cache.release();
    r->listeners.release();
    r->walk.release();
    r->bands.release();
    r->directivity.release();
    r->air.release();
    r->synth.release();
    r->listener_bands.release();
    for (EventRing* ring : {&r->trace_ring, &r->conv_ring, &r->live_ring, &r->analysis_ring}) ring->destroy();
    for (auto& f : r->sets) f.release();
    delete r;
}

arx_status arx_get_config(const arx_renderer* r, arx_config* out) {
    if (!r || !out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = r->cfg;
    return ARX_OK;
}

arx_status arx_set_stream(arx_renderer* r, void* s) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (r->fif != 1) return fail(ARX_ERR_INVALID_ARGUMENT, "a caller's stream needs one frame in flight (arx_set_frames_in_flight)");
    r->stream = (hipStream_t)s;
    return ARX_OK;
}

void* arx_get_stream(const arx_renderer* r) { return r ? (void*)r->stream : nullptr; }

arx_status arx_set_emitter(arx_renderer* r, float x, float y, float z) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->emitter[0] = x;
    r->emitter[1] = y;
    r->emitter[2] = z;
    return ARX_OK;
}

arx_status arx_set_listener(arx_renderer* r, float x, float y, float z, float yaw_deg) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->center[0] = x;
    r->center[1] = y;
    r->center[2] = z;
    r->yaw = yaw_deg;
    r->recv_pose_dirty = true;
    return ARX_OK;
}

arx_status arx_set_thresholds(arx_renderer* r, float energy, uint32_t max_bounces) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->cfg.energy_thres = energy;
    r->cfg.max_bounces = max_bounces;
    return ARX_OK;
}

arx_status arx_set_hrtf_absorption_rate(arx_renderer* r, float v) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (!(v >= 0.0f && v <= 1.0f))  // the cross-ear factor (1 - hrtf) stays in [0, 1] (histogram headroom)
        return fail(ARX_ERR_INVALID_ARGUMENT, "hrtf_absorption_rate %g must be in [0, 1]", (double)v);
    r->cfg.hrtf_absorption_rate = v;
    return ARX_OK;
}

arx_status arx_set_base_power(arx_renderer* r, float v) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->cfg.base_power = v;
    return ARX_OK;
}

arx_status arx_set_mono_output(arx_renderer* r, int mono) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->cfg.is_mono = mono ? 1 : 0;
    return ARX_OK;
}

arx_status arx_set_seed(arx_renderer* r, uint64_t seed) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->cfg.seed = seed;
    return ARX_OK;
}

arx_status arx_set_timing(arx_renderer* r, int32_t on) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    r->timing = on != 0;
    return ARX_OK;
}

arx_status arx_set_frames_in_flight(arx_renderer* r, int32_t n) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n < 1 || n > arx_renderer::kMaxFrames)
        return fail(ARX_ERR_INVALID_ARGUMENT, "frames in flight: 1 to %d, not %d", arx_renderer::kMaxFrames, n);
    if (n == r->fif) return ARX_OK;
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (n > 1 && r->stream != r->cur().stream)
        return fail(ARX_ERR_INVALID_ARGUMENT, "frames in flight need the renderer's own streams (arx_set_stream)");
    if (n > 1 && r->d_hist_ext) return fail(ARX_ERR_INVALID_ARGUMENT, "frames in flight need the renderer's own histograms");
    // nothing of the old arrangement stays in flight: the sets' order and the event slots start over
    const arx_status st = sync_renderer(r);
    if (st != ARX_OK) return st;
    std::swap(r->sets[0], r->sets[r->slot]);  // the current set stays, as set 0
    r->slot = 0;
    r->last_conv = r->last_reduced = r->last_scene = -1;
    // the path cache's records name the stream that made them and the sets that replayed them
    r->path_cache.recorded = r->path_cache.last_valid = r->path_cache.last_filtered = false;
    for (bool& b : r->path_cache.replayed) b = false;
    for (int k = n; k < arx_renderer::kMaxFrames; ++k) r->sets[k].release();
    for (int k = 0; k < n; ++k)
        for (hipEvent_t* e : {&r->ev_traced[k], &r->ev_conv[k], &r->ev_reduced[k], &r->ev_scene[k]})
            if (!*e) ARX_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (int k = 1; k < n; ++k) {
        if (r->sets[k].stream) continue;
        if (const arx_status se = alloc_frame_set(r->ir_len, r->sets[k]); se != ARX_OK) {
            for (int q = 1; q < arx_renderer::kMaxFrames; ++q) r->sets[q].release();
            r->fif = 1;
            return se;
        }
    }
    r->fif = n;
    return ARX_OK;
}

arx_status arx_histogram_device(arx_renderer* r, int64_t** d_hist, size_t* n) {
    if (!r || !d_hist) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    *d_hist = (int64_t*)r->hist();
    if (n) *n = 2 * (size_t)r->ir_len;
    return ARX_OK;
}

arx_status arx_attach_histogram(arx_renderer* r, int64_t* d_hist, size_t n) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (d_hist && n != 2 * (size_t)r->ir_len)
        return fail(ARX_ERR_INVALID_ARGUMENT, "histogram needs 2*ir_len = %zu elements, got %zu", 2 * (size_t)r->ir_len, n);
    if (d_hist && r->fif != 1)
        return fail(ARX_ERR_INVALID_ARGUMENT, "an attached histogram needs one frame in flight (arx_set_frames_in_flight)");
    r->d_hist_ext = (unsigned long long*)d_hist;
    return ARX_OK;
}

arx_status arx_ir_device(arx_renderer* r, float** d_left, float** d_right, size_t* ir_len) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (d_left) *d_left = r->cur().d_ir.p;
    if (d_right) *d_right = r->cur().d_ir.p + r->ir_len;
    if (ir_len) *ir_len = (size_t)r->ir_len;
    return ARX_OK;
}

arx_status arx_copy_ir(arx_renderer* r, float* h_left, float* h_right, size_t ir_len) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (ir_len != (size_t)r->ir_len) return fail(ARX_ERR_INVALID_ARGUMENT, "ir_len %zu != %d", ir_len, r->ir_len);
    ARX_HIP(hipSetDevice(r->cfg.device));
    const float* d_ir = r->cur().d_ir.p;
    if (h_left) ARX_HIP(hipMemcpyAsync(h_left, d_ir, ir_len * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    if (h_right) ARX_HIP(hipMemcpyAsync(h_right, d_ir + r->ir_len, ir_len * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

arx_status arx_get_stats(arx_renderer* r, arx_stats* out) {
    if (!r || !out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    ARX_HIP(hipSetDevice(r->cfg.device));
    const arx_renderer::FrameSet& f = r->cur();
    ARX_HIP(hipMemcpyAsync(f.h_counters.p, f.d_counters.p, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           r->stream));
    ARX_HIP(hipMemcpyAsync(r->h_tree_flag.p, r->d_tree_flag.p, sizeof(unsigned int), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    r->stats.queries = f.h_counters.p[0];
    r->stats.receiver_hits = f.h_counters.p[1];
    r->stats.misses = f.h_counters.p[2];
    double ms = 0.0;
    if (r->trace_ring.launches > 0 && r->trace_ring.last_ms(false, &ms) == ARX_OK) r->stats.trace_ms = ms;
    if (r->conv_ring.launches > 0 && r->conv_ring.last_ms(false, &ms) == ARX_OK) r->stats.conv_ms = ms;
    *out = r->stats;
    // the tree as last written (generation tree_gen) has a box off the quantization grid
    if (r->tree_gen != 0 && *r->h_tree_flag.p == r->tree_gen)
        return fail(ARX_ERR_INTERNAL, "receiver refit / re-quantization: a box left the quantization grid");
    return ARX_OK;
}

}  // extern "C"
