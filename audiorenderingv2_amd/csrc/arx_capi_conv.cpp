// arx_capi_conv.cpp -- the convolution behind the C ABI (include/arx.h): the IR setters, the file
// and live convolution plans and entry points (convoluteAudioFile and the live mode of
// R/prebuild/obj_raytracer/AudioRenderer.cpp), the streaming convolution (UPOLS,
// arx_conv_stream.hip) and the walk-through convolution over a per-block IR schedule
// (arx_conv_walk.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

// A streaming convolution (arx_stream_*).  It belongs to its renderer: arx_destroy releases the
// device side of every stream still attached (r = NULL afterwards), so a stream outliving its
// renderer fails cleanly instead of touching freed memory.
struct arx_stream {
    arx_renderer* r = nullptr;
    int device = 0;
    StreamPlan* plan = nullptr;
    uint64_t ir_generation = ~0ull;  // the IR the partition spectra were made from
    int32_t fade_shape = ARX_FADE_HANN;  // arx_stream_set_crossfade (the frames: stream_plan_fade)
    uint64_t crossfades = 0;             // transition blocks processed
    DeviceBuf<double> d_in;          // host-API staging: block frames in, 2 * block out
    DeviceBuf<double> d_out;
};

namespace {
arx_status live_stream(const arx_stream* s) {
    if (!s) return fail(ARX_ERR_INVALID_ARGUMENT, "stream is NULL");
    if (!s->r) return fail(ARX_ERR_NOT_READY, "the stream's renderer was destroyed");
    return ARX_OK;
}

// spectra = false: leave a changed IR's spectra to the next conv_run (which folds them into its
// own first pass)
arx_status ensure_conv(arx_renderer* r, bool spectra = true) {
    if (!r->conv) {
        char err[256] = {0};
        r->conv = conv_plan_create(r->ir_len, r->cfg.sample_rate, r->cfg.device, err, sizeof(err));
        if (!r->conv) return fail(ARX_ERR_INTERNAL, "convolution plan: %s", err);
        r->conv_ir_dirty = true;
    }
    if (spectra && r->conv_ir_dirty) {
        ARX_HIP(conv_set_ir(r->conv, r->cur().d_ir.p, r->cur().d_ir.p + r->ir_len, r->stream));
        r->conv_ir_dirty = false;
    }
    return ARX_OK;
}

arx_status ensure_conv_live(arx_renderer* r, int32_t block) {
    if (!r->conv_live || conv_plan_block(r->conv_live) < block) {
        if (r->conv_live) conv_plan_destroy(r->conv_live);
        char err[256] = {0};
        // plan block = the longest block seen, rounded up to 4096 frames (main.cpp:37)
        const int32_t b = std::min<int32_t>(r->ir_len, std::max<int32_t>(4096, block));
        r->conv_live = conv_plan_create(r->ir_len, b, r->cfg.device, err, sizeof(err));
        if (!r->conv_live) return fail(ARX_ERR_INTERNAL, "live convolution plan: %s", err);
        r->conv_live_ir_dirty = true;
    }
    if (r->conv_live_ir_dirty) {
        ARX_HIP(conv_set_ir(r->conv_live, r->cur().d_ir.p, r->cur().d_ir.p + r->ir_len, r->stream));
        r->conv_live_ir_dirty = false;
    }
    return ARX_OK;
}
}  // namespace

void arx::release_stream(arx_stream* s) {
    hipSetDevice(s->device);
    if (s->r) sync_renderer(s->r);
    if (s->plan) stream_plan_destroy(s->plan);
    s->d_in.release();
    s->d_out.release();
    s->plan = nullptr;
    s->r = nullptr;
}

arx_status arx::reserve_conv_staging(arx_renderer* r, size_t n) {
    if (n <= r->d_conv_in.cap && 2 * n <= r->d_conv_out.cap) return ARX_OK;
    r->d_conv_in.release();
    r->d_conv_out.release();
    if (const arx_status st = r->d_conv_in.reserve(n); st != ARX_OK) return st;
    return r->d_conv_out.reserve(2 * n);
}

arx_status arx::convolute_pairs(arx_renderer* r, const float* d_in, size_t n_frames, float* d_out_left,
                                float* d_out_right, int64_t pair_begin, int64_t pair_end, bool timed) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n_frames > 0 && (!d_in || !d_out_left || !d_out_right)) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    ARX_HIP(hipSetDevice(r->cfg.device));
    // the plan's spectra and scratch, and the caller's outputs, are shared with the other frame in flight
    arx_status st = fif_wait_conv(r);
    if (st == ARX_OK) st = ensure_conv(r, false);
    if (st != ARX_OK) return st;
    const bool ir_new = r->conv_ir_dirty;
    float* d_ir = r->cur().d_ir.p;
    if (timed && (st = r->conv_ring.begin(r->stream)) != ARX_OK) return st;
    ARX_HIP(conv_run_pairs(r->conv, d_in, (int64_t)n_frames, d_out_left, d_out_right, ir_new ? d_ir : nullptr,
                           ir_new ? d_ir + r->ir_len : nullptr, pair_begin, pair_end, r->stream));
    r->conv_ir_dirty = false;
    if (timed && (st = r->conv_ring.end(r->stream)) != ARX_OK) return st;
    return fif_done_conv(r);
}

bool arx::conv_shards(arx_renderer* r) {
    return ensure_conv(r, false) == ARX_OK && conv_plan_shards(r->conv);
}

extern "C" {

arx_status arx_set_ir(arx_renderer* r, const float* h_left, const float* h_right, size_t ir_len) {
    if (!r || !h_left || !h_right) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (ir_len != (size_t)r->ir_len) return fail(ARX_ERR_INVALID_ARGUMENT, "ir_len %zu != %d", ir_len, r->ir_len);
    ARX_HIP(hipSetDevice(r->cfg.device));
    float* d_ir = r->cur().d_ir.p;
    ARX_HIP(hipMemcpyAsync(d_ir, h_left, ir_len * sizeof(float), hipMemcpyHostToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(d_ir + r->ir_len, h_right, ir_len * sizeof(float), hipMemcpyHostToDevice, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    r->conv_ir_dirty = true;
    r->conv_live_ir_dirty = true;
    ++r->ir_generation;
    return ARX_OK;
}

arx_status arx_set_ir_device(arx_renderer* r, const float* d_left, const float* d_right, size_t ir_len) {
    if (!r || !d_left || !d_right) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (ir_len != (size_t)r->ir_len) return fail(ARX_ERR_INVALID_ARGUMENT, "ir_len %zu != %d", ir_len, r->ir_len);
    ARX_HIP(hipSetDevice(r->cfg.device));
    float* d_ir = r->cur().d_ir.p;
    ARX_HIP(hipMemcpyAsync(d_ir, d_left, ir_len * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(d_ir + r->ir_len, d_right, ir_len * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
    r->conv_ir_dirty = true;
    r->conv_live_ir_dirty = true;
    ++r->ir_generation;
    return ARX_OK;
}

arx_status arx_prepare_ir_spectra(arx_renderer* r, int which) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_status st = fif_wait_conv(r);
    if (st == ARX_OK && (which & 1)) st = ensure_conv(r);
    if (st == ARX_OK && (which & 2)) st = ensure_conv_live(r, 1);
    return st == ARX_OK ? fif_done_conv(r) : st;
}

arx_status arx_conv_describe(arx_renderer* r, int which, char* buf, size_t len) {
    if (!r || !buf || len == 0) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL renderer or buffer");
    if (which != 1 && which != 2) return fail(ARX_ERR_INVALID_ARGUMENT, "which must be 1 (file) or 2 (live)");
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_status st = fif_wait_conv(r);
    if (st == ARX_OK) st = which == 1 ? ensure_conv(r) : ensure_conv_live(r, 1);
    if (st != ARX_OK) return st;
    std::snprintf(buf, len, "%s", conv_plan_describe(which == 1 ? r->conv : r->conv_live));
    return fif_done_conv(r);
}

arx_status arx_convolute_device(arx_renderer* r, const float* d_in, size_t n_frames, float* d_out_left,
                                float* d_out_right) {
    return r ? arx::convolute_pairs(r, d_in, n_frames, d_out_left, d_out_right, 0, INT64_MAX, r->timing)
             : fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
}

arx_status arx_convolute_prepare_input(arx_renderer* r, const float* d_in, size_t n_frames) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n_frames > 0 && !d_in) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_status st = fif_wait_conv(r);  // the plan's scratch is shared with the other frame in flight
    if (st == ARX_OK) st = ensure_conv(r, false);
    if (st != ARX_OK) return st;
    ARX_HIP(conv_prepare_input(r->conv, d_in, (int64_t)n_frames, r->stream));
    return fif_done_conv(r);
}

arx_status arx_convolute_prepared(arx_renderer* r, float* d_out_left, float* d_out_right, size_t* n_frames) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (!r->conv || !conv_has_prepared(r->conv))
        return fail(ARX_ERR_NOT_READY, "no prepared input (arx_convolute_prepare_input; another file convolution on "
                                       "this renderer discards it)");
    const int64_t n = conv_prepared_frames(r->conv);
    if (n > 0 && (!d_out_left || !d_out_right)) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_status st = fif_wait_conv(r);
    if (st != ARX_OK) return st;
    const bool ir_new = r->conv_ir_dirty;
    float* d_ir = r->cur().d_ir.p;
    if (r->timing && (st = r->conv_ring.begin(r->stream)) != ARX_OK) return st;
    ARX_HIP(conv_run_prepared(r->conv, d_out_left, d_out_right, ir_new ? d_ir : nullptr, ir_new ? d_ir + r->ir_len : nullptr,
                              r->stream));
    r->conv_ir_dirty = false;
    if (r->timing && (st = r->conv_ring.end(r->stream)) != ARX_OK) return st;
    if (n_frames) *n_frames = (size_t)n;
    return fif_done_conv(r);
}

arx_status arx_convolute_audio_file(arx_renderer* r, const float* h_in, size_t in_bytes, float* h_out_left,
                                    float* h_out_right, double* conv_ms, double* proc_ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const size_t n = in_bytes / sizeof(float);  // AudioRenderer.cpp:689: bytes / sizeof(float)
    if (n > 0 && (!h_in || !h_out_left || !h_out_right)) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (const arx_status w = fif_wait_conv(r); w != ARX_OK) return w;  // the staging buffers below
    struct Events {  // destroyed on every return below
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) hipEventDestroy(x);
        }
    } ev;
    ARX_HIP(hipEventCreate(&ev.e[0]));
    ARX_HIP(hipEventCreate(&ev.e[1]));
    hipEvent_t p0 = ev.e[0], p1 = ev.e[1];
    ARX_HIP(hipEventRecord(p0, r->stream));
    if (const arx_status rs = reserve_conv_staging(r, n); rs != ARX_OK) return rs;
    if (n > 0) ARX_HIP(hipMemcpyAsync(r->d_conv_in.p, h_in, n * sizeof(float), hipMemcpyHostToDevice, r->stream));
    // timed when asked for the convolution's own window
    const arx_status st = convolute_pairs(r, r->d_conv_in.p, n, r->d_conv_out.p, r->d_conv_out.p + n, 0, INT64_MAX,
                                          r->timing || conv_ms != nullptr);
    if (st != ARX_OK) return st;
    if (n > 0) {
        ARX_HIP(hipMemcpyAsync(h_out_left, r->d_conv_out.p, n * sizeof(float), hipMemcpyDeviceToHost, r->stream));
        ARX_HIP(hipMemcpyAsync(h_out_right, r->d_conv_out.p + n, n * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    }
    ARX_HIP(hipEventRecord(p1, r->stream));
    ARX_HIP(hipEventSynchronize(p1));
    if (conv_ms)
        if (const arx_status t = r->conv_ring.last_ms(false, conv_ms); t != ARX_OK) return t;
    if (proc_ms) {
        float ms = 0.f;
        ARX_HIP(hipEventElapsedTime(&ms, p0, p1));
        *proc_ms = ms;
    }
    return ARX_OK;
}

arx_status arx_convolute_live_device(arx_renderer* r, const double* d_in, size_t n_in, double* d_out) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n_in > (size_t)r->ir_len)  // the reference copies the block into an ir_len buffer (AudioRenderer.cpp:600-603)
        return fail(ARX_ERR_INVALID_ARGUMENT, "live block of %zu samples exceeds ir_len %d", n_in, r->ir_len);
    if ((n_in > 0 && !d_in) || !d_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_status st = fif_wait_conv(r);
    if (st == ARX_OK) st = ensure_conv_live(r, (int32_t)std::max<size_t>(n_in, 1));
    if (st != ARX_OK) return st;
    if ((st = r->live_ring.begin(r->stream)) != ARX_OK) return st;
    ARX_HIP(conv_run_live(r->conv_live, d_in, (int64_t)n_in, d_out, r->stream));
    if ((st = r->live_ring.end(r->stream)) != ARX_OK) return st;
    return fif_done_conv(r);
}

arx_status arx_convolute_live_block(arx_renderer* r, const double* h_in, size_t in_bytes, double* h_out,
                                    size_t out_len) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    const size_t n_in = in_bytes / sizeof(double);
    if (out_len != 2 * (size_t)r->ir_len)
        return fail(ARX_ERR_INVALID_ARGUMENT, "output must hold 2*ir_len = %zu doubles", 2 * (size_t)r->ir_len);
    if ((n_in > 0 && !h_in) || !h_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (n_in > (size_t)r->ir_len)
        return fail(ARX_ERR_INVALID_ARGUMENT, "live block of %zu samples exceeds ir_len %d", n_in, r->ir_len);
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (const arx_status w = fif_wait_conv(r); w != ARX_OK) return w;  // the staging buffers below
    arx_status st;
    if ((st = r->d_live_in.reserve((size_t)r->ir_len)) != ARX_OK || (st = r->d_live_out.reserve(2 * (size_t)r->ir_len)) != ARX_OK)
        return st;
    if (n_in > 0) ARX_HIP(hipMemcpyAsync(r->d_live_in.p, h_in, n_in * sizeof(double), hipMemcpyHostToDevice, r->stream));
    if ((st = arx_convolute_live_device(r, r->d_live_in.p, n_in, r->d_live_out.p)) != ARX_OK) return st;
    ARX_HIP(hipMemcpyAsync(h_out, r->d_live_out.p, out_len * sizeof(double), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

// ---- streaming convolution (UPOLS, arx_conv_stream.hip) -------------------------------------------

arx_status arx_stream_create(arx_renderer* r, int32_t block_frames, arx_stream** out) {
    if (!r || !out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (block_frames <= 0 || block_frames > 4096 || block_frames > r->ir_len)
        return fail(ARX_ERR_INVALID_ARGUMENT, "stream block of %d frames: must be in [1, min(4096, ir_len)]", block_frames);
    ARX_HIP(hipSetDevice(r->cfg.device));
    arx_stream* s = new (std::nothrow) arx_stream();
    if (!s) return fail(ARX_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->r = r;
    s->device = r->cfg.device;
    char err[256] = {0};
    s->plan = stream_plan_create(r->ir_len, block_frames, r->cfg.device, err, sizeof(err));
    if (!s->plan) {
        delete s;
        return fail(ARX_ERR_INTERNAL, "stream plan: %s", err);
    }
    arx_status st;
    if ((st = s->d_in.reserve((size_t)block_frames)) != ARX_OK || (st = s->d_out.reserve(2 * (size_t)block_frames)) != ARX_OK) {
        release_stream(s);
        delete s;
        return st;
    }
    r->streams.push_back(s);
    *out = s;
    return ARX_OK;
}

void arx_stream_destroy(arx_stream* s) {
    if (!s) return;
    if (s->r) {
        std::vector<arx_stream*>& v = s->r->streams;
        v.erase(std::remove(v.begin(), v.end(), s), v.end());
        release_stream(s);
    }
    delete s;
}

arx_status arx_stream_reset(arx_stream* s) {
    arx_status st = live_stream(s);
    if (st != ARX_OK) return st;
    ARX_HIP(hipSetDevice(s->r->cfg.device));
    if (const arx_status w = fif_wait_conv(s->r); w != ARX_OK) return w;
    ARX_HIP(stream_reset(s->plan, s->r->stream));
    return fif_done_conv(s->r);
}

arx_status arx_stream_info(const arx_stream* s, int32_t* block, int32_t* partitions, int32_t* fft_size) {
    const arx_status st = live_stream(s);
    if (st != ARX_OK) return st;
    if (block) *block = stream_plan_block(s->plan);
    if (partitions) *partitions = stream_plan_partitions(s->plan);
    if (fft_size) *fft_size = stream_plan_fft(s->plan);
    return ARX_OK;
}

arx_status arx_stream_process_device(arx_stream* s, const double* d_in, size_t n_frames, double* d_out) {
    if (const arx_status st0 = live_stream(s); st0 != ARX_OK) return st0;
    const int32_t B = stream_plan_block(s->plan);
    if (n_frames > (size_t)B) return fail(ARX_ERR_INVALID_ARGUMENT, "%zu frames exceed the stream block %d", n_frames, B);
    if ((n_frames > 0 && !d_in) || !d_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    arx_renderer* r = s->r;
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (const arx_status w = fif_wait_conv(r); w != ARX_OK) return w;  // the stream's delay line and spectra
    bool transition = false;
    if (s->ir_generation != r->ir_generation) {  // the IR changed: new partition spectra
        // a transition block: a fade is on and the last block (since creation or the last reset) ran
        // with the spectra that are current until now; they become the previous set
        transition = stream_plan_fade(s->plan) > 0 && s->ir_generation != ~0ull && stream_plan_blocks(s->plan) > 0;
        ARX_HIP(stream_set_ir(s->plan, r->cur().d_ir.p, r->cur().d_ir.p + r->ir_len, transition, r->stream));
        s->ir_generation = r->ir_generation;
    }
    if (const arx_status t = r->live_ring.begin(r->stream); t != ARX_OK) return t;
    if (transition) {
        ARX_HIP(stream_run_xfade(s->plan, d_in, (int64_t)n_frames, d_out, r->stream));
        ++s->crossfades;
    } else {
        ARX_HIP(stream_run(s->plan, d_in, (int64_t)n_frames, d_out, r->stream));
    }
    if (const arx_status t = r->live_ring.end(r->stream); t != ARX_OK) return t;
    return fif_done_conv(r);
}

arx_status arx_stream_fade_weights(int32_t shape, int32_t fade_frames, double* w) {
    if (fade_frames <= 0) return fail(ARX_ERR_INVALID_ARGUMENT, "fade of %d frames: must be positive", fade_frames);
    if (shape != ARX_FADE_LINEAR && shape != ARX_FADE_HANN) return fail(ARX_ERR_INVALID_ARGUMENT, "unknown fade shape %d", shape);
    if (!w) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    const double pi = 3.14159265358979323846;
    for (int32_t i = 0; i < fade_frames; ++i) {
        const double t = ((double)i + 0.5) / (double)fade_frames;
        w[i] = shape == ARX_FADE_LINEAR ? t : 0.5 - 0.5 * std::cos(pi * t);
    }
    return ARX_OK;
}

arx_status arx_stream_set_crossfade(arx_stream* s, int32_t fade_frames, int32_t shape) {
    if (const arx_status st0 = live_stream(s); st0 != ARX_OK) return st0;
    const int32_t B = stream_plan_block(s->plan);
    if (fade_frames < 0 || fade_frames > B)
        return fail(ARX_ERR_INVALID_ARGUMENT, "fade of %d frames: must be in [0, block = %d]", fade_frames, B);
    if (shape != ARX_FADE_LINEAR && shape != ARX_FADE_HANN) return fail(ARX_ERR_INVALID_ARGUMENT, "unknown fade shape %d", shape);
    std::vector<double> w((size_t)fade_frames);
    if (fade_frames > 0)
        if (const arx_status st = arx_stream_fade_weights(shape, fade_frames, w.data()); st != ARX_OK) return st;
    arx_renderer* r = s->r;
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (const arx_status wt = fif_wait_conv(r); wt != ARX_OK) return wt;  // blocks in flight read the weights
    const hipError_t e = stream_set_fade(s->plan, fade_frames, w.data(), r->stream);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(ARX_ERR_OUT_OF_MEMORY, "the crossfade's second set of partition spectra");
    }
    ARX_HIP(e);
    s->fade_shape = shape;
    return fif_done_conv(r);
}

arx_status arx_stream_get_crossfade(const arx_stream* s, int32_t* fade_frames, int32_t* shape) {
    if (const arx_status st0 = live_stream(s); st0 != ARX_OK) return st0;
    if (fade_frames) *fade_frames = stream_plan_fade(s->plan);
    if (shape) *shape = s->fade_shape;
    return ARX_OK;
}

arx_status arx_stream_crossfades(const arx_stream* s, uint64_t* n) {
    if (const arx_status st0 = live_stream(s); st0 != ARX_OK) return st0;
    if (!n) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    *n = s->crossfades;
    return ARX_OK;
}

arx_status arx_stream_process(arx_stream* s, const double* h_in, size_t n_frames, double* h_out, size_t out_len) {
    if (const arx_status st0 = live_stream(s); st0 != ARX_OK) return st0;
    const int32_t B = stream_plan_block(s->plan);
    if (out_len != 2 * (size_t)B) return fail(ARX_ERR_INVALID_ARGUMENT, "output must hold 2*block = %d doubles", 2 * B);
    if (n_frames > (size_t)B) return fail(ARX_ERR_INVALID_ARGUMENT, "%zu frames exceed the stream block %d", n_frames, B);
    if ((n_frames > 0 && !h_in) || !h_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL buffer");
    arx_renderer* r = s->r;
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (const arx_status w = fif_wait_conv(r); w != ARX_OK) return w;  // the staging buffers below
    if (n_frames > 0)
        ARX_HIP(hipMemcpyAsync(s->d_in.p, h_in, n_frames * sizeof(double), hipMemcpyHostToDevice, r->stream));
    const arx_status st = arx_stream_process_device(s, s->d_in.p, n_frames, s->d_out.p);
    if (st != ARX_OK) return st;
    ARX_HIP(hipMemcpyAsync(h_out, s->d_out.p, out_len * sizeof(double), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ARX_OK;
}

// ---- walk-through convolution (arx_conv_walk.hip) ---------------------------------------------------

arx_status arx_convolute_walk(arx_renderer* r, const float* ir_left, const float* ir_right, size_t n_irs,
                              const int32_t* ir_of_block, size_t n_blocks, const double* in, size_t n_frames,
                              int32_t block_frames, int32_t fade_frames, int32_t fade_shape, double* out, double* ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n_blocks == 0) return ARX_OK;
    if (!ir_left || !ir_right || !ir_of_block || !out || (n_frames > 0 && !in))
        return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_irs == 0) return fail(ARX_ERR_INVALID_ARGUMENT, "no IRs");
    const int32_t B = block_frames, F = fade_frames;
    if (B <= 0 || B > 4096 || B > r->ir_len)
        return fail(ARX_ERR_INVALID_ARGUMENT, "walk block of %d frames: must be in [1, min(4096, ir_len)]", B);
    if (F < 0 || F > B) return fail(ARX_ERR_INVALID_ARGUMENT, "fade of %d frames: must be in [0, block = %d]", F, B);
    if (fade_shape != ARX_FADE_LINEAR && fade_shape != ARX_FADE_HANN)
        return fail(ARX_ERR_INVALID_ARGUMENT, "unknown fade shape %d", fade_shape);
    if (n_blocks > (size_t)(INT32_MAX / 2)) return fail(ARX_ERR_INVALID_ARGUMENT, "%zu blocks are too many", n_blocks);
    if (n_frames > n_blocks * (size_t)B)
        return fail(ARX_ERR_INVALID_ARGUMENT, "%zu frames exceed %zu blocks of %d", n_frames, n_blocks, B);
    for (size_t b = 0; b < n_blocks; ++b)
        if (ir_of_block[b] < 0 || (size_t)ir_of_block[b] >= n_irs)
            return fail(ARX_ERR_INVALID_ARGUMENT, "block %zu names IR %d of %zu", b, ir_of_block[b], n_irs);
    WalkScratch& w = r->walk;
    const size_t n = (size_t)r->ir_len;

    // the schedule as items: the distinct IRs it names get slots in order of first use; a transition
    // block's item of the previous IR goes in front of the block's own
    std::vector<int32_t>& slot = w.h_slot;
    slot.assign(n_irs, -1);
    std::vector<int32_t> used;  // slot -> IR
    size_t n_trans = 0;
    for (size_t b = 0; b < n_blocks; ++b) {
        const int32_t j = ir_of_block[b];
        if (slot[(size_t)j] < 0) {
            slot[(size_t)j] = (int32_t)used.size();
            used.push_back(j);
        }
        if (F > 0 && b > 0 && j != ir_of_block[b - 1]) ++n_trans;
    }
    const size_t n_items = n_blocks + n_trans;
    std::vector<int32_t>& tab = w.h_tables;
    tab.assign(3 * n_items + n_trans, 0);
    int32_t *item_block = tab.data(), *item_ir = item_block + n_items, *item_trans = item_ir + n_items,
            *trans_block = item_trans + n_items;
    size_t i = 0, t = 0;
    for (size_t b = 0; b < n_blocks; ++b) {
        const int32_t j = ir_of_block[b];
        if (F > 0 && b > 0 && j != ir_of_block[b - 1]) {
            item_block[i] = (int32_t)b;
            item_ir[i] = slot[(size_t)ir_of_block[b - 1]];
            item_trans[i++] = (int32_t)t;
            trans_block[t++] = (int32_t)b;
        }
        item_block[i] = (int32_t)b;
        item_ir[i] = slot[(size_t)j];
        item_trans[i++] = -1;
    }
    const WalkLayout lay = walk_layout(r->ir_len, B, used.size(), n_blocks, n_trans, F);
    if ((uint64_t)used.size() * (uint64_t)lay.P > (uint64_t)INT32_MAX)
        return fail(ARX_ERR_INVALID_ARGUMENT, "%zu IRs of %d partitions are too many", used.size(), lay.P);

    ARX_HIP(hipSetDevice(r->cfg.device));
    if (const arx_status wt = fif_wait_conv(r); wt != ARX_OK) return wt;
    if (lay.total > w.d_scratch.cap) {  // nothing of an earlier call is in flight: every call ends synchronised
        w.tw_n = 0;
        if (const arx_status rs = w.d_scratch.reserve(lay.total); rs != ARX_OK) return rs;
    }
    char* base = w.d_scratch.p;
    const bool timed = r->timing || ms != nullptr;
    if (timed)
        if (const arx_status tb = w.timer.begin(r->stream); tb != ARX_OK) return tb;
    if (w.tw_n != lay.N) {
        if (w.h_tw.size() != 2 * (size_t)lay.N) walk_twiddle_table(lay.N, w.h_tw);
        w.tw_n = 0;
        ARX_HIP(hipMemcpyAsync(base + lay.tw, w.h_tw.data(), w.h_tw.size() * sizeof(double), hipMemcpyHostToDevice, r->stream));
        w.tw_n = lay.N;
    }
    if (n_trans > 0) {
        w.h_w.resize((size_t)F);
        if (const arx_status fw = arx_stream_fade_weights(fade_shape, F, w.h_w.data()); fw != ARX_OK) return fw;
        ARX_HIP(hipMemcpyAsync(base + lay.w, w.h_w.data(), (size_t)F * sizeof(double), hipMemcpyHostToDevice, r->stream));
    }
    ARX_HIP(hipMemcpyAsync(base + lay.tables, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, r->stream));
    float* d_l = reinterpret_cast<float*>(base + lay.irs);
    float* d_r = d_l + used.size() * n;
    for (size_t u = 0; u < used.size();) {  // runs of consecutive IRs in one copy per ear
        size_t e = u + 1;
        while (e < used.size() && used[e] == used[e - 1] + 1) ++e;
        const size_t src = (size_t)used[u] * n, bytes = (e - u) * n * sizeof(float);
        ARX_HIP(hipMemcpyAsync(d_l + u * n, ir_left + src, bytes, hipMemcpyDefault, r->stream));
        ARX_HIP(hipMemcpyAsync(d_r + u * n, ir_right + src, bytes, hipMemcpyDefault, r->stream));
        u = e;
    }
    if (n_frames > 0) ARX_HIP(hipMemcpyAsync(base + lay.in, in, n_frames * sizeof(double), hipMemcpyDefault, r->stream));
    WalkArgs a{};
    a.scratch = w.d_scratch.p;
    a.layout = lay;
    a.ir_len = r->ir_len;
    a.n_frames = (int64_t)n_frames;
    a.n_blocks = (int32_t)n_blocks;
    a.n_transitions = (int32_t)n_trans;
    a.n_used = (int32_t)used.size();
    a.fade = F;
    a.tile = w.forced_tile > 0 ? w.forced_tile : kWalkTile;
    ARX_HIP(launch_walk(a, r->stream));
    ARX_HIP(hipMemcpyAsync(out, base + lay.out, 2 * n_blocks * (size_t)B * sizeof(double), hipMemcpyDefault, r->stream));
    if (timed)
        if (const arx_status te = w.timer.end(r->stream); te != ARX_OK) return te;
    if (const arx_status d = fif_done_conv(r); d != ARX_OK) return d;
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (ms)
        if (const arx_status tm = w.timer.elapsed(ms); tm != ARX_OK) return tm;
    w.state[0] = n_blocks;
    w.state[1] = n_trans;
    w.state[2] = used.size();
    w.state[3] = (n_items + (size_t)a.tile - 1) / (size_t)a.tile;
    w.state[4] = lay.total;
    return ARX_OK;
}

uint64_t arx_walk_blocks(uint64_t n_frames, int32_t block_frames, int32_t ir_len) {
    if (block_frames <= 0 || ir_len <= 0) return 0;
    const uint64_t B = (uint64_t)block_frames;
    return (n_frames + B - 1) / B + ((uint64_t)ir_len - 1 + B - 1) / B;
}

arx_status arx_walk_even_schedule(uint64_t n_input_blocks, uint64_t n_blocks, size_t n_irs, int32_t* ir_of_block) {
    if (n_irs == 0 || n_irs > (size_t)INT32_MAX || (n_blocks > 0 && !ir_of_block))
        return fail(ARX_ERR_INVALID_ARGUMENT, "bad schedule arguments");
    int32_t last = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) {
        if (b < n_input_blocks) {
            const unsigned __int128 q = (unsigned __int128)b * n_irs / n_input_blocks;
            last = (int32_t)std::min<unsigned __int128>(q, n_irs - 1);
        }
        ir_of_block[b] = last;
    }
    return ARX_OK;
}

uint64_t arx_debug_walk_bytes(int32_t ir_len, int32_t block_frames, uint64_t irs_used, uint64_t n_blocks,
                              uint64_t n_transitions, int32_t fade_frames) {
    if (ir_len <= 0 || block_frames <= 0 || block_frames > 4096 || block_frames > ir_len || fade_frames < 0 ||
        fade_frames > block_frames)
        return 0;
    return walk_layout(ir_len, block_frames, irs_used, n_blocks, n_transitions, fade_frames).total;
}

arx_status arx_debug_set_walk_tile(arx_renderer* r, int32_t blocks) {
    if (!r || blocks < 0 || blocks > kWalkTileMax)
        return fail(ARX_ERR_INVALID_ARGUMENT, "walk tile: 0 (the product's) or 1..%d", kWalkTileMax);
    r->walk.forced_tile = blocks;
    return ARX_OK;
}

arx_status arx_debug_walk_state(arx_renderer* r, uint64_t out5[5]) {
    if (!r || !out5) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    std::copy(r->walk.state, r->walk.state + 5, out5);
    return ARX_OK;
}

}  // extern "C"
