// arx_capi_bands.cpp -- frequency-band absorption behind the C ABI (include/arx.h): the band table and
// its rule, and arx_render_bands -- every band's frame from one walk over the path cache's records
// (band_replay_kernel, arx_replay.hip), each finalized and analysed as arx_render and arx_analyze_ir do it;
// and band synthesis -- arx_band_filters' filter bank (host only) and arx_combine_bands, the band IRs
// filtered and summed into one IR pair (band_synth_kernel, arx_band_synth.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

namespace {

bool is_mark(float v) { return v == -1.0f || v == -2.0f; }

// The rule for a band table (include/arx.h).  scene[t] NaN: triangle t is not in the tree (the builder
// dropped it), so no ray meets it and only the value's range is checked.  False: *bad_band / *bad_tri name
// the first offender, in band-major order.
bool band_rule_holds(const float* scene, const float* table, int32_t n_bands, int64_t n_tris, int32_t* bad_band,
                     int64_t* bad_tri) {
    for (int32_t b = 0; b < n_bands; ++b)
        for (int64_t t = 0; t < n_tris; ++t) {
            const float v = table[(int64_t)b * n_tris + t], s = scene[t];
            bool ok;
            if (std::isnan(s))
                ok = is_mark(v) || (v >= 0.0f && v <= 1.0f);
            else if (is_mark(s))
                ok = v == s;
            else
                ok = v >= s && v <= 1.0f;  // false for a NaN
            if (!ok) {
                *bad_band = b;
                *bad_tri = t;
                return false;
            }
        }
    return true;
}

uint64_t band_table_bytes(int64_t n_tris, int32_t n_bands) {
    return (uint64_t)n_tris * (uint64_t)band_width(n_bands) * sizeof(float);
}

bool synth_taps_ok(int32_t taps) { return taps >= 1 && taps <= ARX_BAND_TAPS_MAX && (taps & 1) == 1; }

// arx_combine_bands' scratch as byte offsets, every part rounded up to 256 B (include/arx.h's formula).
struct SynthLayout {
    uint64_t in_left, in_right, filters, out_left, out_right, total;
};
SynthLayout synth_layout(size_t ir_len, int32_t n_bands, int32_t taps) {
    SynthLayout s;
    Take take{256};
    const uint64_t B = (uint64_t)n_bands, L = (uint64_t)ir_len;
    s.in_left = take(4 * B * L);
    s.in_right = take(4 * B * L);
    s.filters = take(8 * B * (uint64_t)taps);
    s.out_left = take(4 * L);
    s.out_right = take(4 * L);
    s.total = take.at;
    return s;
}

}  // namespace

BandScratchLayout arx::band_scratch_layout(int32_t ir_len, int32_t n_bands) {
    BandScratchLayout s;
    Take take{16};
    const uint64_t B = (uint64_t)n_bands, L = (uint64_t)ir_len;
    s.hist = take(B * 16 * L);
    s.counters = take(B * kBandCounterWords * 8);
    s.res = take(B * 3 * sizeof(arx_acoustics));
    s.ir = take(B * 8 * L);  // the bands' left IRs, then their right IRs
    s.edc = take(24 * L);
    s.acou = take(acoustics_scratch_bytes());
    s.total = take.at;
    return s;
}

arx_status arx::record_for_bands(arx_renderer* r, uint64_t N, const arx_listener_pose* pose, ReplayProbe* probe, int32_t* warm) {
    arx_status st;
    for (;;) {
        if ((st = trace_rays(r, 0, N, false, false, probe)) != ARX_OK) return st;
        if (probe->recorded) return ARX_OK;
        const int32_t would = probe->state;  // what the next launch would do
        if (would == kPathOff) return fail(ARX_ERR_NOT_READY, "a band render replays the path cache, which is off");
        if (would == kPathNotCacheable)
            return fail(ARX_ERR_NOT_READY, "this launch is not cacheable (global stack, CW4 or f32 nodes): no records to replay");
        if (would == kPathOverCap)
            return fail(ARX_ERR_NOT_READY,
                        "the launch's records (%llu B) are over the path cache's cap or do not fit on the device "
                        "(arx_debug_set_path_cache max_bytes)",
                        (unsigned long long)arx_debug_path_cache_bytes(N, r->cfg.max_bounces));
        if (*warm == 3) return fail(ARX_ERR_NOT_READY, "the path cache did not record within three launches");
        if (*warm == 0 && pose && (st = arx_set_listener(r, pose->x, pose->y, pose->z, pose->yaw_deg)) != ARX_OK) return st;
        if ((st = arx_render(r, nullptr)) != ARX_OK) return st;
        ++*warm;
    }
}

arx_status arx::finalize_and_analyse(arx_renderer* r, const unsigned long long* hist, float* irl, float* irr,
                                     arx_acoustics* d_res, void* edc, void* acou, bool want_ir, bool analyse) {
    const long long* h = reinterpret_cast<const long long*>(hist);
    if (want_ir) ARX_HIP(launch_finalize_ir(h, irl, irr, r->ir_len, ir_unit(r->cfg), r->cfg.is_mono, r->stream));
    if (analyse) ARX_HIP(launch_acoustics(acoustics_args(r, h, static_cast<long long*>(edc), d_res, acou), r->stream));
    return ARX_OK;
}

extern "C" {

arx_status arx_band_table_check(const float* scene_absorption, const float* table, int32_t n_bands, int64_t n_tris,
                                int32_t* bad_band, int64_t* bad_tri) {
    if (bad_band) *bad_band = -1;
    if (bad_tri) *bad_tri = -1;
    if (n_bands < 0 || n_bands > kMaxBands) return fail(ARX_ERR_INVALID_ARGUMENT, "n_bands %d: 0..%d", n_bands, kMaxBands);
    if (n_tris < 0 || (n_tris > 0 && (!scene_absorption || (n_bands > 0 && !table))))
        return fail(ARX_ERR_INVALID_ARGUMENT, "bad band table arguments");
    for (int64_t t = 0; t < n_tris; ++t) {
        const float s = scene_absorption[t];
        if (!(is_mark(s) || (s >= 0.0f && s <= 1.0f))) {
            if (bad_tri) *bad_tri = t;
            return fail(ARX_ERR_INVALID_ARGUMENT, "scene absorption of triangle %lld is neither in [0, 1] nor a receiver mark",
                        (long long)t);
        }
    }
    int32_t b = -1;
    int64_t t = -1;
    if (band_rule_holds(scene_absorption, table, n_bands, n_tris, &b, &t)) return ARX_OK;
    if (bad_band) *bad_band = b;
    if (bad_tri) *bad_tri = t;
    return fail(ARX_ERR_INVALID_ARGUMENT,
                "band %d, triangle %lld: absorption %g breaks the rule (scene %g; in [scene, 1], a receiver mark kept)", b,
                (long long)t, (double)table[(int64_t)b * n_tris + t], (double)scene_absorption[t]);
}

arx_status arx_set_band_absorption(arx_renderer* r, const float* table, int32_t n_bands, int64_t n_tris) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n_bands < 0 || n_bands > kMaxBands) return fail(ARX_ERR_INVALID_ARGUMENT, "n_bands %d: 0..%d", n_bands, kMaxBands);
    BandState& bs = r->bands;
    if (n_bands == 0) {
        bs.n_bands = 0;
        return ARX_OK;
    }
    if (!table) return fail(ARX_ERR_INVALID_ARGUMENT, "table is NULL");
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    const SceneImage& img = *r->scene_img;
    if (n_tris != img.n_input || n_tris < 1)
        return fail(ARX_ERR_INVALID_ARGUMENT, "n_tris %lld: the scene has %lld triangles", (long long)n_tris,
                    (long long)img.n_input);
    // the scene's absorption by global id, from the triangle records the kernels shade
    std::vector<float> scene((size_t)n_tris, std::nanf(""));
    for (const TriRec& t : img.bvh.tris)
        if (t.id >= 0 && (int64_t)t.id < n_tris) scene[(size_t)t.id] = t.absorption;
    int32_t b = -1;
    int64_t t = -1;
    if (!band_rule_holds(scene.data(), table, n_bands, n_tris, &b, &t))
        return fail(ARX_ERR_INVALID_ARGUMENT,
                    "band %d, triangle %lld: absorption %g breaks the rule (scene %g; in [scene, 1], a receiver mark kept)",
                    b, (long long)t, (double)table[(int64_t)b * n_tris + t], (double)scene[(size_t)t]);
    const int32_t W = band_width(n_bands);
    std::vector<float> rows((size_t)n_tris * (size_t)W, 0.0f);
    for (int32_t k = 0; k < n_bands; ++k)
        for (int64_t i = 0; i < n_tris; ++i) rows[(size_t)i * W + k] = table[(int64_t)k * n_tris + i];
    ARX_HIP(hipSetDevice(r->cfg.device));
    bs.n_bands = 0;
    // no call is in flight: every arx_render_bands ends synchronised
    if (const arx_status st = bs.d_table.reserve(rows.size()); st != ARX_OK) return st;
    ARX_HIP(hipMemcpy(bs.d_table.p, rows.data(), band_table_bytes(n_tris, n_bands), hipMemcpyHostToDevice));
    bs.n_bands = n_bands;
    bs.n_tris = n_tris;
    return ARX_OK;
}

arx_status arx_render_bands(arx_renderer* r, float* ir_left, float* ir_right, arx_acoustics* acoustics,
                            arx_band_result* results, double* ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if ((ir_left == nullptr) != (ir_right == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ir_left and ir_right: both or neither");
    if (r->fif != 1) return fail(ARX_ERR_INVALID_ARGUMENT, "a band render needs one frame in flight");
    if (r->stream != r->cur().stream) return fail(ARX_ERR_INVALID_ARGUMENT, "a band render needs the renderer's own stream");
    if (r->d_hist_ext) return fail(ARX_ERR_INVALID_ARGUMENT, "a band render needs the renderer's own histogram");
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    BandState& bs = r->bands;
    if (bs.n_bands < 1) return fail(ARX_ERR_NOT_READY, "arx_set_band_absorption has not been called for this scene");
    if (const arx_status dst = directivity_check_bands(r, bs.n_bands); dst != ARX_OK) return dst;
    if (const arx_status ast = air_check_bands(r, bs.n_bands); ast != ARX_OK) return ast;
    PathCache& pc = r->path_cache;
    if (pc.mode != 1) return fail(ARX_ERR_NOT_READY, "a band render replays the path cache, which is off");
    const uint64_t N = n_rays(r->cfg);
    if (N == 0) return fail(ARX_ERR_NOT_READY, "a launch of no rays is not cacheable");
    ARX_HIP(hipSetDevice(r->cfg.device));
    const int32_t B = bs.n_bands;
    const size_t ir_len = (size_t)r->ir_len;
    const bool timed = ms != nullptr;  // around the whole call, its warm launches included
    arx_status st;
    if (timed && (st = bs.timer.begin(r->stream)) != ARX_OK) return st;
    // 1. the recording: ordinary launches of the current settings until the cache holds the key's records
    ReplayProbe probe;
    int32_t warm = 0;
    if ((st = record_for_bands(r, N, nullptr, &probe, &warm)) != ARX_OK) return st;
    // 2. the scratch and the pinned block of the host-side outputs
    if ((st = bs.h_pinned.reserve(kMaxBands * (kBandCounterWords * 8 + 3 * sizeof(arx_acoustics)))) != ARX_OK) return st;
    unsigned long long* h_cnt = reinterpret_cast<unsigned long long*>(bs.h_pinned.p);
    arx_acoustics* h_res = reinterpret_cast<arx_acoustics*>(h_cnt + kMaxBands * kBandCounterWords);
    const BandScratchLayout sc = band_scratch_layout(r->ir_len, B);
    bs.hist_bands = 0;
    if ((st = bs.d_scratch.reserve(sc.total)) != ARX_OK) return st;
    char* const base = bs.d_scratch.p;
    unsigned long long* d_hist = reinterpret_cast<unsigned long long*>(base + sc.hist);
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(base + sc.counters);
    arx_acoustics* d_res = reinterpret_cast<arx_acoustics*>(base + sc.res);
    float* d_irl = reinterpret_cast<float*>(base + sc.ir);
    float* d_irr = d_irl + (size_t)B * ir_len;
    // 3. one walk for every band, then each band's finalize and analysis
    BandArgs ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.table = bs.d_table.p;
    ba.hist = d_hist;
    ba.counters = d_cnt;
    ba.n_tris = bs.n_tris;
    ba.n_bands = B;
    // a source pattern: the gain plane of this recording (remade only when stale), and the directed replay
    if ((st = directivity_plane(r, probe.args.dirs, N, B, &ba.gain)) != ARX_OK) return st;
    // air absorption: the attenuation table (remade only when stale), and the replay that weights its deposits
    if ((st = air_table(r, B, &ba.air)) != ARX_OK) return st;
    ARX_HIP(launch_band_replay(probe.args, ba, r->stream));
    for (size_t b = 0; b < (size_t)B; ++b)
        if ((st = finalize_and_analyse(r, d_hist + b * 2 * ir_len, d_irl + b * ir_len, d_irr + b * ir_len, d_res + 3 * b,
                                       base + sc.edc, base + sc.acou, ir_left != nullptr, acoustics != nullptr)) != ARX_OK)
            return st;
    if (ir_left) {
        ARX_HIP(hipMemcpyAsync(ir_left, d_irl, (size_t)B * ir_len * sizeof(float), hipMemcpyDefault, r->stream));
        ARX_HIP(hipMemcpyAsync(ir_right, d_irr, (size_t)B * ir_len * sizeof(float), hipMemcpyDefault, r->stream));
    }
    ARX_HIP(hipMemcpyAsync(h_cnt, d_cnt, (size_t)B * kBandCounterWords * 8, hipMemcpyDeviceToHost, r->stream));
    if (acoustics)
        ARX_HIP(hipMemcpyAsync(h_res, d_res, (size_t)B * 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost, r->stream));
    // the tree as the probe's refit left it (a listener move): its off-grid flag, as arx_get_stats reads it
    ARX_HIP(hipMemcpyAsync(r->h_tree_flag.p, r->d_tree_flag.p, sizeof(unsigned int), hipMemcpyDeviceToHost, r->stream));
    if (timed && (st = bs.timer.end(r->stream)) != ARX_OK) return st;
    // 4. the one synchronisation, then the host-side outputs
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (r->tree_gen != 0 && *r->h_tree_flag.p == r->tree_gen)
        return fail(ARX_ERR_INTERNAL, "receiver refit / re-quantization: a box left the quantization grid");
    bs.hist_bands = B;
    bs.hist_ir_len = r->ir_len;
    for (int32_t b = 0; b < B; ++b) {
        if (results) {
            arx_band_result& o = results[b];
            std::memset(&o, 0, sizeof(o));
            o.queries = h_cnt[b * kBandCounterWords + 0];
            o.receiver_hits = h_cnt[b * kBandCounterWords + 1];
            o.misses = h_cnt[b * kBandCounterWords + 2];
            o.warm_launches = warm;
        }
    }
    if (acoustics) std::memcpy(acoustics, h_res, (size_t)B * 3 * sizeof(arx_acoustics));
    return timed ? bs.timer.elapsed(ms) : ARX_OK;
}

int32_t arx_band_count(const arx_renderer* r) { return r ? r->bands.n_bands : 0; }

arx_status arx_debug_band_histograms(arx_renderer* r, int64_t* h_out, size_t capacity) {
    if (!r || !h_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    const BandState& bs = r->bands;
    if (bs.hist_bands < 1 || !bs.d_scratch.p) return fail(ARX_ERR_NOT_READY, "no arx_render_bands call has finished yet");
    const size_t words = (size_t)bs.hist_bands * 2 * (size_t)bs.hist_ir_len;
    if (capacity < words) return fail(ARX_ERR_INVALID_ARGUMENT, "the histograms hold %zu words", words);
    ARX_HIP(hipSetDevice(r->cfg.device));
    // the last call ended synchronised; its histograms lead the scratch (band_scratch_layout)
    ARX_HIP(hipMemcpy(h_out, bs.d_scratch.p + band_scratch_layout(bs.hist_ir_len, bs.hist_bands).hist,
                      words * sizeof(int64_t), hipMemcpyDeviceToHost));
    return ARX_OK;
}

uint64_t arx_debug_band_bytes(int32_t ir_len, int64_t n_tris, int32_t n_bands) {
    if (ir_len < 0 || n_tris < 0 || n_bands < 1 || n_bands > kMaxBands) return 0;
    return band_table_bytes(n_tris, n_bands) + band_scratch_layout(ir_len, n_bands).total;
}

// ---- band synthesis (arx_band_synth.hip) ------------------------------------------------------------

arx_status arx_band_filters(int32_t sample_rate, const double* crossovers_hz, int32_t n_bands, int32_t taps, double* g) {
    if (!g) return fail(ARX_ERR_INVALID_ARGUMENT, "g is NULL");
    if (n_bands < 1 || n_bands > kMaxBands) return fail(ARX_ERR_INVALID_ARGUMENT, "n_bands %d: 1..%d", n_bands, kMaxBands);
    if (!synth_taps_ok(taps)) return fail(ARX_ERR_INVALID_ARGUMENT, "taps %d: odd, 1..%d", taps, ARX_BAND_TAPS_MAX);
    if (sample_rate <= 0) return fail(ARX_ERR_INVALID_ARGUMENT, "sample rate %d: must be positive", sample_rate);
    if (n_bands > 1 && !crossovers_hz) return fail(ARX_ERR_INVALID_ARGUMENT, "crossovers_hz is NULL");
    for (int32_t i = 0; i + 1 < n_bands; ++i) {
        const double x = crossovers_hz[i];
        if (!std::isfinite(x) || x <= 0.0 || x >= 0.5 * (double)sample_rate || (i > 0 && !(x > crossovers_hz[i - 1])))
            return fail(ARX_ERR_INVALID_ARGUMENT,
                        "crossover %d (%g Hz): finite, positive, strictly ascending and below sample_rate / 2 = %g", i, x,
                        0.5 * (double)sample_rate);
    }
    int64_t N = 1;
    while (N < 4 * (int64_t)taps) N *= 2;
    const int64_t H = N / 2, c = (taps - 1) / 2;
    const double pi = 3.14159265358979323846;
    std::vector<double> ct((size_t)N);  // cos(2 pi r / N)
    for (int64_t r = 0; r < N; ++r) ct[(size_t)r] = std::cos(2.0 * pi * (double)r / (double)N);
    // L_i on the grid, i = -1 .. n_bands-1, two rows at a time: G_b = L_b - L_(b-1), times w_m
    std::vector<double> lo((size_t)H + 1, 0.0), hi((size_t)H + 1), G((size_t)H + 1);
    std::vector<int64_t> support;
    for (int32_t b = 0; b < n_bands; ++b) {
        for (int64_t m = 0; m <= H; ++m) {
            double L = 1.0;
            if (b + 1 < n_bands && m > 0) {
                const double u = std::log2((double)m * (double)sample_rate / (double)N / crossovers_hz[b]);
                L = u <= -0.5 ? 1.0 : u >= 0.5 ? 0.0 : 0.5 * (1.0 - std::sin(pi * u));
            }
            hi[(size_t)m] = L;
            G[(size_t)m] = ((m == 0 || m == H) ? 1.0 : 2.0) * (L - lo[(size_t)m]);
        }
        support.clear();  // outside the band G is zero, and a zero term leaves the sum as it is
        for (int64_t m = 0; m <= H; ++m)
            if (G[(size_t)m] != 0.0) support.push_back(m);
        double* const gb = g + (size_t)b * (size_t)taps;
        for (int64_t j = 0; j <= c; ++j) {
            double sum = 0.0;
            for (const int64_t m : support) sum += G[(size_t)m] * ct[(size_t)((m * j) & (N - 1))];
            const double win = 0.5 * (1.0 + std::cos(pi * (double)j / (double)(c + 1)));
            const double v = sum / (double)N * win;
            gb[c + j] = v;
            gb[c - j] = v;
        }
        lo.swap(hi);
    }
    return ARX_OK;
}

arx_status arx_combine_bands(arx_renderer* r, const float* ir_left, const float* ir_right, int32_t n_bands, size_t ir_len,
                             const double* filters, int32_t taps, float* out_left, float* out_right, double* ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (!ir_left || !ir_right || !filters || !out_left || !out_right) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_bands < 1 || n_bands > kMaxBands) return fail(ARX_ERR_INVALID_ARGUMENT, "n_bands %d: 1..%d", n_bands, kMaxBands);
    if (!synth_taps_ok(taps)) return fail(ARX_ERR_INVALID_ARGUMENT, "taps %d: odd, 1..%d", taps, ARX_BAND_TAPS_MAX);
    if (ir_len == 0 || ir_len > (size_t)INT32_MAX) return fail(ARX_ERR_INVALID_ARGUMENT, "ir_len %zu: 1..%d", ir_len, INT32_MAX);
    if (r->stream != r->cur().stream) return fail(ARX_ERR_INVALID_ARGUMENT, "a band combine needs the renderer's own stream");
    const SynthLayout lay = synth_layout(ir_len, n_bands, taps);
    SynthScratch& sc = r->synth;
    ARX_HIP(hipSetDevice(r->cfg.device));
    if (const arx_status wt = fif_wait_conv(r); wt != ARX_OK) return wt;
    // nothing of an earlier call is in flight: every call ends synchronised
    if (const arx_status rs = sc.d_scratch.reserve(lay.total); rs != ARX_OK) return rs;
    char* const base = sc.d_scratch.p;
    const bool timed = r->timing || ms != nullptr;
    if (timed)
        if (const arx_status tb = sc.timer.begin(r->stream); tb != ARX_OK) return tb;
    BandSynthArgs a{};
    a.ir_left = reinterpret_cast<const float*>(base + lay.in_left);
    a.ir_right = reinterpret_cast<const float*>(base + lay.in_right);
    a.filters = reinterpret_cast<const double*>(base + lay.filters);
    a.out_left = reinterpret_cast<float*>(base + lay.out_left);
    a.out_right = reinterpret_cast<float*>(base + lay.out_right);
    a.ir_len = (int64_t)ir_len;
    a.n_bands = n_bands;
    a.taps = taps;
    const size_t in_bytes = (size_t)n_bands * ir_len * sizeof(float), out_bytes = ir_len * sizeof(float);
    ARX_HIP(hipMemcpyAsync(base + lay.in_left, ir_left, in_bytes, hipMemcpyDefault, r->stream));
    ARX_HIP(hipMemcpyAsync(base + lay.in_right, ir_right, in_bytes, hipMemcpyDefault, r->stream));
    ARX_HIP(hipMemcpyAsync(base + lay.filters, filters, (size_t)n_bands * (size_t)taps * sizeof(double), hipMemcpyDefault,
                           r->stream));
    ARX_HIP(launch_band_synth(a, r->stream));
    ARX_HIP(hipMemcpyAsync(out_left, base + lay.out_left, out_bytes, hipMemcpyDefault, r->stream));
    ARX_HIP(hipMemcpyAsync(out_right, base + lay.out_right, out_bytes, hipMemcpyDefault, r->stream));
    if (timed)
        if (const arx_status te = sc.timer.end(r->stream); te != ARX_OK) return te;
    if (const arx_status d = fif_done_conv(r); d != ARX_OK) return d;
    ARX_HIP(hipStreamSynchronize(r->stream));
    return ms ? sc.timer.elapsed(ms) : ARX_OK;
}

uint64_t arx_debug_combine_bytes(size_t ir_len, int32_t n_bands, int32_t taps) {
    if (ir_len == 0 || ir_len > (size_t)INT32_MAX || n_bands < 1 || n_bands > kMaxBands || !synth_taps_ok(taps)) return 0;
    return synth_layout(ir_len, n_bands, taps).total;
}

}  // extern "C"
