// arx_capi_bands.cpp -- frequency-band absorption behind the C ABI (include/arx.h): the band table and
// its rule, and arx_render_bands -- every band's frame from one walk over the path cache's records
// (band_replay_kernel, arx_replay.hip), each finalized and analysed as arx_render and arx_analyze_ir do it.
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

}  // namespace

BandScratchLayout arx::band_scratch_layout(int32_t ir_len, int32_t n_bands) {
    BandScratchLayout s;
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 15) & ~15ull;
        return o;
    };
    const uint64_t B = (uint64_t)n_bands, L = (uint64_t)ir_len;
    s.hist = take(B * 16 * L);
    s.counters = take(B * kBandCounterWords * 8);
    s.res = take(B * 3 * sizeof(arx_acoustics));
    s.ir = take(B * 8 * L);  // the bands' left IRs, then their right IRs
    s.edc = take(24 * L);
    s.acou = take(acoustics_scratch_bytes());
    s.total = at;
    return s;
}

void arx::free_bands(BandState& b) {
    hipFree(b.d_table);
    hipFree(b.d_scratch);
    if (b.h_pinned) hipHostFree(b.h_pinned);
    if (b.ev0) hipEventDestroy(b.ev0);
    if (b.ev1) hipEventDestroy(b.ev1);
    b = BandState{};
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
    const uint64_t need = band_table_bytes(n_tris, n_bands);
    if (need > bs.table_cap) {  // no call is in flight: every arx_render_bands ends synchronised
        hipFree(bs.d_table);
        bs.d_table = nullptr;
        bs.table_cap = 0;
        ARX_HIP(hipMalloc(&bs.d_table, need));
        bs.table_cap = need;
    }
    ARX_HIP(hipMemcpy(bs.d_table, rows.data(), need, hipMemcpyHostToDevice));
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
    PathCache& pc = r->path_cache;
    if (pc.mode != 1) return fail(ARX_ERR_NOT_READY, "a band render replays the path cache, which is off");
    const uint64_t N = n_rays(r->cfg);
    if (N == 0) return fail(ARX_ERR_NOT_READY, "a launch of no rays is not cacheable");
    ARX_HIP(hipSetDevice(r->cfg.device));
    const int32_t B = bs.n_bands;
    const size_t ir_len = (size_t)r->ir_len;
    const bool timed = ms != nullptr;  // around the whole call, its warm launches included
    if (timed) {
        if (!bs.ev0) ARX_HIP(hipEventCreate(&bs.ev0));
        if (!bs.ev1) ARX_HIP(hipEventCreate(&bs.ev1));
        ARX_HIP(hipEventRecord(bs.ev0, r->stream));
    }
    // 1. the recording: ordinary launches of the current settings until the cache holds the key's records
    ReplayProbe probe;
    int32_t warm = 0;
    arx_status st;
    for (;;) {
        if ((st = trace_rays(r, 0, N, false, false, &probe)) != ARX_OK) return st;
        if (probe.recorded) break;
        const int32_t would = probe.state;  // what the next launch would do
        if (would == kPathOff) return fail(ARX_ERR_NOT_READY, "a band render replays the path cache, which is off");
        if (would == kPathNotCacheable)
            return fail(ARX_ERR_NOT_READY, "this launch is not cacheable (global stack, CW4 or f32 nodes): no records to replay");
        if (would == kPathOverCap)
            return fail(ARX_ERR_NOT_READY,
                        "the launch's records (%llu B) are over the path cache's cap or do not fit on the device "
                        "(arx_debug_set_path_cache max_bytes)",
                        (unsigned long long)arx_debug_path_cache_bytes(N, r->cfg.max_bounces));
        if (warm == 3) return fail(ARX_ERR_NOT_READY, "the path cache did not record within three launches");
        if ((st = arx_render(r, nullptr)) != ARX_OK) return st;
        ++warm;
    }
    // 2. the scratch and the pinned block of the host-side outputs
    if (!bs.h_pinned)
        ARX_HIP(hipHostMalloc(&bs.h_pinned, kMaxBands * (kBandCounterWords * 8 + 3 * sizeof(arx_acoustics)),
                              hipHostMallocDefault));
    unsigned long long* h_cnt = static_cast<unsigned long long*>(bs.h_pinned);
    arx_acoustics* h_res = reinterpret_cast<arx_acoustics*>(h_cnt + kMaxBands * kBandCounterWords);
    const BandScratchLayout sc = band_scratch_layout(r->ir_len, B);
    if (sc.total > bs.scratch_cap) {
        hipFree(bs.d_scratch);
        bs.d_scratch = nullptr;
        bs.scratch_cap = 0;
        ARX_HIP(hipMalloc(&bs.d_scratch, sc.total));
        bs.scratch_cap = sc.total;
    }
    char* const base = static_cast<char*>(bs.d_scratch);
    unsigned long long* d_hist = reinterpret_cast<unsigned long long*>(base + sc.hist);
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(base + sc.counters);
    arx_acoustics* d_res = reinterpret_cast<arx_acoustics*>(base + sc.res);
    float* d_irl = reinterpret_cast<float*>(base + sc.ir);
    float* d_irr = d_irl + (size_t)B * ir_len;
    // 3. one walk for every band, then each band's finalize and analysis
    BandArgs ba;
    std::memset(&ba, 0, sizeof(ba));
    ba.table = bs.d_table;
    ba.hist = d_hist;
    ba.counters = d_cnt;
    ba.n_tris = bs.n_tris;
    ba.n_bands = B;
    ARX_HIP(launch_band_replay(probe.args, ba, r->stream));
    const double unit = std::ldexp((double)initial_energy(r->cfg), -arx_frac_bits(N));
    for (int32_t b = 0; b < B; ++b) {
        const long long* h = reinterpret_cast<const long long*>(d_hist + (size_t)b * 2 * ir_len);
        if (ir_left)
            ARX_HIP(launch_finalize_ir(h, d_irl + (size_t)b * ir_len, d_irr + (size_t)b * ir_len, r->ir_len, unit,
                                       r->cfg.is_mono, r->stream));
        if (acoustics) {
            AcousticsArgs args{};
            args.hist = h;
            args.n = r->ir_len;
            args.sample_rate = r->cfg.sample_rate;
            args.unit = unit;
            args.edc = reinterpret_cast<long long*>(base + sc.edc);
            args.out = d_res + 3 * b;
            args.scratch = base + sc.acou;
            args.shape = r->scan_shape == 0 ? kScanDefault : r->scan_shape;
            ARX_HIP(launch_acoustics(args, r->stream));
        }
    }
    if (ir_left) {
        ARX_HIP(hipMemcpyAsync(ir_left, d_irl, (size_t)B * ir_len * sizeof(float), hipMemcpyDefault, r->stream));
        ARX_HIP(hipMemcpyAsync(ir_right, d_irr, (size_t)B * ir_len * sizeof(float), hipMemcpyDefault, r->stream));
    }
    ARX_HIP(hipMemcpyAsync(h_cnt, d_cnt, (size_t)B * kBandCounterWords * 8, hipMemcpyDeviceToHost, r->stream));
    if (acoustics)
        ARX_HIP(hipMemcpyAsync(h_res, d_res, (size_t)B * 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost, r->stream));
    // the tree as the probe's refit left it (a listener move): its off-grid flag, as arx_get_stats reads it
    ARX_HIP(hipMemcpyAsync(r->h_tree_flag, r->d_tree_flag, sizeof(unsigned int), hipMemcpyDeviceToHost, r->stream));
    if (timed) ARX_HIP(hipEventRecord(bs.ev1, r->stream));
    // 4. the one synchronisation, then the host-side outputs
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (r->tree_gen != 0 && *r->h_tree_flag == r->tree_gen)
        return fail(ARX_ERR_INTERNAL, "receiver refit / re-quantization: a box left the quantization grid");
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
    if (timed) {
        float t = 0.0f;
        ARX_HIP(hipEventElapsedTime(&t, bs.ev0, bs.ev1));
        *ms = (double)t;
    }
    return ARX_OK;
}

int32_t arx_band_count(const arx_renderer* r) { return r ? r->bands.n_bands : 0; }

uint64_t arx_debug_band_bytes(int32_t ir_len, int64_t n_tris, int32_t n_bands) {
    if (ir_len < 0 || n_tris < 0 || n_bands < 1 || n_bands > kMaxBands) return 0;
    return band_table_bytes(n_tris, n_bands) + band_scratch_layout(ir_len, n_bands).total;
}

}  // extern "C"
