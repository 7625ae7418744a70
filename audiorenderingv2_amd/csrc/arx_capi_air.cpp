// arx_capi_air.cpp -- air absorption behind the C ABI (include/arx.h): the coefficients (dB per metre per band)
// and their rule, the attenuation table's host definition (arx_air_attenuation_host, the one loop the device
// table is uploaded from), ISO 9613-1's pure-tone formula, and the device table with the generation word that
// says when it must be remade.  The kernels that read it are the band replays' AIR instantiations
// (band_shade, arx_replay.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "arx_bands.hpp"
#include "arx_internal.hpp"

using namespace arx;

namespace {

constexpr double kNeperPerDb = 0.23025850929940458;  // ln(10) / 10: dB of energy to the exponent

// The rule for coefficients: 1..kMaxBands of them, each finite and >= 0 (false for a NaN).
arx_status check_alpha(const double* alpha, int32_t n) {
    if (n < 1 || n > kMaxBands) return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: n %d: 1..%d", n, kMaxBands);
    if (!alpha) return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: alpha_db_per_m is NULL");
    for (int32_t b = 0; b < n; ++b)
        if (!(std::isfinite(alpha[b]) && alpha[b] >= 0.0))
            return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: band %d: %.17g dB/m is not finite and >= 0", b, alpha[b]);
    return ARX_OK;
}

// The table's definition (include/arx.h), arguments checked by the caller: out[k * width + b].
void fill_table(const double* alpha, int32_t n, int32_t sample_rate, int32_t ir_len, int32_t width, float* out) {
    const int32_t filled = n == 1 ? width : n;  // one coefficient serves every band
    for (int64_t k = 0; k < (int64_t)ir_len; ++k) {
        const double d = ((double)k * (double)kSpeedOfSound) / (double)sample_rate;
        float* row = out + k * width;
        for (int32_t b = 0; b < width; ++b)
            row[b] = b < filled ? (float)std::exp(-((alpha[n == 1 ? 0 : b] * kNeperPerDb) * d)) : 0.0f;
    }
}

}  // namespace

arx_status arx::air_check_bands(const arx_renderer* r, int32_t n_bands) {
    const int32_t n = r->air.n;
    if (n > 1 && n != n_bands)
        return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption has %d coefficients and the band table %d bands: one, or as many", n, n_bands);
    return ARX_OK;
}

arx_status arx::air_table(arx_renderer* r, int32_t n_bands, const float** table) {
    AirState& a = r->air;
    *table = nullptr;
    if (a.n < 1) return ARX_OK;
    if (const arx_status st = air_check_bands(r, n_bands); st != ARX_OK) return st;
    if (n_bands < 1 || n_bands > kMaxBands || r->ir_len < 1) return fail(ARX_ERR_INTERNAL, "air table: no bands or no bins");
    const int32_t W = band_width(n_bands);
    const uint64_t need = (uint64_t)r->ir_len * (uint64_t)W;  // floats
    if (need > a.d_table.cap) {
        a.table_valid = false;
        if (const arx_status st = a.d_table.reserve(need); st != ARX_OK) return st;
    }
    if (!a.table_valid || a.made_gen != a.gen || a.made_bands != n_bands) {
        a.table_valid = false;
        std::vector<float> rows((size_t)need);
        fill_table(a.alpha, a.n, r->cfg.sample_rate, r->ir_len, W, rows.data());
        // blocking: the rows are pageable, and no kernel that reads the old table is in flight
        ARX_HIP(hipMemcpy(a.d_table.p, rows.data(), need * sizeof(float), hipMemcpyHostToDevice));
        a.made_gen = a.gen;
        a.made_bands = n_bands;
        a.table_valid = true;
        ++a.tables_made;
    }
    *table = a.d_table.p;
    return ARX_OK;
}

extern "C" {

arx_status arx_set_air_absorption(arx_renderer* r, const double* alpha_db_per_m, int32_t n) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    AirState& a = r->air;
    if (n == 0) {
        if (a.n != 0) ++a.gen;
        a.n = 0;
        return ARX_OK;
    }
    if (const arx_status st = check_alpha(alpha_db_per_m, n); st != ARX_OK) return st;
    if (a.n != n || std::memcmp(a.alpha, alpha_db_per_m, (size_t)n * sizeof(double)) != 0) {
        std::memset(a.alpha, 0, sizeof(a.alpha));
        std::memcpy(a.alpha, alpha_db_per_m, (size_t)n * sizeof(double));
        a.n = n;
        ++a.gen;
    }
    return ARX_OK;
}

int32_t arx_air_absorption_bands(const arx_renderer* r) { return r ? r->air.n : 0; }

arx_status arx_air_attenuation_host(const double* alpha_db_per_m, int32_t n, int32_t sample_rate, int32_t ir_len,
                                    int32_t width, float* out) {
    if (const arx_status st = check_alpha(alpha_db_per_m, n); st != ARX_OK) return st;
    if (width != 4 && width != 8) return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: width %d: 4 or 8", width);
    if (n > width) return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: %d coefficients do not fit a row of %d", n, width);
    if (sample_rate <= 0) return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: sample rate %d: must be positive", sample_rate);
    if (ir_len <= 0) return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: ir_len %d: must be positive", ir_len);
    if (!out) return fail(ARX_ERR_INVALID_ARGUMENT, "air absorption: out is NULL");
    fill_table(alpha_db_per_m, n, sample_rate, ir_len, width, out);
    return ARX_OK;
}

arx_status arx_air_absorption_iso9613(double temperature_c, double relative_humidity_percent, double pressure_kpa,
                                      const double* freq_hz, int32_t n, double* alpha_db_per_m) {
    if (!(temperature_c >= -20.0 && temperature_c <= 50.0))  // a NaN fails each of these
        return fail(ARX_ERR_INVALID_ARGUMENT, "ISO 9613-1: temperature %g C: -20..50", temperature_c);
    if (!(relative_humidity_percent >= 0.0 && relative_humidity_percent <= 100.0))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ISO 9613-1: relative humidity %g %%: 0..100", relative_humidity_percent);
    if (!(pressure_kpa > 0.0 && pressure_kpa <= 200.0))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ISO 9613-1: pressure %g kPa: above 0, up to 200", pressure_kpa);
    if (n < 0 || (n > 0 && (!freq_hz || !alpha_db_per_m))) return fail(ARX_ERR_INVALID_ARGUMENT, "ISO 9613-1: bad frequency arguments");
    for (int32_t i = 0; i < n; ++i)
        if (!(std::isfinite(freq_hz[i]) && freq_hz[i] > 0.0))
            return fail(ARX_ERR_INVALID_ARGUMENT, "ISO 9613-1: frequency %d (%g Hz): finite and positive", i, freq_hz[i]);
    const double T = temperature_c + 273.15, T0 = 293.15, T01 = 273.16, pr = 101.325;
    const double p = pressure_kpa / pr;
    const double C = -6.8346 * std::pow(T01 / T, 1.261) + 4.6151;
    const double h = relative_humidity_percent * std::pow(10.0, C) / p;
    const double tr = T / T0;
    const double frO = p * (24.0 + 4.04e4 * h * (0.02 + h) / (0.391 + h));
    const double frN = p * std::pow(tr, -0.5) * (9.0 + 280.0 * h * std::exp(-4.170 * (std::pow(tr, -1.0 / 3.0) - 1.0)));
    for (int32_t i = 0; i < n; ++i) {
        const double f2 = freq_hz[i] * freq_hz[i];
        alpha_db_per_m[i] = 8.686 * f2 *
                            (1.84e-11 / p * std::pow(tr, 0.5) +
                             std::pow(tr, -2.5) * (0.01275 * std::exp(-2239.1 / T) / (frO + f2 / frO) +
                                                   0.1068 * std::exp(-3352.0 / T) / (frN + f2 / frN)));
    }
    return ARX_OK;
}

arx_status arx_debug_air_table(arx_renderer* r, int64_t first_bin, int64_t count, float* h_out) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (count > 0 && !h_out) return fail(ARX_ERR_INVALID_ARGUMENT, "NULL output");
    if (r->air.n < 1) return fail(ARX_ERR_NOT_READY, "arx_set_air_absorption has not been called");
    // the band count the next band call will run with: the table's, or without a table the coefficients'.
    // The table depends on no recording, so none is needed.
    const int32_t B = r->bands.n_bands >= 1 ? r->bands.n_bands : r->air.n;
    if (const arx_status st = air_check_bands(r, B); st != ARX_OK) return st;
    if (first_bin < 0 || count < 0 || first_bin > (int64_t)r->ir_len || count > (int64_t)r->ir_len - first_bin)
        return fail(ARX_ERR_INVALID_ARGUMENT, "the table holds %d bins", r->ir_len);
    ARX_HIP(hipSetDevice(r->cfg.device));
    const float* table = nullptr;
    if (const arx_status st = air_table(r, B, &table); st != ARX_OK) return st;
    const uint64_t W = (uint64_t)band_width(B);
    if (count > 0)
        ARX_HIP(hipMemcpy(h_out, table + (uint64_t)first_bin * W, (uint64_t)count * W * sizeof(float), hipMemcpyDeviceToHost));
    return ARX_OK;
}

uint64_t arx_debug_air_bytes(int32_t ir_len, int32_t n_bands) {
    if (ir_len < 0 || n_bands < 1 || n_bands > kMaxBands) return 0;
    return (uint64_t)ir_len * (uint64_t)band_width(n_bands) * sizeof(float);
}

uint64_t arx_debug_air_tables_made(const arx_renderer* r) { return r ? r->air.tables_made : 0; }

}  // extern "C"
