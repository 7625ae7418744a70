// arx_acoustics.hip -- room-acoustic parameters of the traced histogram (ISO 3382-1: Schroeder's
// energy decay curve, EDT, T20, T30, C50, C80, D50, Ts), on the device behind a frame's IR finalize
// and, with the same definitions in plain C++, on the host (arx_acoustics_from_histogram).
//
// No reference counterpart: the reference only ever convolves its IR.  The definitions are
// include/arx.h's (arx_acoustics); this file holds
//   * the reverse inclusive scan E[k] = sum_{j >= k} h[j] of three channels (L, R, L + R formed on the
//     fly) in int64 -- exact, so the curve is as independent of the GPU count as the histogram -- in
//     two shapes (launch_acoustics: one workgroup per channel, or a tiled two-launch scan);
//   * the statistics: E never rises, so every level bin is a count of a monotone predicate, found by
//     a two-level sampled search; the three line fits share one pass over E (one log10 per bin) with
//     a fixed reduction order (strided partials per lane, an LDS tree per tile, the tiles in index
//     order), so the same histogram gives the same bits on every run; Ts sums E in two 64-bit limbs;
//   * the arithmetic from those counts and sums to the results, shared by the device and the host.
// No kernel here waits for another workgroup: what one launch needs from all of another is handed
// over at the launch boundary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/arx.h"
#include "arx_internal.hpp"
#include "arx_kernels.hpp"

namespace arx {
namespace {

__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

constexpr int kScanLanes = 1024;  // one-workgroup scan
constexpr int kTileLanes = 256;   // tiled scan: lanes per tile
constexpr int kMaxTiles = 1024;   // tiled scan: tiles per channel
constexpr int kFitLanes = 256;
constexpr int kFitTiles = 32;     // fit partials per channel (their order is the reduction order)
constexpr int kPreds = 6;

// ---- the definitions, shared by host and device ----------------------------------------------

struct Levels {
    long long total;
    double t5, t10, t25, t35;  // (double)E[0] * Cx
};

__host__ __device__ inline Levels make_levels(long long total) {
    Levels l;
    l.total = total;
    const double d = (double)total;
    l.t5 = d * ARX_ACOUSTICS_C5;
    l.t10 = d * ARX_ACOUSTICS_C10;
    l.t25 = d * ARX_ACOUSTICS_C25;
    l.t35 = d * ARX_ACOUSTICS_C35;
    return l;
}

// Six predicates that hold on a prefix of the bins (E never rises, and neither does (double)E):
// E == total (up to the onset), E > 0 (up to the last bin), not yet at or below -5 dB, at or above
// -10 / -25 / -35 dB.  The count of bins each holds on gives the bin.
__host__ __device__ inline bool level_pred(int p, long long e, const Levels& l) {
    const double d = (double)e;
    switch (p) {
        case 0: return e == l.total;
        case 1: return e > 0;
        case 2: return !(d <= l.t5);
        case 3: return d >= l.t10;
        case 4: return d >= l.t25;
        default: return d >= l.t35;
    }
}

struct Ranges {
    int32_t onset, last;
    int32_t a[3], b[3];  // EDT, T20, T30 (inclusive; -1, -1: no such bins)
    bool ok[3];          // b - a >= 1
};

__host__ __device__ inline Ranges make_ranges(const int32_t* cnt, int32_t n) {
    Ranges r;
    r.onset = cnt[0] - 1;
    r.last = cnt[1] - 1;
    const int32_t a5 = cnt[2] > r.onset ? cnt[2] : r.onset;  // first bin >= onset at or below -5 dB
    const bool has5 = a5 < n;
    for (int f = 0; f < 3; ++f) {
        const int32_t top = cnt[3 + f] - 1;  // last bin at or above the level
        const int32_t b = top < r.last ? top : r.last;
        if (f == 0) {
            r.a[f] = r.onset;
            r.b[f] = b;
        } else {
            r.a[f] = has5 ? a5 : -1;
            r.b[f] = has5 ? b : -1;
        }
        r.ok[f] = r.a[f] >= 0 && (int64_t)r.b[f] - (int64_t)r.a[f] >= 1;
    }
    return r;
}

__host__ __device__ inline double fit_mid(const Ranges& r, int f) { return ((double)r.a[f] + (double)r.b[f]) * 0.5; }

// log10 for the levels, one statement for the host and the device: libm's and the device library's log10 are
// both within an ulp and not the same function, so a result that is to be the same bytes on both sides cannot go
// through them.  IEEE f64 add, mul and div only, in the order written, never contracted: x = m * 2^k with m in
// [sqrt(1/2), sqrt(2)), f = m - 1, s = f / (2 + f), ln(m) = f - f^2/2 + s (f^2/2 + R(s^2)) with the classic
// degree-7 minimax R, then times 1 / ln(10): the logarithm within 1 ulp and one more rounded product, so within
// 2 ulp (tests/test_log10_host.py holds it to numpy's over the analysis' argument range).  Every argument here
// is a ratio of two positive int64, a normal number; anything else (zero, negative, subnormal, inf, NaN) goes
// to the library's log10.
__host__ __device__ inline double log10_shared(double x) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, x);
    const int ex = (int)((bits >> 52) & 0x7ffu);
    if ((bits >> 63) != 0 || ex == 0 || ex == 0x7ff) return log10(x);
    int k = ex - 1023;
    double m = __builtin_bit_cast(double, (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull);  // [1, 2)
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        ++k;
    }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s, w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 +
                           w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double R = t2 + t1;
    const double hfsq = (0.5 * f) * f;
    const double dk = (double)k;
    const double ln = dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
    return ln * 4.34294481903251816668e-01;
}

__host__ __device__ inline double level_db(long long e, double dtotal) { return 10.0 * log10_shared((double)e / dtotal); }

__host__ __device__ inline void acoustics_empty(arx_acoustics* o, double unit) {
    const double nan = __builtin_nan("");
    o->total = 0;
    o->unit = unit;
    o->edt_s = o->t20_s = o->t30_s = o->c50_db = o->c80_db = o->d50 = o->ts_s = nan;
    o->onset_bin = o->last_bin = -1;
    for (int i = 0; i < 2; ++i) o->edt_bins[i] = o->t20_bins[i] = o->t30_bins[i] = -1;
    o->valid = 0;
    o->reserved = 0;
}

__host__ __device__ inline int32_t window_bins(int32_t ms, int32_t sample_rate) {
    return (int32_t)(((int64_t)ms * sample_rate + 500) / 1000);
}

// From the ranges, the fits' sums of x*y, the two-limb sum of E over the bins after the onset and
// the decay curve at the two window ends (late energy; 0 past the end) to the results.
__host__ __device__ inline void acoustics_finish(arx_acoustics* o, long long total, int32_t sample_rate, double unit,
                                                 const Ranges& r, const double* sxy, unsigned long long ts_hi,
                                                 unsigned long long ts_lo, long long late50, long long late80) {
    acoustics_empty(o, unit);
    if (total <= 0) return;
    const double dtotal = (double)total, sr = (double)sample_rate;
    o->total = total;
    o->onset_bin = r.onset;
    o->last_bin = r.last;
    int32_t* bins[3] = {o->edt_bins, o->t20_bins, o->t30_bins};
    double* times[3] = {&o->edt_s, &o->t20_s, &o->t30_s};
    uint32_t valid = 0;
    for (int f = 0; f < 3; ++f) {
        bins[f][0] = r.a[f];
        bins[f][1] = r.b[f];
        if (!r.ok[f]) continue;
        const double m = (double)((int64_t)r.b[f] - (int64_t)r.a[f] + 1);
        const double sxx = m * (m * m - 1.0) / 12.0;  // sum of (k - mid)^2 over m consecutive bins
        const double slope = sxy[f] / sxx;            // dB per bin
        if (slope < 0.0) {
            *times[f] = -60.0 / (slope * sr);
            valid |= 1u << f;
        }
    }
    const long long late[2] = {late50, late80};
    const int32_t wbins[2] = {window_bins(50, sample_rate), window_bins(80, sample_rate)};
    double* clarity[2] = {&o->c50_db, &o->c80_db};
    for (int w = 0; w < 2; ++w) {
        if (wbins[w] <= 0) continue;
        const long long early = total - late[w];  // E[onset] == total
        if (w == 0) {
            o->d50 = (double)early / dtotal;
            valid |= 1u << 5;
        }
        if (early > 0) {
            *clarity[w] = late[w] == 0 ? __builtin_inf() : 10.0 * log10_shared((double)early / (double)late[w]);
            valid |= 1u << (3 + w);
        }
    }
    const double num = (double)ts_hi * 18446744073709551616.0 + (double)ts_lo;
    o->ts_s = num / (dtotal * sr);
    valid |= 1u << 6;
    o->valid = valid;
}

// ---- device ------------------------------------------------------------------------------------

// Exclusive suffix sum over the block's lanes (the sum of v on every lane above this one) and the
// block total; s_w: one word per wave.  Two barriers.
__device__ __forceinline__ long long block_suffix_exclusive(long long v, long long* s_w, long long* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_down(inc, d, 64);
        if (lane + d < 64) inc += o;
    }
    if (lane == 0) s_w[w] = inc;
    __syncthreads();
    long long above = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const long long t = s_w[i];
        tot += t;
        if (i > w) above += t;
    }
    __syncthreads();
    *total = tot;
    return inc - v + above;
}

// Channel c of the histogram [L | R]: 0 left, 1 right, 2 their sum.
struct Channel {
    const long long* a;
    const long long* b;  // null unless c == 2
    __device__ __forceinline__ long long at(int64_t k) const { return b ? a[k] + b[k] : a[k]; }
};
__device__ __forceinline__ Channel channel_of(const long long* hist, int32_t n, int c) {
    return Channel{hist + (c == 1 ? n : 0), c == 2 ? hist + n : nullptr};
}

// Bins [k0, k1) of one lane: their sum, and the suffix sums written from the top down on top of
// `above`, the sum of every bin from k1 on.
__device__ __forceinline__ long long lane_sum(const Channel& ch, int64_t k0, int64_t k1) {
    long long s = 0;
#pragma unroll 4
    for (int64_t k = k0; k < k1; ++k) s += ch.at(k);
    return s;
}
__device__ __forceinline__ void lane_write(const Channel& ch, int64_t k0, int64_t k1, long long above, long long* e) {
    long long run = above;
#pragma unroll 4
    for (int64_t k = k1 - 1; k >= k0; --k) {
        run += ch.at(k);
        e[k] = run;
    }
}

// Shape 1: one workgroup of kScanLanes lanes per channel, each lane a contiguous chunk of bins; the
// chunk sums are scanned across the lanes, then every lane writes its chunk.  grid = 3.
__global__ __launch_bounds__(kScanLanes) void scan_wg_kernel(const long long* __restrict__ hist, int32_t n,
                                                             long long* __restrict__ edc) {
    __shared__ long long s_w[kScanLanes / 64];
    const int c = blockIdx.x;
    const Channel ch = channel_of(hist, n, c);
    const int64_t chunk = ((int64_t)n + kScanLanes - 1) / kScanLanes;
    const int64_t k0 = min64((int64_t)n, (int64_t)threadIdx.x * chunk), k1 = min64((int64_t)n, k0 + chunk);
    long long total;
    const long long above = block_suffix_exclusive(lane_sum(ch, k0, k1), s_w, &total);
    lane_write(ch, k0, k1, above, edc + (size_t)c * n);
}

// Shape 2: tiles of kTileLanes * epl bins (at most kMaxTiles per channel).  grid = (tiles, 3).
__device__ __forceinline__ void tile_range(int32_t n, int32_t epl, int64_t* k0, int64_t* k1) {
    const int64_t t0 = (int64_t)blockIdx.x * kTileLanes * epl;
    *k0 = min64((int64_t)n, t0 + (int64_t)threadIdx.x * epl);
    *k1 = min64((int64_t)n, *k0 + epl);
}
__global__ __launch_bounds__(kTileLanes) void tile_sum_kernel(const long long* __restrict__ hist, int32_t n, int32_t epl,
                                                              long long* __restrict__ tsum) {
    __shared__ long long s_w[kTileLanes / 64];
    const int c = blockIdx.y;
    int64_t k0, k1;
    tile_range(n, epl, &k0, &k1);
    long long total;
    block_suffix_exclusive(lane_sum(channel_of(hist, n, c), k0, k1), s_w, &total);
    if (threadIdx.x == 0) tsum[c * kMaxTiles + blockIdx.x] = total;
}
// Every tile adds up the sums of the tiles above it itself (at most kMaxTiles words, read by the whole
// block): no launch between the sums and the apply, and no workgroup waits for another.
__global__ __launch_bounds__(kTileLanes) void tile_apply_kernel(const long long* __restrict__ hist, int32_t n, int32_t epl,
                                                                const long long* __restrict__ tsum,
                                                                long long* __restrict__ edc) {
    __shared__ long long s_w[kTileLanes / 64];
    const int c = blockIdx.y, tiles = gridDim.x;
    const Channel ch = channel_of(hist, n, c);
    int64_t k0, k1;
    tile_range(n, epl, &k0, &k1);
    long long part = 0, carry, total;
    for (int t = blockIdx.x + 1 + threadIdx.x; t < tiles; t += kTileLanes) part += tsum[c * kMaxTiles + t];
    block_suffix_exclusive(part, s_w, &carry);
    const long long above = block_suffix_exclusive(lane_sum(ch, k0, k1), s_w, &total);
    lane_write(ch, k0, k1, above + carry, edc + (size_t)c * n);
}

// The six counts of level_pred over e[0, n), by the whole block: the block's lanes sample e every
// `step` bins, then count inside the one step where the predicate turns false.  s_cnt: 2 * kPreds
// words.  Every lane gets every count.
__device__ void block_level_counts(const long long* __restrict__ e, int32_t n, const Levels& lv, int32_t* s_cnt,
                                   int32_t* cnt) {
    const int nb = blockDim.x, t = threadIdx.x;
    const int64_t step = ((int64_t)n + nb - 1) / nb;
    if (t < 2 * kPreds) s_cnt[t] = 0;
    __syncthreads();
    const int64_t ks = (int64_t)t * step;
    if (ks < n) {
        const long long v = e[ks];
        for (int p = 0; p < kPreds; ++p)
            if (level_pred(p, v, lv)) atomicAdd(&s_cnt[p], 1);
    }
    __syncthreads();
    for (int p = 0; p < kPreds; ++p) {
        const int32_t c1 = s_cnt[p];  // samples 0 .. c1 - 1 hold, sample c1 does not
        if (c1 == 0) continue;
        const int64_t lo = (int64_t)(c1 - 1) * step + 1, hi = min64((int64_t)n, (int64_t)c1 * step);
        for (int64_t k = lo + t; k < hi; k += nb)
            if (level_pred(p, e[k], lv)) atomicAdd(&s_cnt[kPreds + p], 1);
    }
    __syncthreads();
    for (int p = 0; p < kPreds; ++p) {
        const int32_t c1 = s_cnt[p];
        cnt[p] = c1 == 0 ? 0 : (int32_t)((int64_t)(c1 - 1) * step + 1 + s_cnt[kPreds + p]);
    }
}

// Fit partials of tile blockIdx.x of channel blockIdx.y: the three fits' sums of x*y over the tile's
// bins and the two-limb sum of E over its bins after the onset.  Every block finds the level bins
// itself (two rounds of loads; cheaper than a launch of its own), tile 0 leaves them for the results
// kernel.  grid = (kFitTiles, 3).
__global__ __launch_bounds__(kFitLanes) void fit_partials_kernel(const long long* __restrict__ edc, int32_t n,
                                                                 double* __restrict__ part,
                                                                 unsigned long long* __restrict__ tspart,
                                                                 int32_t* __restrict__ counts) {
    __shared__ int32_t s_cnt[2 * kPreds];
    __shared__ double s_xy[3][kFitLanes];
    __shared__ unsigned long long s_ts[2][kFitLanes];
    const int c = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const long long* e = edc + (size_t)c * n;
    const long long total = e[0];
    double* out = part + ((size_t)c * kFitTiles + tile) * 3;
    unsigned long long* tout = tspart + ((size_t)c * kFitTiles + tile) * 2;
    if (total <= 0) {  // the same on every lane
        if (t < 3) out[t] = 0.0;
        if (t < 2) tout[t] = 0;
        return;
    }
    const Levels lv = make_levels(total);
    int32_t cnt[kPreds];
    block_level_counts(e, n, lv, s_cnt, cnt);
    if (tile == 0 && t < kPreds) counts[c * kPreds + t] = cnt[t];  // for the results kernel
    const Ranges r = make_ranges(cnt, n);
    const double mid[3] = {fit_mid(r, 0), fit_mid(r, 1), fit_mid(r, 2)};
    const double dtotal = (double)total;
    const int64_t tlen = ((int64_t)n + kFitTiles - 1) / kFitTiles;
    const int64_t k0 = min64((int64_t)n, (int64_t)tile * tlen), k1 = min64((int64_t)n, k0 + tlen);
    double s[3] = {0.0, 0.0, 0.0};
    unsigned long long lo = 0, hi = 0;
    for (int64_t k = k0 + t; k < k1; k += kFitLanes) {
        const long long v = e[k];
        if (k > r.onset) {
            lo += (unsigned long long)v;
            hi += lo < (unsigned long long)v;
        }
        bool in[3];
        for (int f = 0; f < 3; ++f) in[f] = r.ok[f] && k >= r.a[f] && k <= r.b[f];
        if ((in[0] || in[1] || in[2]) && v > 0) {
            const double y = level_db(v, dtotal);
            for (int f = 0; f < 3; ++f)
                if (in[f]) s[f] += ((double)k - mid[f]) * y;
        }
    }
    for (int f = 0; f < 3; ++f) s_xy[f][t] = s[f];
    s_ts[0][t] = lo;
    s_ts[1][t] = hi;
    for (int stride = kFitLanes / 2; stride > 0; stride >>= 1) {
        __syncthreads();
        if (t < stride) {
            for (int f = 0; f < 3; ++f) s_xy[f][t] += s_xy[f][t + stride];
            const unsigned long long l = s_ts[0][t] + s_ts[0][t + stride];
            s_ts[1][t] += s_ts[1][t + stride] + (l < s_ts[0][t]);
            s_ts[0][t] = l;
        }
    }
    if (t == 0) {
        for (int f = 0; f < 3; ++f) out[f] = s_xy[f][0];
        tout[0] = s_ts[0][0];
        tout[1] = s_ts[1][0];
    }
}

// The results of channel threadIdx.x (one lane each): the level bins as the fit kernel found them,
// the partials summed in tile order.  grid = 1, 64 lanes.
__global__ __launch_bounds__(64) void acoustics_final_kernel(const long long* __restrict__ edc, int32_t n,
                                                             int32_t sample_rate, double unit,
                                                             const double* __restrict__ part,
                                                             const unsigned long long* __restrict__ tspart,
                                                             const int32_t* __restrict__ counts,
                                                             arx_acoustics* __restrict__ res) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    const long long* e = edc + (size_t)c * n;
    const long long total = e[0];
    if (total <= 0) {
        acoustics_empty(res + c, unit);
        return;
    }
    int32_t cnt[kPreds];
    for (int p = 0; p < kPreds; ++p) cnt[p] = counts[c * kPreds + p];
    const Ranges r = make_ranges(cnt, n);
    double sxy[3] = {0.0, 0.0, 0.0};
    unsigned long long lo = 0, hi = 0;
    for (int tile = 0; tile < kFitTiles; ++tile) {
        const double* p = part + ((size_t)c * kFitTiles + tile) * 3;
        for (int f = 0; f < 3; ++f) sxy[f] += p[f];
        const unsigned long long* q = tspart + ((size_t)c * kFitTiles + tile) * 2;
        lo += q[0];
        hi += q[1] + (lo < q[0]);
    }
    long long late[2];
    const int32_t wms[2] = {50, 80};
    for (int w = 0; w < 2; ++w) {
        const int64_t k = (int64_t)r.onset + window_bins(wms[w], sample_rate);
        late[w] = k < n ? e[k] : 0;
    }
    acoustics_finish(res + c, total, sample_rate, unit, r, sxy, hi, lo, late[0], late[1]);
}

constexpr size_t kTsumBytes = 3 * (size_t)kMaxTiles * sizeof(long long);
constexpr size_t kPartBytes = 3 * (size_t)kFitTiles * 3 * sizeof(double);
constexpr size_t kTsPartBytes = 3 * (size_t)kFitTiles * 2 * sizeof(unsigned long long);
constexpr size_t kCountBytes = 3 * (size_t)kPreds * sizeof(int32_t);

}  // namespace

size_t acoustics_scratch_bytes() { return kTsumBytes + kPartBytes + kTsPartBytes + kCountBytes; }

hipError_t launch_acoustics(const AcousticsArgs& a, hipStream_t s) {
    if (!a.hist || !a.edc || !a.out || !a.scratch || a.n < 1 || a.sample_rate < 1) return hipErrorInvalidValue;
    (void)hipGetLastError();
    long long* tsum = (long long*)a.scratch;
    double* part = (double*)((char*)a.scratch + kTsumBytes);
    unsigned long long* tspart = (unsigned long long*)((char*)a.scratch + kTsumBytes + kPartBytes);
    int32_t* counts = (int32_t*)((char*)a.scratch + kTsumBytes + kPartBytes + kTsPartBytes);
    if (a.shape == kScanTiled) {
        // 8 bins per lane; more only where kMaxTiles tiles of that size would not cover the bins
        const int64_t need = ((int64_t)a.n + (int64_t)kMaxTiles * kTileLanes - 1) / ((int64_t)kMaxTiles * kTileLanes);
        const int32_t epl = (int32_t)(need > 8 ? need : 8);
        const int32_t tiles = (int32_t)(((int64_t)a.n + (int64_t)kTileLanes * epl - 1) / ((int64_t)kTileLanes * epl));
        hipLaunchKernelGGL(tile_sum_kernel, dim3(tiles, 3), dim3(kTileLanes), 0, s, a.hist, a.n, epl, tsum);
        hipLaunchKernelGGL(tile_apply_kernel, dim3(tiles, 3), dim3(kTileLanes), 0, s, a.hist, a.n, epl, tsum, a.edc);
    } else {
        hipLaunchKernelGGL(scan_wg_kernel, dim3(3), dim3(kScanLanes), 0, s, a.hist, a.n, a.edc);
    }
    hipLaunchKernelGGL(fit_partials_kernel, dim3(kFitTiles, 3), dim3(kFitLanes), 0, s, a.edc, a.n, part, tspart,
                       counts);
    hipLaunchKernelGGL(acoustics_final_kernel, dim3(1), dim3(64), 0, s, a.edc, a.n, a.sample_rate, a.unit, part, tspart,
                       counts, a.out);
    return hipGetLastError();
}

}  // namespace arx

// ---- host: the same definitions in plain C++ (no device needed) ---------------------------------

extern "C" {

arx_status arx_debug_log10_shared(const double* x, size_t n, double* out) {
    if (n > 0 && (!x || !out)) return arx::fail(ARX_ERR_INVALID_ARGUMENT, "NULL argument");
    for (size_t i = 0; i < n; ++i) out[i] = arx::log10_shared(x[i]);
    return ARX_OK;
}

arx_status arx_edc_from_histogram(const int64_t* hist, size_t ir_len, int64_t* edc) {
    if (!hist || !edc || ir_len == 0) return arx::fail(ARX_ERR_INVALID_ARGUMENT, "NULL histogram / curve or ir_len == 0");
    unsigned __int128 run = 0;
    for (size_t k = ir_len; k-- > 0;) {
        if (hist[k] < 0) return arx::fail(ARX_ERR_INVALID_ARGUMENT, "histogram bin %zu is negative", k);
        run += (unsigned __int128)hist[k];
        if (run > (unsigned __int128)INT64_MAX)
            return arx::fail(ARX_ERR_INVALID_ARGUMENT, "the histogram's sum does not fit 63 bits");
        edc[k] = (int64_t)run;
    }
    return ARX_OK;
}

arx_status arx_acoustics_from_histogram(const int64_t* left, const int64_t* right, size_t ir_len, int32_t sample_rate,
                                        double unit, arx_acoustics out[3]) {
    using namespace arx;
    if (!left || !right || !out || ir_len == 0 || ir_len > (size_t)INT32_MAX)
        return fail(ARX_ERR_INVALID_ARGUMENT, "NULL histogram / result, or ir_len not in [1, 2^31)");
    if (sample_rate <= 0) return fail(ARX_ERR_INVALID_ARGUMENT, "sample_rate %d must be positive", sample_rate);
    const int32_t n = (int32_t)ir_len;
    std::vector<int64_t> sum(ir_len), e(ir_len);
    for (size_t k = 0; k < ir_len; ++k) {
        if (left[k] < 0 || right[k] < 0) return fail(ARX_ERR_INVALID_ARGUMENT, "histogram bin %zu is negative", k);
        sum[k] = (int64_t)((uint64_t)left[k] + (uint64_t)right[k]);
        if (sum[k] < 0) return fail(ARX_ERR_INVALID_ARGUMENT, "the histogram's sum does not fit 63 bits");
    }
    const int64_t* chan[3] = {left, right, sum.data()};
    for (int c = 0; c < 3; ++c) {
        const arx_status st = arx_edc_from_histogram(chan[c], ir_len, e.data());
        if (st != ARX_OK) return st;
        const long long total = e[0];
        if (total <= 0) {
            acoustics_empty(out + c, unit);
            continue;
        }
        const Levels lv = make_levels(total);
        int32_t cnt[kPreds] = {};
        for (int p = 0; p < kPreds; ++p)
            while (cnt[p] < n && level_pred(p, e[cnt[p]], lv)) ++cnt[p];
        const Ranges r = make_ranges(cnt, n);
        // The fits' sums in the device's reduction order (fit_partials_kernel, acoustics_final_kernel): per tile
        // a strided partial per lane, the lanes' tree, then the tiles in index order -- f64 addition is not
        // associative, and in this order the same curve gives the device's sums term for term.
        double sxy[3] = {0.0, 0.0, 0.0};
        const double dtotal = (double)total;
        const double mid[3] = {fit_mid(r, 0), fit_mid(r, 1), fit_mid(r, 2)};
        const int64_t tlen = ((int64_t)n + kFitTiles - 1) / kFitTiles;
        std::vector<double> lanes(3 * (size_t)kFitLanes);
        for (int tile = 0; tile < kFitTiles; ++tile) {
            const int64_t k0 = min64((int64_t)n, (int64_t)tile * tlen), k1 = min64((int64_t)n, k0 + tlen);
            std::fill(lanes.begin(), lanes.end(), 0.0);
            for (int t = 0; t < kFitLanes; ++t)
                for (int64_t k = k0 + t; k < k1; k += kFitLanes) {
                    const long long v = e[(size_t)k];
                    bool in[3];
                    for (int f = 0; f < 3; ++f) in[f] = r.ok[f] && k >= r.a[f] && k <= r.b[f];
                    if ((in[0] || in[1] || in[2]) && v > 0) {
                        const double y = level_db(v, dtotal);
                        for (int f = 0; f < 3; ++f)
                            if (in[f]) lanes[(size_t)f * kFitLanes + t] += ((double)k - mid[f]) * y;
                    }
                }
            for (int stride = kFitLanes / 2; stride > 0; stride >>= 1)
                for (int t = 0; t < stride; ++t)
                    for (int f = 0; f < 3; ++f) lanes[(size_t)f * kFitLanes + t] += lanes[(size_t)f * kFitLanes + t + stride];
            for (int f = 0; f < 3; ++f) sxy[f] += lanes[(size_t)f * kFitLanes];
        }
        unsigned __int128 ts = 0;
        for (int32_t k = r.onset + 1; k < n; ++k) ts += (unsigned __int128)e[k];
        long long late[2];
        const int32_t wms[2] = {50, 80};
        for (int w = 0; w < 2; ++w) {
            const int64_t k = (int64_t)r.onset + window_bins(wms[w], sample_rate);
            late[w] = k < n ? e[k] : 0;
        }
        acoustics_finish(out + c, total, sample_rate, unit, r, sxy, (unsigned long long)(ts >> 64), (unsigned long long)ts,
                         late[0], late[1]);
    }
    return ARX_OK;
}

}  // extern "C"
