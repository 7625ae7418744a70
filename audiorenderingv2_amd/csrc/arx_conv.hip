// arx_conv.hip -- file-mode FFT convolution for gfx950.
//
// Semantics restated from R/prebuild/obj_raytracer/kernels.cu:382-438
// (convoluteFromAudioBuffer) + AudioRenderer.cpp:706-711: the input is cut into
// S = floor(len/sr) one-second blocks (the tail len mod sr is never processed), each
// block is zero padded to n = ir_len and CIRCULARLY convolved (length n) with the IR,
// the unnormalised results (n * circconv) are overlap-added at 1-s hops clipped to len,
// and the sum is divided by (ir_len/2) (integer division).
//
// MI355X design: instead of 4 launches + 2 cuFFT calls + 3 device syncs per block, all
// blocks of both channels are convolved by four batched launches:
//   A  fwd column FFTs (length N1, in LDS) of the block PAIRS packed as re/im
//      (x = block_2p + i*block_2p+1: one complex FFT serves two real blocks, and the
//      inverse of (X * H) returns both results in re/im because h is real), times the
//      four-step twiddle W_M^(n2*k1);
//   B  per row: fwd row FFT (N2), * H_c, inverse row FFT, * W_M^(-n2*k1) -- for both
//      channels from one forward pass (spectrum kept in registers);
//   C  inverse column FFTs -> M * linear convolution of each block, to a f64 scratch;
//   D  overlap-add gather with the circular fold cc[i] = lin[i] + lin[i+n], scaled
//      n/(M*(n/2)), rounded once to f32 (deterministic, no atomics).
// FFT length: when n = N1 x N2 with both factors 7-smooth and <= 512 (every 2-s IR at the usual
// rates: 96000 = 300 x 320 at 48 kHz), M = n itself -- the reference's own circular length -- with
// mixed-radix (8/4/2/3/5/7) sub-FFTs and no fold ("direct" path, pass_*_mr).  Otherwise M is the
// power of two >= n + sr - 1 (linear convolution, folded back to length n in pass D), so every
// (ir_len, sr) pair works with radix-8/4/2 stages.  At C3 the direct path moves 2.7x fewer
// FFT points per block pair than 2^18.  On the direct path a new IR rides along as one packed batch
// h_L + i h_R (its columns in A, its rows and the split into H_L / H_R in B: pass_b_pair), and when
// n = 2 sr with N1 even, C and D are one pass (pass_c_chain: no block window goes through HBM).
// All FFT arithmetic is f64: the result matches the f64 oracle to ~1e-15 relative
// before the single f32 rounding (the "1 ULP of max|y|" bar of SURVEY.md §8c).
//
// This file is the host side: the plan, its scratch, the launch shapes and the entry points.  The
// kernels are arx_conv_kernels.hpp over the FFT device code of arx_conv_fft.hpp; those two headers
// alone are the kernels' identity (conv_kernel_source_id), so a host edit here keeps the stored
// traffic profile.  The streaming convolution is arx_conv_stream.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "arx_conv_kernels.hpp"
#include "arx_kernels.hpp"

namespace arx {

constexpr int kMaxSubLen = 512;  // N1, N2 <= 512: n <= 2^18 (longer IRs take the power-of-two path)

struct ConvPlan {
    bool direct = false;  // mixed-radix FFTs of length n (no fold); else the power-of-two path
    bool r7 = false;      // direct: radix-7 stages present (selects the kernels that carry them)
    Factors f1{}, f2{};   // direct: the radices of N1 and N2
    int32_t n = 0;      // ir_len (circular length of the reference)
    int32_t sr = 0;     // hop (block length)
    int32_t M = 0;      // FFT length (power of two >= n + sr - 1, or n on the direct path)
    int32_t N1 = 0, N2 = 0, lg1 = 0, lg2 = 0;
    int32_t tc = 1;     // pow2: columns per workgroup in passes A / C
    int device = 0;
    double2* d_tw = nullptr;     // W_M^e, e in [0, M)
    double2* d_H = nullptr;      // 2 * M, transposed layout [k1][k2]
    double2* d_G = nullptr;      // direct: M, the packed IR h_L + i h_R after pass A's columns
    double2* d_S = nullptr;      // scratch spectra: pairs_cap * 3 * M (shared + 2 channels)
    double* d_Y = nullptr;       // per block, per channel M*lin (length n + sr - 1)
    int64_t pairs_cap = 0;
    // input reuse (conv_prepare_input): the prepared file's length, and where its spectra live --
    // S[pair][0] on the direct path with the chained pass C, else a copy of the input (d_prep_in)
    // that conv_run_prepared convolves in full
    bool prepared = false;
    bool prep_spectra = false;
    int64_t prep_frames = 0;
    float* d_prep_in = nullptr;
    size_t prep_cap = 0;
    char desc[160] = {0};
};

namespace {

// L = 8^a 4^b 2^c 3^d 5^e 7^f; false if L has another prime factor
bool factor7(int32_t L, Factors& f) {
    f.L = L;
    f.count = 0;
    int32_t v = L, twos = 0;
    while (v % 2 == 0) {
        v /= 2;
        ++twos;
    }
    auto push = [&](int r) {
        if (f.count < kMaxRadices) f.r[f.count] = r;
        ++f.count;
    };
    for (; twos >= 3; twos -= 3) push(8);
    if (twos == 2) push(4);
    if (twos == 1) push(2);
    for (int q : {3, 5, 7})
        while (v % q == 0) {
            v /= q;
            push(q);
        }
    return v == 1 && f.count <= kMaxRadices;
}

// n = N1 x N2, both 7-smooth and <= kMaxSubLen; prefer N2 % 8 == 0 (full 128-B row segments in
// passes A / C), then the most balanced split.
bool direct_split(int32_t n, int32_t& N1, int32_t& N2) {
    Factors f;
    int64_t best = -1;
    for (int32_t d = 2; d <= kMaxSubLen; ++d) {
        if (n % d) continue;
        const int32_t e = n / d;
        if (e < 2 || e > kMaxSubLen || !factor7(d, f) || !factor7(e, f)) continue;
        const int64_t score = (e % 8 ? 1000000 : 0) + std::abs(d - e);
        if (best < 0 || score < best) {
            best = score;
            N1 = d;
            N2 = e;
        }
    }
    return best >= 0;
}

}  // namespace

ConvPlan* conv_plan_create(int32_t ir_len, int32_t sample_rate, int device, char* err, size_t errlen) {
    auto bad = [&](const char* m) -> ConvPlan* {
        if (err && errlen) std::snprintf(err, errlen, "%s", m);
        return nullptr;
    };
    if (ir_len <= 0 || sample_rate <= 0) return bad("ir_len and sample_rate must be positive");
    const int64_t need = (int64_t)ir_len + (int64_t)std::min(ir_len, sample_rate) - 1;
    const int lg = ilog2(std::max<int64_t>(need, 4));
    if (lg > 24) return bad("FFT length above 2^24 is not supported");
    ConvPlan* p = new ConvPlan();
    p->n = ir_len;
    p->sr = sample_rate;
    p->device = device;
    int32_t d1 = 0, d2 = 0;
    if (ir_len >= sample_rate && direct_split(ir_len, d1, d2) && factor7(d1, p->f1) && factor7(d2, p->f2)) {
        p->direct = true;
        for (int i = 0; i < p->f1.count; ++i) p->r7 |= p->f1.r[i] == 7;
        for (int i = 0; i < p->f2.count; ++i) p->r7 |= p->f2.r[i] == 7;
        p->M = ir_len;
        p->N1 = d1;
        p->N2 = d2;
        std::snprintf(p->desc, sizeof(p->desc), "mixed-radix direct circular: n=%d sr=%d (%dx%d) f64", p->n, p->sr,
                      p->N1, p->N2);
    } else {
        p->M = 1 << lg;
        p->lg1 = lg / 2;
        p->lg2 = lg - p->lg1;
        p->N1 = 1 << p->lg1;
        p->N2 = 1 << p->lg2;
        p->tc = std::max(1, std::min(std::min(16, p->N2), 4096 / p->N1));
        std::snprintf(p->desc, sizeof(p->desc), "pow2 linear+fold: n=%d sr=%d M=%d (%dx%d) f64", p->n, p->sr, p->M,
                      p->N1, p->N2);
    }
    hipSetDevice(device);
    std::vector<double2> tw((size_t)p->M);
    const long double two_pi = 6.283185307179586476925286766559L;
    for (int64_t e = 0; e < p->M; ++e) {
        const long double ang = two_pi * (long double)e / (long double)p->M;
        tw[(size_t)e] = make_double2((double)cosl(ang), -(double)sinl(ang));
    }
    if (hipMalloc(&p->d_tw, (size_t)p->M * sizeof(double2)) != hipSuccess ||
        hipMalloc(&p->d_H, 2 * (size_t)p->M * sizeof(double2)) != hipSuccess ||
        (p->direct && hipMalloc(&p->d_G, (size_t)p->M * sizeof(double2)) != hipSuccess) ||
        hipMemcpy(p->d_tw, tw.data(), (size_t)p->M * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess) {
        conv_plan_destroy(p);
        return bad("device allocation failed");
    }
    return p;
}

void conv_plan_destroy(ConvPlan* p) {
    if (!p) return;
    hipFree(p->d_prep_in);
    hipFree(p->d_tw);
    hipFree(p->d_H);
    hipFree(p->d_G);
    hipFree(p->d_S);
    hipFree(p->d_Y);
    delete p;
}

const char* conv_plan_describe(const ConvPlan* p) { return p ? p->desc : ""; }
int32_t conv_plan_block(const ConvPlan* p) { return p ? p->sr : 0; }

// The chained pass C (inverse columns and seams in one pass, no block windows in HBM): n = 2 sr on the
// direct path with N1 even.  Only these plans convolve a time-block shard on its own, and only they
// keep a prepared input as spectra.
static bool chain_plan(const ConvPlan* p) { return p->direct && p->n == 2 * p->sr && p->N1 % 2 == 0; }

bool conv_plan_shards(const ConvPlan* p) { return p && chain_plan(p); }

// per block and channel: n (direct) or the linear length n + sr - 1 that pass D folds
static int64_t plan_ylen(const ConvPlan* p) {
    return p->direct ? (int64_t)p->n : (int64_t)p->n + std::min(p->n, p->sr) - 1;
}

// The only code that frees or allocates S and Y: room for `pairs` (>= 1) block pairs' spectra and,
// with need_windows, their block windows (every pass C but the chained one writes them).  Scratch
// that is large enough is reused; else both are re-made at this size, and a prepared input, whose
// spectra lived in S, is gone.
static hipError_t ensure_scratch(ConvPlan* p, int64_t pairs, bool need_windows) {
    if (pairs <= p->pairs_cap && (p->d_Y || !need_windows)) return hipSuccess;  // pairs_cap > 0: S exists
    hipFree(p->d_S);
    hipFree(p->d_Y);
    p->d_S = nullptr;
    p->d_Y = nullptr;
    p->pairs_cap = 0;
    p->prepared = false;
    hipError_t e = hipMalloc(&p->d_S, (size_t)pairs * 3 * p->M * sizeof(double2));
    if (e == hipSuccess && need_windows) e = hipMalloc(&p->d_Y, (size_t)pairs * 2 * 2 * plan_ylen(p) * sizeof(double));
    if (e == hipSuccess) p->pairs_cap = pairs;
    return e;
}

// The plan's part of the kernels' arguments ...
static PassArgs base_args(const ConvPlan* p) {
    PassArgs a;
    std::memset(&a, 0, sizeof(a));
    a.tw = p->d_tw;
    a.M = p->M;
    a.N1 = p->N1;
    a.N2 = p->N2;
    a.lg1 = p->lg1;
    a.lg2 = p->lg2;
    a.tc = p->tc;
    a.n = p->n;
    a.sr = p->sr;
    a.H = p->d_H;
    a.G = p->d_G;
    a.ylen = plan_ylen(p);
    a.tail = 1;  // the whole file: every pair emits (emit_from 0), the last segment included
    return a;
}

// ... and a run's: the scratch, the blocks, the outputs and their scale, a new IR (or nulls).
static PassArgs run_args(const ConvPlan* p, int64_t blocks, int64_t pairs, int64_t len, float* out_l, float* out_r,
                         const float* ir_l, const float* ir_r) {
    PassArgs a = base_args(p);
    a.S = p->d_S;
    a.Y = p->d_Y;
    a.n_blocks = blocks;
    a.n_pairs = pairs;
    a.len = len;
    a.out_l = out_l;
    a.out_r = out_r;
    // the unnormalised inverse FFT gives M x the convolution; the reference keeps n x (cuFFT Z2D) and
    // divides by ir_len / 2 in integers (AudioRenderer.cpp:709; live: normalizeBuffers)
    a.scale = (double)p->n / ((double)p->M * (double)(p->n / 2));
    a.ir_l = ir_l;
    a.ir_r = ir_r;
    return a;
}

static void launch_pass_d(const PassArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pass_d, dim3((unsigned)((a.len + kThreads - 1) / kThreads), 2), dim3(kThreads), 0, s, a);
}

// ---- power-of-two path ----
// passes A / C: tc columns of N1 and the twiddle table
static size_t pow2_lds_a(const ConvPlan* p) { return ((size_t)p->tc + 1) * p->N1 * sizeof(double2); }

// Pass B: the wave-per-row pass (pass_bw) for rows of 512 or 256, else the generic radix-4 pass.
template <int MODE>
static void launch_pass_b(const ConvPlan* p, unsigned batches, const PassArgs& a, hipStream_t s) {
    if (p->N2 == 512 && p->N1 % 4 == 0)
        hipLaunchKernelGGL((pass_bw<MODE, 512>), dim3(p->N1 / 4, batches), dim3(kThreads), (4 + 1) * 512 * sizeof(double2), s, a);
    else if (p->N2 == 256 && p->N1 % 4 == 0)
        hipLaunchKernelGGL((pass_bw<MODE, 256>), dim3(p->N1 / 4, batches), dim3(kThreads), (4 + 1) * 256 * sizeof(double2), s, a);
    else
        hipLaunchKernelGGL(pass_b<MODE>, dim3(p->N1, batches), dim3(kThreads), 2 * (size_t)p->N2 * sizeof(double2), s, a);
}

// Passes A (MODE 0: block pairs of a file, 2: the live block), B and C over `pairs` block pairs.
template <int MODE>
static void pow2_abc(const ConvPlan* p, unsigned pairs, const PassArgs& a, hipStream_t s) {
    const size_t lds_a = pow2_lds_a(p);
    hipLaunchKernelGGL(pass_a<MODE>, dim3(p->N2 / p->tc, pairs), dim3(kThreads), lds_a, s, a);
    launch_pass_b<0>(p, pairs, a, s);
    hipLaunchKernelGGL(pass_c, dim3(p->N2 / p->tc, 2 * pairs), dim3(kThreads), lds_a, s, a);
}

// ---- direct path ----
static MrArgs mr_args(const ConvPlan* p, const PassArgs& a) { return MrArgs{a, p->f1, p->f2, /*batches*/ 1, /*chain*/ 1}; }
// Launch shapes: passes A / C run one wave per column, tc columns per block (ARX_CONV_TCA / _TCC for
// the batched block pairs, 2 for the single live block, for more blocks); pass B one wave per row,
// `rows` rows per block (ARX_CONV_ROWSB; 2 mirror rows in pass_b_pair); ARX_CONV_CHAIN pairs per block
// of the chained pass C.  The macros exist only for design-experiment builds (build.py --exp).
#ifndef ARX_CONV_TCA
#define ARX_CONV_TCA 8
#endif
#ifndef ARX_CONV_TCC
#define ARX_CONV_TCC 4
#endif
#ifndef ARX_CONV_ROWSB
#define ARX_CONV_ROWSB 4
#endif
#ifndef ARX_CONV_CHAIN
#define ARX_CONV_CHAIN 2
#endif
static unsigned mr_tiles(const ConvPlan* p, int tc) { return (unsigned)((p->N2 + tc - 1) / tc); }
static size_t mr_lds_a(const ConvPlan* p, int tc) {
    return ((size_t)tc * mr_col_stride(p->N1, tc) + p->N1 + p->N2) * sizeof(double2);
}
static size_t mr_lds_c(const ConvPlan* p, int tc) { return ((size_t)tc * mr_col_stride(p->N1, tc) + p->N1) * sizeof(double2); }
static unsigned mr_rows(const ConvPlan* p, int rows) { return (unsigned)((p->N1 + rows - 1) / rows); }
static size_t mr_lds_b(const ConvPlan* p, int rows) { return ((size_t)rows * 2 * p->N2 + p->N2) * sizeof(double2); }

// The direct path's launchers for one set of kernel template arguments (mr_dispatch): R7 / LM as in
// fft_mr_wave, L1 / L2 the compile-time sub-FFT lengths or 0.
template <bool R7, int LM, int L1, int L2>
struct Mr {
    // pass A over the block pairs (and, as the batch past them, the packed IR)
    static void launch_a(const ConvPlan* p, unsigned batches, const MrArgs& m, hipStream_t s) {
        hipLaunchKernelGGL((pass_a_mr<0, R7, LM, L1>), dim3(mr_tiles(p, ARX_CONV_TCA), batches), dim3(64 * ARX_CONV_TCA),
                           mr_lds_a(p, ARX_CONV_TCA), s, m);
    }
    // the packed IR's columns alone, to G: with no pairs before it, the IR is batch 0
    static void launch_ir_columns(const ConvPlan* p, MrArgs m, hipStream_t s) {
        m.p.n_pairs = 0;
        launch_a(p, 1u, m, s);
    }
    template <bool XS = false, bool HONLY = false>
    static void launch_b_pair(const ConvPlan* p, int batches, MrArgs m, hipStream_t s) {
        const unsigned units8 = (unsigned)((p->N1 + 1) / 2 + 7) / 8 * 8;  // see pass_b_pair's XCD mapping
        m.batches = batches;
        hipLaunchKernelGGL((pass_b_pair<R7, LM, L2, XS, HONLY>), dim3(units8 * (unsigned)batches), dim3(128),
                           mr_lds_b(p, 2), s, m);
    }
    template <int MODE>
    static void launch_b_mr(const ConvPlan* p, int rows, int batches, MrArgs m, hipStream_t s) {
        const unsigned groups8 = (mr_rows(p, rows) + 7) / 8 * 8;  // see pass_b_mr's XCD mapping
        m.batches = batches;
        hipLaunchKernelGGL((pass_b_mr<MODE, R7, LM, L2>), dim3(groups8 * (unsigned)batches), dim3(64 * rows),
                           mr_lds_b(p, rows), s, m);
    }

    // IR spectra alone (arx_prepare_ir_spectra, the live path, a file shorter than one block): the packed
    // IR h_L + i h_R through pass A's IR batch (to G) and pass B's mirror-row split (to H) -- the route a
    // file convolution with a new IR takes, so H comes out the same bits either way
    static void ir(const ConvPlan* p, const PassArgs& a, hipStream_t s) {
        const MrArgs m = mr_args(p, a);
        launch_ir_columns(p, m, s);
        launch_b_pair<false, true>(p, 1, m, s);
    }

    // File convolution; with_ir: the packed IR's columns ride in pass A's launch as an extra batch and
    // its rows in pass B (pass_b_pair).
    static void file(const ConvPlan* p, const PassArgs& a, int64_t pairs, bool with_ir, hipStream_t s) {
        const MrArgs m = mr_args(p, a);
        launch_a(p, (unsigned)(pairs + (with_ir ? 1 : 0)), m, s);
        if (with_ir)
            launch_b_pair(p, (int)pairs, m, s);
        else
            launch_b_mr<0>(p, ARX_CONV_ROWSB, (int)pairs, m, s);
        pass_c(p, a, pairs, s);
    }

    // Input reuse, step 1 (conv_prepare_input): the audio's columns (pass A) and forward rows (pass B
    // mode 3) once; S[pair][0] keeps every block pair's spectrum.
    static void prepare(const ConvPlan* p, const PassArgs& a, int64_t pairs, hipStream_t s) {
        const MrArgs m = mr_args(p, a);
        launch_a(p, (unsigned)pairs, m, s);
        launch_b_mr<3>(p, ARX_CONV_ROWSB, (int)pairs, m, s);
    }

    // Input reuse, step 2 (conv_run_prepared): a new IR's columns alone in pass A (one batch, to G), then
    // pass B without the audio's forward rows (pass_b_pair<XS> with a new IR, mode 4 without), then pass C.
    static void prepared(const ConvPlan* p, const PassArgs& a, int64_t pairs, bool with_ir, hipStream_t s) {
        const MrArgs m = mr_args(p, a);
        if (with_ir) {
            launch_ir_columns(p, m, s);
            launch_b_pair<true>(p, (int)pairs, m, s);
        } else {
            launch_b_mr<4>(p, ARX_CONV_ROWSB, (int)pairs, m, s);
        }
        pass_c(p, a, pairs, s);
    }

    // Pass C and the overlap-add: one chained pass where the plan has it, else pass_c_mr and pass D.
    static void pass_c(const ConvPlan* p, const PassArgs& a, int64_t pairs, hipStream_t s) {
        MrArgs m = mr_args(p, a);
        const dim3 block(64 * ARX_CONV_TCC);
        const size_t lds = mr_lds_c(p, ARX_CONV_TCC);
        if (chain_plan(p)) {
            m.chain = ARX_CONV_CHAIN;
            const unsigned chains = (unsigned)((pairs - a.emit_from + m.chain - 1) / m.chain);
            const dim3 grid(mr_tiles(p, ARX_CONV_TCC), 2 * chains);
            if constexpr (L1 > 0)
                hipLaunchKernelGGL((pass_c_chain3<R7, LM, L1>), grid, block, lds, s, m);
            else
                hipLaunchKernelGGL((pass_c_chain<R7, LM, L1>), grid, block, lds, s, m);
            return;
        }
        hipLaunchKernelGGL((pass_c_mr<R7, LM, L1>), dim3(mr_tiles(p, ARX_CONV_TCC), (unsigned)(2 * pairs)), block, lds, s, m);
        launch_pass_d(a, s);
    }

    // The live block: two columns / one row per block, for more blocks; its window goes to Y.
    static void live(const ConvPlan* p, const PassArgs& a, hipStream_t s) {
        const MrArgs m = mr_args(p, a);
        hipLaunchKernelGGL((pass_a_mr<2, R7, LM, L1>), dim3(mr_tiles(p, 2), 1), dim3(128), mr_lds_a(p, 2), s, m);
        launch_b_mr<0>(p, 1, 1, m, s);
        hipLaunchKernelGGL((pass_c_mr<R7, LM, L1>), dim3(mr_tiles(p, 2), 2), dim3(128), mr_lds_c(p, 2), s, m);
    }
};

// The kernels exist for the sub-FFT pairs with compile-time plans (fft_ct_stages) and, for any
// other split, for sub-FFT lengths <= 320 / <= 512 with and without radix-7 stages.
template <typename Fn>
static void mr_dispatch(const ConvPlan* p, Fn&& fn) {
    const int N1 = p->N1, N2 = p->N2;
    if (N1 == 300 && N2 == 320) fn(Mr<false, 320, 300, 320>{});
    else if (N1 == 160 && N2 == 200) fn(Mr<false, 320, 160, 200>{});
    else if (N1 == 315 && N2 == 280) fn(Mr<true, 320, 315, 280>{});
    else if (N1 == 250 && N2 == 256) fn(Mr<false, 320, 250, 256>{});
    else if (std::max(N1, N2) <= 320) p->r7 ? fn(Mr<true, 320, 0, 0>{}) : fn(Mr<false, 320, 0, 0>{});
    else p->r7 ? fn(Mr<true, 512, 0, 0>{}) : fn(Mr<false, 512, 0, 0>{});
}

#if ARX_CONV_PROF
// Measurement builds only: read (and clear) the per-workgroup phase records (tools/conv_phases.py).
extern "C" int arx_exp_conv_profile(unsigned long long* out, size_t n_words) {
    const size_t total = 3 * (size_t)kProfPass;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv_prof), std::min(n_words, total) * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
        return 1;
    std::vector<unsigned long long> z(total, 0ull);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_conv_prof), z.data(), total * 8, 0, hipMemcpyHostToDevice) != hipSuccess;
}
#endif

// ---- entry points ----
hipError_t conv_set_ir(ConvPlan* p, const float* d_ir_left, const float* d_ir_right, hipStream_t s) {
    (void)hipGetLastError();  // report this launch's error, not a stale one
    PassArgs a = base_args(p);
    a.ir_l = d_ir_left;
    a.ir_r = d_ir_right;
    if (p->direct) {
        mr_dispatch(p, [&](auto k) { k.ir(p, a, s); });
    } else {
        hipLaunchKernelGGL(pass_a<1>, dim3(p->N2 / p->tc, 2), dim3(kThreads), pow2_lds_a(p), s, a);
        launch_pass_b<1>(p, 2, a, s);
    }
    return hipGetLastError();
}

hipError_t conv_run(ConvPlan* p, const float* d_in, int64_t n_frames, float* d_out_left, float* d_out_right,
                    const float* d_ir_left, const float* d_ir_right, hipStream_t s) {
    return conv_run_pairs(p, d_in, n_frames, d_out_left, d_out_right, d_ir_left, d_ir_right, 0, INT64_MAX, s);
}

// conv_run restricted to the block pairs [pair_begin, pair_end) (time blocks sharded
// across GPUs).  On a chained plan the shard runs passes A and B over its pairs plus the pair before
// them (the seam: its second block's tail F, re-made here instead of received from the neighbour) and
// pass C emits exactly the output segments of its own pairs -- the same per-pair arithmetic in the
// same summation order as the whole file's chains (which re-make the previous pair at every chain
// boundary already), so the union of the shards is the whole convolution bit for bit.  Other plans
// convolve the whole file (every frame written).
hipError_t conv_run_pairs(ConvPlan* p, const float* d_in, int64_t n_frames, float* d_out_left, float* d_out_right,
                          const float* d_ir_left, const float* d_ir_right, int64_t pair_begin, int64_t pair_end,
                          hipStream_t s) {
    const bool with_ir = d_ir_left && d_ir_right;
    if (with_ir && (!p->direct || n_frames < p->sr)) {  // spectra first, then the audio
        const hipError_t e = conv_set_ir(p, d_ir_left, d_ir_right, s);
        if (e != hipSuccess) return e;
        return conv_run_pairs(p, d_in, n_frames, d_out_left, d_out_right, nullptr, nullptr, pair_begin, pair_end, s);
    }
    if (n_frames <= 0) return hipSuccess;
    p->prepared = false;  // any other file convolution discards a prepared input (pass A overwrites its spectra)
    int64_t S = n_frames / p->sr;  // kernels.cu:413
    if (S == 0) {  // nothing convolved: the reference output stays zero (a shard past pair 0 owns none of it)
        if (pair_begin > 0) return hipSuccess;
        hipError_t e = hipMemsetAsync(d_out_left, 0, (size_t)n_frames * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(d_out_right, 0, (size_t)n_frames * sizeof(float), s);
        return e;
    }
    const int64_t all_pairs = (S + 1) / 2;
    int64_t base = 0, pairs = all_pairs;  // local pair 0 = global pair `base`
    int32_t emit_from = 0, tail = 1;
    if (chain_plan(p) && (pair_begin > 0 || pair_end < all_pairs)) {
        const int64_t pb = std::max<int64_t>(0, std::min(pair_begin, all_pairs));
        const int64_t pe = std::max<int64_t>(pb, std::min(pair_end, all_pairs));
        if (pe == pb) {  // an empty shard: its IR spectra still follow the IR
            if (!with_ir) return hipSuccess;
            return conv_set_ir(p, d_ir_left, d_ir_right, s);
        }
        base = pb > 0 ? pb - 1 : 0;
        emit_from = pb > 0 ? 1 : 0;
        tail = pe == all_pairs ? 1 : 0;
        pairs = pe - base;
        const int64_t off = 2 * base * (int64_t)p->sr;
        d_in += off;
        d_out_left += off;
        d_out_right += off;
        n_frames -= off;
        S = std::min<int64_t>(S - 2 * base, 2 * pairs);
    }
    const hipError_t e = ensure_scratch(p, pairs, !chain_plan(p));  // the chained pass C needs no Y
    if (e != hipSuccess) return e;
    (void)hipGetLastError();  // report this launch's error, not a stale one
    PassArgs a = run_args(p, S, pairs, n_frames, d_out_left, d_out_right, d_ir_left, d_ir_right);
    a.in = d_in;
    a.emit_from = emit_from;
    a.tail = tail;
    if (p->direct) {
        mr_dispatch(p, [&](auto k) { k.file(p, a, pairs, with_ir, s); });
    } else {
        pow2_abc<0>(p, (unsigned)pairs, a, s);
        launch_pass_d(a, s);
    }
    return hipGetLastError();
}

// Input reuse (the reference's re-render pattern: full_render_cycle convolves the same file with
// every new IR, AudioRenderer.cpp:790-798, main.cpp:40-67).  conv_prepare_input transforms the file's
// block pairs once (pass A + forward rows, S[pair][0] keeps the spectra); conv_run_prepared then costs
// a new IR's spectra (its columns alone in pass A, its rows in pass B), the products and the inverse
// rows (pass B, no forward FFT of the audio) and pass C.  Same arithmetic as conv_run in the same
// order, so the output is bit-identical.  Plans without the chained pass C keep a copy of the input
// and convolve it in full.
hipError_t conv_prepare_input(ConvPlan* p, const float* d_in, int64_t n_frames, hipStream_t s) {
    p->prepared = false;
    p->prep_frames = n_frames > 0 ? n_frames : 0;
    p->prep_spectra = chain_plan(p);
    const int64_t S = p->prep_frames / p->sr, pairs = (S + 1) / 2;
    (void)hipGetLastError();
    if (!p->prep_spectra) {  // keep the samples: conv_run_prepared convolves them in full
        if ((size_t)p->prep_frames > p->prep_cap) {
            hipFree(p->d_prep_in);
            p->d_prep_in = nullptr;
            p->prep_cap = 0;
            const hipError_t e = hipMalloc(&p->d_prep_in, (size_t)p->prep_frames * sizeof(float));
            if (e != hipSuccess) return e;
            p->prep_cap = (size_t)p->prep_frames;
        }
        if (p->prep_frames > 0) {
            const hipError_t e = hipMemcpyAsync(p->d_prep_in, d_in, (size_t)p->prep_frames * sizeof(float),
                                                hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return e;
        }
        p->prepared = true;
        return hipSuccess;
    }
    if (S > 0) {
        hipError_t e = ensure_scratch(p, pairs, false);
        if (e != hipSuccess) return e;
        PassArgs a = run_args(p, S, pairs, p->prep_frames, nullptr, nullptr, nullptr, nullptr);
        a.in = d_in;
        mr_dispatch(p, [&](auto k) { k.prepare(p, a, pairs, s); });
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    p->prepared = true;
    return hipSuccess;
}

bool conv_has_prepared(const ConvPlan* p) { return p && p->prepared; }
int64_t conv_prepared_frames(const ConvPlan* p) { return p && p->prepared ? p->prep_frames : 0; }

hipError_t conv_run_prepared(ConvPlan* p, float* d_out_left, float* d_out_right, const float* d_ir_left,
                             const float* d_ir_right, hipStream_t s) {
    if (!p->prepared) return hipErrorInvalidValue;
    const int64_t n_frames = p->prep_frames;
    if (!p->prep_spectra) {
        const hipError_t e = conv_run(p, p->d_prep_in, n_frames, d_out_left, d_out_right, d_ir_left, d_ir_right, s);
        p->prepared = true;  // conv_run above reads the kept copy; nothing of it is overwritten
        return e;
    }
    const bool with_ir = d_ir_left && d_ir_right;
    const int64_t S = n_frames / p->sr;
    if (S == 0) {  // no block: the output stays zero (kernels.cu:413), the IR spectra still follow the IR
        if (with_ir) {
            const hipError_t e = conv_set_ir(p, d_ir_left, d_ir_right, s);
            if (e != hipSuccess) return e;
        }
        if (n_frames <= 0) return hipSuccess;
        hipError_t e = hipMemsetAsync(d_out_left, 0, (size_t)n_frames * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(d_out_right, 0, (size_t)n_frames * sizeof(float), s);
        return e;
    }
    const int64_t pairs = (S + 1) / 2;
    (void)hipGetLastError();
    const PassArgs a = run_args(p, S, pairs, n_frames, d_out_left, d_out_right, d_ir_left, d_ir_right);
    mr_dispatch(p, [&](auto k) { k.prepared(p, a, pairs, with_ir, s); });
    return hipGetLastError();
}

hipError_t conv_run_live(ConvPlan* p, const double* d_in, int64_t n_in, double* d_out_interleaved, hipStream_t s) {
    if (n_in < 0 || n_in > p->sr) return hipErrorInvalidValue;
    // the live pass C writes the block's window to Y on every plan, a chained one included; as before,
    // scratch without Y is re-made for this one pair (S shrinks to it)
    const hipError_t e = ensure_scratch(p, 1, true);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();  // report this launch's error, not a stale one
    PassArgs a = run_args(p, 1, 1, 0, nullptr, nullptr, nullptr, nullptr);
    a.in_d = d_in;
    a.n_in = n_in;
    a.out_d = d_out_interleaved;
    if (p->direct)
        mr_dispatch(p, [&](auto k) { k.live(p, a, s); });
    else
        pow2_abc<2>(p, 1, a, s);
    hipLaunchKernelGGL(pass_d_live, dim3((unsigned)((p->n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

#ifndef ARX_CONV_SRC_ID
#define ARX_CONV_SRC_ID 0ull  // set by build.py: hash of the kernel headers and experiment macros
#endif
uint64_t conv_kernel_source_id() { return ARX_CONV_SRC_ID; }

}  // namespace arx
