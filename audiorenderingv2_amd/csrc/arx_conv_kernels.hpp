// arx_conv_kernels.hpp -- the kernels of the file / live convolution (passes A-D of arx_conv.hip's
// header): the power-of-two path (pass_a / pass_b / pass_bw / pass_c), pass D and its live form, and
// the mixed-radix direct path (pass_a_mr, pass_b_mr, pass_b_pair, pass_c_mr, pass_c_chain*), with
// their argument blocks.  Included by arx_conv.hip alone; with arx_conv_fft.hpp it is the kernels'
// identity (build.py CONV_KERNEL_FILES) -- host code stays out of it.
#pragma once

#include "arx_conv_fft.hpp"

namespace arx {

namespace {

constexpr int kThreads = 256;

// Column FFTs of the tile in LDS (tc columns of L, then the twiddle table) by the block's
// 4 waves, tc / 4 columns each.
template <int L>
__device__ __forceinline__ void columns_wave(double2* lds, const double2* twl, int tc, int sign) {
    constexpr int R = L / 64;
    const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
    const int per_wave = tc / 4;
    for (int cc = 0; cc < per_wave; ++cc) {
        double2* cl = lds + (size_t)(per_wave * w + cc) * L;
        double2 x[R];
#pragma unroll
        for (int r = 0; r < R; ++r) x[r] = cl[j + 64 * r];
        fft_wave<L>(x, cl, twl, j, sign);
#pragma unroll
        for (int r = 0; r < R; ++r) cl[j + 64 * r] = x[r];
    }
    __syncthreads();
}

struct PassArgs {
    const double2* tw;
    int32_t M, N1, N2, lg1, lg2, tc;
    int32_t n, sr;
    int64_t n_blocks;   // S
    int64_t n_pairs;
    const float* in;    // audio input (mode 0) or IR pair base (mode 1)
    const float* ir_l;
    const float* ir_r;
    double2* S;         // [pair][3][M]: 0 = forward (shared), 1/2 = per channel
    double2* H;         // [2][M]
    double2* G;         // [M]: pass_a_mr mode 0's packed IR batch
    double* Y;          // [block][2][ylen]
    int64_t ylen;       // n + sr - 1
    float* out_l;
    float* out_r;
    int64_t len;
    double scale;
    const double* in_d;  // live block input (f64)
    int64_t n_in;        // live block length (<= block length of the plan)
    double* out_d;       // live output, interleaved L/R, 2*n doubles
    // chained pass C of a time-block shard (conv_run_pairs): the first local pair whose output
    // segments are written (1 when local pair 0 is the seam pair, re-transformed only for its
    // second block's tail), and whether the segment after the last pair is this shard's (the file's
    // last shard)
    int32_t emit_from;
    int32_t tail;
};

// Pass A: forward column FFTs.  mode 0: batch = block pair p; mode 1: batch = IR channel c.
template <int MODE>
__global__ __launch_bounds__(kThreads) void pass_a(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const int tc = a.tc;
    const int per = kThreads / tc;
    const int col = threadIdx.x / per;  // local column
    const int t = threadIdx.x % per;
    const int64_t batch = blockIdx.y;
    const int n2_0 = blockIdx.x * tc;
    const int n2 = n2_0 + col;
    double2* buf = lds + (size_t)col * a.N1;
    // the N1 twiddles W_N1^e, staged once in LDS after the columns (a global load per
    // butterfly put an L2 round trip into every FFT stage)
    double2* twl = lds + (size_t)tc * a.N1;
    for (int i = threadIdx.x; i < a.N1; i += kThreads) twl[i] = a.tw[(size_t)i * (a.M / a.N1)];
    // load column n2: element n1 at x[N2*n1 + n2]
    for (int i = threadIdx.x; i < tc * a.N1; i += kThreads) {
        const int c = i % tc, n1 = i / tc;  // consecutive threads -> consecutive columns
        const int64_t idx = (int64_t)a.N2 * n1 + n2_0 + c;
        double2 x = make_double2(0.0, 0.0);
        if (MODE == 0) {
            if (idx < a.sr) {
                const int64_t b0 = 2 * batch, b1 = 2 * batch + 1;
                if (b0 < a.n_blocks) x.x = (double)a.in[b0 * a.sr + idx];
                if (b1 < a.n_blocks) x.y = (double)a.in[b1 * a.sr + idx];
            }
        } else if (MODE == 2) {  // live block (f64 samples), zero padded
            if (idx < a.n_in) x.x = a.in_d[idx];
        } else {
            if (idx < a.n) x.x = (double)(batch == 0 ? a.ir_l : a.ir_r)[idx];
        }
        lds[(size_t)c * a.N1 + n1] = x;
    }
    __syncthreads();
    if (a.N1 == 512 && tc == 8) {  // 4 waves x 2 columns, radix-8 in registers (fft512_wave)
        columns_wave<512>(lds, twl, tc, -1);
    } else if (a.N1 == 256 && tc == 16) {  // 4 waves x 4 columns, radix-4 in registers
        columns_wave<256>(lds, twl, tc, -1);
    } else {
        lds_fft(buf, a.N1, a.lg1, -1, t, per, twl, a.N1);
    }
    // twiddle W_M^(n2*k1) and store transposed: S[k1*N2 + n2]
    double2* dst = (MODE != 1) ? a.S + (size_t)batch * 3 * a.M : a.H + (size_t)batch * a.M;
    for (int i = threadIdx.x; i < tc * a.N1; i += kThreads) {
        const int c = i % tc, k1 = i / tc;
        const int64_t e = (int64_t)(n2_0 + c) * k1;
        const double2 x = cmul(lds[(size_t)c * a.N1 + k1], twiddle(a.tw, a.M, e, -1));
        dst[(int64_t)k1 * a.N2 + n2_0 + c] = x;
    }
}

// Pass B.  mode 0: row FFT, * H_c, inverse row FFT, * W_M^(-n2*k1) for c = 0, 1.
//          mode 1: row FFT only (IR spectrum, in place in H).
template <int MODE>
__global__ __launch_bounds__(kThreads) void pass_b(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const int k1 = blockIdx.x;
    const int64_t batch = blockIdx.y;
    const int N2 = a.N2;
    constexpr bool kMul = MODE == 0 || MODE == 4;  // multiply by H and invert
    double2* row = (MODE == 1) ? a.H + (size_t)batch * a.M + (int64_t)k1 * N2 : a.S + (size_t)batch * 3 * a.M + (int64_t)k1 * N2;
    double2* twl = lds + N2;  // W_N2^e staged in LDS (see pass A)
    for (int i = threadIdx.x; i < N2; i += kThreads) {
        lds[i] = row[i];
        twl[i] = a.tw[(size_t)i * (a.M / N2)];
    }
    __syncthreads();
    lds_fft(lds, N2, a.lg2, -1, threadIdx.x, kThreads, twl, N2);
    if (MODE == 1) {
        for (int i = threadIdx.x; i < N2; i += kThreads) row[i] = lds[i];
        return;
    }
    constexpr int kMaxPer = 16;  // N2 <= 4096
    double2 keep[kMaxPer];
#pragma unroll
    for (int b = 0; b < kMaxPer; ++b) {
        const int i = threadIdx.x + b * kThreads;
        if (i < N2) keep[b] = lds[i];
    }
    for (int c = 0; c < 2; ++c) {
        const double2* Hc = a.H + (size_t)c * a.M + (int64_t)k1 * N2;
#pragma unroll
        for (int b = 0; b < kMaxPer; ++b) {
            const int i = threadIdx.x + b * kThreads;
            if (i < N2) lds[i] = cmul(keep[b], Hc[i]);
        }
        __syncthreads();
        lds_fft(lds, N2, a.lg2, +1, threadIdx.x, kThreads, twl, N2);
        double2* dst = a.S + ((size_t)batch * 3 + 1 + c) * a.M + (int64_t)k1 * N2;
        for (int i = threadIdx.x; i < N2; i += kThreads)
            dst[i] = cmul(lds[i], twiddle(a.tw, a.M, (int64_t)i * k1, +1));
        __syncthreads();
    }
}

template <int MODE, int L>
__global__ __launch_bounds__(kThreads) void pass_bw(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    constexpr int kRows = kThreads / 64;
    constexpr int R = L / 64;
    const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
    const int k1 = blockIdx.x * kRows + w;
    const int64_t batch = blockIdx.y;
    double2* buf = lds + w * L;
    double2* twl = lds + kRows * L;
    for (int i = threadIdx.x; i < L; i += kThreads) twl[i] = a.tw[(size_t)i * (a.M / L)];
    double2* row = (MODE == 0) ? a.S + (size_t)batch * 3 * a.M + (int64_t)k1 * L : a.H + (size_t)batch * a.M + (int64_t)k1 * L;
    double2 x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = row[j + 64 * r];
    __syncthreads();  // twiddle table
    fft_wave<L>(x, buf, twl, j, -1);
    if (MODE == 1) {
#pragma unroll
        for (int r = 0; r < R; ++r) row[j + 64 * r] = x[r];
        return;
    }
    double2 keep[R];
#pragma unroll
    for (int r = 0; r < R; ++r) keep[r] = x[r];
    for (int c = 0; c < 2; ++c) {
        const double2* Hc = a.H + (size_t)c * a.M + (int64_t)k1 * L;
#pragma unroll
        for (int r = 0; r < R; ++r) x[r] = cmul(keep[r], Hc[j + 64 * r]);
        fft_wave<L>(x, buf, twl, j, +1);
        double2* dst = a.S + ((size_t)batch * 3 + 1 + c) * a.M + (int64_t)k1 * L;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = j + 64 * r;
            dst[i] = cmul(x[r], twiddle(a.tw, a.M, (int64_t)i * k1, +1));
        }
    }
}

// Pass C: inverse column FFTs of each (pair, channel) -> M * linear convolution of the
// two blocks of the pair (re / im), written to Y for indices < n + sr - 1.
__global__ __launch_bounds__(kThreads) void pass_c(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const int tc = a.tc;
    const int per = kThreads / tc;
    const int col = threadIdx.x / per;
    const int t = threadIdx.x % per;
    const int64_t pair = blockIdx.y >> 1;
    const int ch = blockIdx.y & 1;
    const int n2_0 = blockIdx.x * tc;
    const double2* src = a.S + ((size_t)pair * 3 + 1 + ch) * a.M;
    double2* twl = lds + (size_t)tc * a.N1;  // W_N1^e staged in LDS (see pass A)
    for (int i = threadIdx.x; i < a.N1; i += kThreads) twl[i] = a.tw[(size_t)i * (a.M / a.N1)];
    for (int i = threadIdx.x; i < tc * a.N1; i += kThreads) {
        const int c = i % tc, k1 = i / tc;
        lds[(size_t)c * a.N1 + k1] = src[(int64_t)k1 * a.N2 + n2_0 + c];
    }
    __syncthreads();
    if (a.N1 == 512 && tc == 8) {  // as in pass A
        columns_wave<512>(lds, twl, tc, +1);
    } else if (a.N1 == 256 && tc == 16) {
        columns_wave<256>(lds, twl, tc, +1);
    } else {
        lds_fft(lds + (size_t)col * a.N1, a.N1, a.lg1, +1, t, per, twl, a.N1);
    }
    const int64_t b0 = 2 * pair, b1 = 2 * pair + 1;
    double* y0 = a.Y + (b0 * 2 + ch) * a.ylen;
    double* y1 = a.Y + (b1 * 2 + ch) * a.ylen;
    for (int i = threadIdx.x; i < tc * a.N1; i += kThreads) {
        const int c = i % tc, n1 = i / tc;
        const int64_t idx = (int64_t)a.N2 * n1 + n2_0 + c;
        if (idx < a.ylen) {
            const double2 v = lds[(size_t)c * a.N1 + n1];
            if (b0 < a.n_blocks) y0[idx] = v.x;
            if (b1 < a.n_blocks) y1[idx] = v.y;
        }
    }
}

// Pass D: out_c[j] = scale * sum_s (lin_s[j - s*sr] + lin_s[j - s*sr + n]) over the
// blocks whose window [s*sr, s*sr + n) covers j (kernels.cu:425-428 clip at len).
__global__ __launch_bounds__(kThreads) void pass_d(PassArgs a) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= a.len) return;
    const int ch = blockIdx.y;
    int64_t s_hi = j / a.sr;
    if (s_hi > a.n_blocks - 1) s_hi = a.n_blocks - 1;
    int64_t s_lo = (j - a.n + 1 <= 0) ? 0 : (j - a.n + 1 + a.sr - 1) / a.sr;
    double acc = 0.0;
    for (int64_t s = s_lo; s <= s_hi; ++s) {
        const int64_t i = j - s * a.sr;
        const double* y = a.Y + (s * 2 + ch) * a.ylen;
        double v = y[i];
        if (i + a.n < a.ylen) v += y[i + a.n];
        acc += v;
    }
    (ch == 0 ? a.out_l : a.out_r)[j] = (float)(acc * a.scale);
}

// Live pass D (convoluteLiveInput, AudioRenderer.cpp:623-644): the single block's circular
// length-n convolution (lin[i] + lin[i+n]) for i in [0, n), scaled n/(M*(n/2)) (Z2D x n then
// normalizeBuffers' /(ir_len/2)) and zipped L/R (d_zipArrays, kernels.cu:469-479), in f64.
__global__ __launch_bounds__(kThreads) void pass_d_live(PassArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const double* y = a.Y + ch * a.ylen;
        double v = y[i];
        if (i + a.n < a.ylen) v += y[i + a.n];
        a.out_d[2 * i + ch] = v * a.scale;
    }
}

// ==================================================================================================
// Mixed-radix direct path: when ir_len n = N1 x N2 with both factors 7-smooth and <= 512 (every
// 2 s IR at 16 / 32 / 44.1 / 48 / 96 kHz), the block circular convolution of length n is computed
// with FFTs of length n itself -- the reference's own transform length (cuFFT, kernels.cu:413-437)
// -- instead of the power of two >= n + sr - 1 and the fold: 96000 instead of 2^18 points per
// 48 kHz block pair, no fold terms in pass D.  Same four passes and layouts as above; the sub-FFTs
// are one wave per row / column in LDS (fft_wave_any, arx_conv_fft.hpp).

// Workgroups are dealt round-robin over the 8 XCDs: give each XCD a contiguous run of tiles, so
// that the tiles sharing a 128-B line (pass A's f32 rows, pass C's f64 rows) share its L2.
__device__ __forceinline__ int xcd_tile(int bid, int nblk) {
    return (nblk & 7) ? bid : (bid & 7) * (nblk >> 3) + (bid >> 3);
}

struct MrArgs {
    PassArgs p;
    Factors f1, f2;  // the column (N1) and row (N2) sub-FFTs
    int32_t batches;  // pass B: batches in its 1-D grid
    int32_t chain;    // pass_c_chain: pairs per block
};

// Measurement builds only (build.py --exp cprof -D ARX_CONV_PROF=1, tools/conv_phases.py): per
// workgroup of passes A / B / C, the 100-MHz device real-time counter at entry, after its loads
// reached LDS, after its FFT and at its last store; kProfSlot words per workgroup, pass k's records
// from k * kProfPass.  The product build compiles none of it.
#ifndef ARX_CONV_PROF
#define ARX_CONV_PROF 0
#endif
#if ARX_CONV_PROF
constexpr int kProfSlot = 8, kProfPass = 4096 * kProfSlot;
__device__ unsigned long long g_conv_prof[3 * kProfPass];
struct ConvProf {
    unsigned long long t[4] = {0, 0, 0, 0};
    __device__ void mark(int k) { t[k] = __builtin_amdgcn_s_memrealtime(); }
    // one word per lane of wave 0 (a vector store with per-lane addresses)
    __device__ void flush(int pass) {
        const int l = (int)threadIdx.x;
        if (l >= kProfSlot) return;
        const unsigned wg = blockIdx.y * gridDim.x + blockIdx.x;
        unsigned long long v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v = l == k ? t[k] : v;
        v = l == 4 ? (unsigned long long)__builtin_amdgcn_s_getreg((15 << 11) | 20) : v;  // XCC id
        v = l == 5 ? (unsigned long long)wg : v;
        if (wg < 4096) g_conv_prof[pass * kProfPass + wg * kProfSlot + l] = v;
    }
};
#define CONV_PROF_DECL ConvProf prof_;
#define CONV_PROF_MARK(k) prof_.mark(k)
#define CONV_PROF_FLUSH(pass) prof_.flush(pass)
#else
#define CONV_PROF_DECL
#define CONV_PROF_MARK(k)
#define CONV_PROF_FLUSH(pass)
#endif

// LDS column stride of passes A / C with tc columns per block: N1 padded to the residue that keeps
// the tile's transposing stores (a ds_write_b128 group of 8 lanes spans 8 columns for tc = 8) and
// the loads that read it back free of bank conflicts: 7 mod 16 for tc = 8, 4 mod 8 for 4, 8 mod 16
// for 2 (an enumeration over the usual N1 on the banking model of MI355X_MICROARCH.md's LDS table).
__host__ __device__ inline int mr_col_stride(int N1, int tc) {
    const int t = tc >= 8 ? 7 : (tc == 4 ? 4 : 8), m = tc == 4 ? 8 : 16;
    return N1 + ((t - N1) % m + m) % m;
}

// Pass A: forward column FFTs of length N1 (one wave per column, tc = waves per block), * W_n^(n2 k1),
// stored transposed S[k1 N2 + n2].  LDS: tile tc x sc (mr_col_stride), W_N1 (N1), W_n^r (N2).  Mode 0's
// batch past the block pairs (batch = n_pairs) is the IR, packed h_L + i h_R: its columns go to
// G (pass_b_pair), so the IR spectra's column pass rides in the same launch as the audio's (alone in
// it, with n_pairs = 0, when only the spectra are wanted).  Mode 2: the live block (f64 samples).
template <int MODE, bool R7, int LM, int L1>
__global__ __launch_bounds__(512) void pass_a_mr(MrArgs m) {
    constexpr int IT = LM / 64;  // per-lane elements of a column, per-thread tile loads
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const PassArgs& a = m.p;
    const int nt = blockDim.x, tc = nt >> 6, lgc = __builtin_ctz(tc), N1 = a.N1, N2 = a.N2;
    const int64_t batch = blockIdx.y;
    const bool ir = MODE == 0 && batch >= a.n_pairs;
    const int n2_0 = xcd_tile(blockIdx.x, gridDim.x) * tc, sc = mr_col_stride(N1, tc);
    double2* twl = lds + (size_t)tc * sc;
    double2* tr = twl + N1;
    CONV_PROF_DECL
    CONV_PROF_MARK(0);
    double2 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {  // every load in flight before the first use
        const int i = threadIdx.x + it * nt;
        const int c = i & (tc - 1), n1 = i >> lgc, n2 = n2_0 + c;
        const int64_t idx = (int64_t)N2 * n1 + n2;
        double2 x = make_double2(0.0, 0.0);
        if (n1 < N1 && n2 < N2) {
            if (ir) {
                x.x = (double)a.ir_l[idx];
                x.y = (double)a.ir_r[idx];
            } else if (MODE == 0) {
                if (idx < a.sr) {
                    const int64_t b0 = 2 * batch, b1 = 2 * batch + 1;
                    if (b0 < a.n_blocks) x.x = (double)a.in[b0 * a.sr + idx];
                    if (b1 < a.n_blocks) x.y = (double)a.in[b1 * a.sr + idx];
                }
            } else {
                if (idx < a.n_in) x.x = a.in_d[idx];
            }
        }
        v[it] = x;
    }
    stage_table<IT>(twl, a.tw, N1, N2, nt);  // W_N1^i = W_n^(i N2)
    stage_table<IT>(tr, a.tw, N2, 1, nt);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * nt;
        const int c = i & (tc - 1), n1 = i >> lgc;
        if (n1 < N1) lds[(size_t)c * sc + n1] = v[it];
    }
    __syncthreads();
    CONV_PROF_MARK(1);
    fft_wave_any<R7, LM, L1>(lds + (size_t)(threadIdx.x >> 6) * sc, twl, m.f1, threadIdx.x & 63, -1);
    __syncthreads();
    CONV_PROF_MARK(2);
    double2* dst = ir ? a.G : a.S + (size_t)batch * 3 * a.M;
    // W_n^(n2 k1) = W_N1^q W_n^r with n2 k1 = q N2 + r; this thread's column n2 is fixed and k1 steps
    // by 64, so (q, r) advance by (64 n2) div / mod N2 -- one division per thread, not per element
    const int c = threadIdx.x & (tc - 1), n2 = n2_0 + c;
    const int k10 = threadIdx.x >> lgc;
    const int step = 64 * n2, dq = step / N2, dr = step - dq * N2;
    int q = (n2 * k10) / N2, r = n2 * k10 - q * N2;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int k1 = k10 + 64 * it;
        if (k1 < N1 && n2 < N2) dst[(int64_t)k1 * N2 + n2] = cmul(lds[(size_t)c * sc + k1], cmul(twl[q], tr[r]));
        q += dq;
        r += dr;
        if (r >= N2) {
            r -= N2;
            ++q;
        }
    }
    CONV_PROF_MARK(3);
    if (MODE == 0) CONV_PROF_FLUSH(0);
}

// Pass B: per row k1 (one wave; nt / 64 rows per block): forward row FFT (N2); mode 0 multiplies by
// H_c (pass_b_pair's spectra), inverse row FFT, * W_n^(-n2 k1), for both channels.  Input
// reuse (conv_prepare_input / conv_run_prepared): mode 3 stores the forward row FFT of an audio
// block pair in place (S[pair][0] becomes the pair's full spectrum X), mode 4 is mode 0 on such an
// X (no forward FFT) -- the same arithmetic as mode 0 in two launches, so the outputs are identical.
// LDS: 2 x N2 per row (the spectrum; H_0's row, then the product), W_N2 (N2) -- small enough for
// 3 blocks per CU, so one round of blocks covers the C3 grid.
template <int MODE, bool R7, int LM, int L2>
__global__ __launch_bounds__(512) void pass_b_mr(MrArgs m) {
    constexpr int IT = LM / 64;
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const PassArgs& a = m.p;
    const int nt = blockDim.x, rows = nt >> 6, N1 = a.N1, N2 = a.N2;
    const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
    // 1-D grid of (row group, batch), dealt so that every batch of a row group runs on the same XCD:
    // the H rows the batches share are fetched into that XCD's L2 once, not once per batch.
    const int batches = (int)m.batches;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int group = (slot / batches) * 8 + xcd;
    const int64_t batch = slot % batches;
    const int k1 = group * rows + w;
    double2* spec = lds + (size_t)w * 2 * N2;
    double2* work = spec + N2;
    double2* tw2 = lds + (size_t)rows * 2 * N2;
    const bool live = k1 < N1;
    constexpr bool kMul = MODE == 0 || MODE == 4;  // multiply by H and invert
    double2* row = a.S + (size_t)batch * 3 * a.M + (int64_t)k1 * N2;
    // every global operand of the row up front: the row, H_0 and H_1's rows and the four-step
    // twiddles, so the wave's only global round trip before its stores is this one
    // W_n^(n2 k1) = W_N1^q W_n^r with n2 k1 = q N2 + r (as in pass A): two small tables that stay in
    // L2, where the direct W_n^(n2 k1) gathered lines from all of the n-entry table
    double2 v[IT], h[IT], h1[IT], twq[IT], twr[IT];
    const int step = 64 * k1, dq = step / N2, dr = step - dq * N2;
    int q = (j * k1) / N2, r = j * k1 - q * N2;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        const bool in = live && i < N2;
        const bool in0 = kMul && in;
        v[it] = in ? row[i] : make_double2(0.0, 0.0);
        h[it] = in0 ? a.H[(int64_t)k1 * N2 + i] : make_double2(0.0, 0.0);
        h1[it] = in0 ? a.H[(size_t)a.M + (int64_t)k1 * N2 + i] : make_double2(0.0, 0.0);
        twq[it] = in0 ? a.tw[(int64_t)q * N2] : make_double2(1.0, 0.0);
        twr[it] = in0 ? a.tw[r] : make_double2(1.0, 0.0);
        q += dq;
        r += dr;
        if (r >= N2) {
            r -= N2;
            ++q;
        }
    }
    stage_table<IT>(tw2, a.tw, N2, N1, nt);  // W_N2^i = W_n^(i N1)
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        if (live && i < N2) {
            spec[i] = v[it];
            if (kMul) work[i] = h[it];
        }
    }
    __syncthreads();
    if (!live) return;  // no block barrier below
    if (MODE != 4) fft_wave_any<R7, LM, L2>(spec, tw2, m.f2, j, -1);
    if (MODE == 3) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = j + 64 * it;
            if (i < N2) row[i] = spec[i];
        }
        return;
    }
    // both channels' products (spec x H_0 -> work, spec x H_1 -> spec), then both inverse row FFTs
    // interleaved
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        if (i < N2) {
            const double2 x = spec[i];
            work[i] = cmul(x, work[i]);
            spec[i] = cmul(x, h1[it]);
        }
    }
    __builtin_amdgcn_wave_barrier();
    fft2_wave_any<R7, LM, L2>(work, spec, tw2, m.f2, j, +1);
    double2* dst0 = a.S + ((size_t)batch * 3 + 1) * a.M + (int64_t)k1 * N2;
    double2* dst1 = dst0 + a.M;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        if (i < N2) {
            const double2 w = cmul(twq[it], twr[it]);
            const double2 t = make_double2(w.x, -w.y);
            dst0[i] = cmul(work[i], t);
            dst1[i] = cmul(spec[i], t);
        }
    }
}

// Pass B of a file convolution with a new IR, the IR's row FFTs folded in (no separate IR pass):
// pass A transformed the columns of g = h_L + i h_R as one packed batch (G).  For real h_L, h_R,
//   H_L[k] = (G[k] + conj(G[-k])) / 2,   H_R[k] = (G[k] - conj(G[-k])) / (2i),
// and with k = k1 + N1 k2, -k lies in row k1' = N1 - k1 at column N2 - 1 - k2 (k1 != 0), or in
// row 0 at column (N2 - k2) mod N2 (k1 = 0).  A block is the two waves of mirror rows k1, k1' of
// one block pair (rows 0 and N1/2 are their own mirrors and share a block): each wave
// transforms its S row and its G row (interleaved), reads its mirror's G row from LDS, and goes on
// as pass_b_mr<0>.  Block pair 0 also stores H_L / H_R, the spectra later calls reuse.
// LDS: 2 x N2 per wave (S's spectrum; G's row, then the product), W_N2 (N2).
// XS (input reuse, conv_run_prepared): the S rows already hold the block pairs' row spectra (pass_b_mr
// mode 3), so only the G rows are transformed forward.
// HONLY (the IR spectra alone, conv_set_ir): no block pair -- the G rows are transformed and H_L / H_R
// stored, by the same arithmetic as the fused pass's, so the spectra a convolution uses are the same
// bits whichever call made them.
template <bool R7, int LM, int L2, bool XS, bool HONLY = false>
__global__ __launch_bounds__(128) void pass_b_pair(MrArgs m) {
    constexpr int IT = LM / 64;
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const PassArgs& a = m.p;
    const int N1 = a.N1, N2 = a.N2, units = (N1 + 1) / 2;
    const int w = threadIdx.x >> 6, j = threadIdx.x & 63;
    const int batches = (int)m.batches;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int u = (slot / batches) * 8 + xcd;  // mirror-row unit, dealt as pass_b_mr's row groups
    const int64_t batch = slot % batches;
    if (u >= units) return;  // the whole block: no barrier is reached
    CONV_PROF_DECL
    CONV_PROF_MARK(0);
    const bool self = u == 0;  // rows 0 and N1 / 2: each its own mirror
    const int k1 = w == 0 ? u : (self ? N1 / 2 : N1 - u);
    const bool live = !(self && w == 1 && (N1 & 1));  // odd N1: row 0 has no partner row
    double2* spec = lds + (size_t)w * 2 * N2;
    double2* gbuf = spec + N2;
    double2* gmir = self ? gbuf : lds + (size_t)(w ^ 1) * 2 * N2 + N2;
    double2* tw2 = lds + (size_t)4 * N2;
    double2* row = HONLY ? nullptr : a.S + (size_t)batch * 3 * a.M + (int64_t)k1 * N2;
    double2 v[IT], g[IT], twq[IT], twr[IT];
    const int step = 64 * k1, dq = step / N2, dr = step - dq * N2;
    int q = (j * k1) / N2, r = j * k1 - q * N2;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        const bool in = live && i < N2;
        v[it] = (in && !HONLY) ? row[i] : make_double2(0.0, 0.0);
        g[it] = in ? a.G[(int64_t)k1 * N2 + i] : make_double2(0.0, 0.0);
        twq[it] = in ? a.tw[(int64_t)q * N2] : make_double2(1.0, 0.0);
        twr[it] = in ? a.tw[r] : make_double2(1.0, 0.0);
        q += dq;
        r += dr;
        if (r >= N2) {
            r -= N2;
            ++q;
        }
    }
    stage_table<IT>(tw2, a.tw, N2, N1, 128);  // W_N2^i = W_n^(i N1)
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        if (i < N2) {
            spec[i] = v[it];
            gbuf[i] = g[it];
        }
    }
    __syncthreads();
    CONV_PROF_MARK(1);
    if constexpr (XS || HONLY)
        fft_wave_any<R7, LM, L2>(gbuf, tw2, m.f2, j, -1);
    else
        fft2_wave_any<R7, LM, L2>(spec, gbuf, tw2, m.f2, j, -1);
    __syncthreads();  // the mirror row's G spectrum is complete
    double2 h0[IT], h1[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        if (i < N2) {
            const int mi = k1 == 0 ? (i == 0 ? 0 : N2 - i) : N2 - 1 - i;
            const double2 x = gbuf[i], y = gmir[mi];
            h0[it] = make_double2(0.5 * (x.x + y.x), 0.5 * (x.y - y.y));  // (G + conj(G-)) / 2
            h1[it] = make_double2(0.5 * (x.y + y.y), -0.5 * (x.x - y.x));  // (G - conj(G-)) / 2i
        } else {
            h0[it] = h1[it] = make_double2(0.0, 0.0);
        }
    }
    if (batch == 0 && live) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = j + 64 * it;
            if (i < N2) {
                a.H[(int64_t)k1 * N2 + i] = h0[it];
                a.H[(size_t)a.M + (int64_t)k1 * N2 + i] = h1[it];
            }
        }
    }
    if constexpr (HONLY) return;  // no barrier below is reached by any wave
    __syncthreads();  // every mirror read is done before gbuf is overwritten
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        if (i < N2) {
            const double2 x = spec[i];
            gbuf[i] = cmul(x, h0[it]);
            spec[i] = cmul(x, h1[it]);
        }
    }
    __builtin_amdgcn_wave_barrier();
    fft2_wave_any<R7, LM, L2>(gbuf, spec, tw2, m.f2, j, +1);
    CONV_PROF_MARK(2);
#if ARX_CONV_PROF
    if (!live) {
        CONV_PROF_MARK(3);
        CONV_PROF_FLUSH(1);
        return;
    }
#endif
    if (!live) return;
    double2* dst0 = a.S + ((size_t)batch * 3 + 1) * a.M + (int64_t)k1 * N2;
    double2* dst1 = dst0 + a.M;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = j + 64 * it;
        if (i < N2) {
            const double2 tw = cmul(twq[it], twr[it]);
            const double2 t = make_double2(tw.x, -tw.y);
            dst0[i] = cmul(gbuf[i], t);
            dst1[i] = cmul(spec[i], t);
        }
    }
    CONV_PROF_MARK(3);
    CONV_PROF_FLUSH(1);
}

// Pass C: inverse column FFTs of each (pair, channel) -> n * circular convolution of the pair's two
// blocks (re / im), to Y (length n per block and channel).  LDS: tile tc x sc, W_N1 (N1).
template <bool R7, int LM, int L1>
__global__ __launch_bounds__(512) void pass_c_mr(MrArgs m) {
    constexpr int IT = LM / 64;
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const PassArgs& a = m.p;
    const int nt = blockDim.x, tc = nt >> 6, lgc = __builtin_ctz(tc), N1 = a.N1, N2 = a.N2;
    const int64_t pair = blockIdx.y >> 1;
    const int ch = blockIdx.y & 1;
    const int n2_0 = xcd_tile(blockIdx.x, gridDim.x) * tc, sc = mr_col_stride(N1, tc);
    const double2* src = a.S + ((size_t)pair * 3 + 1 + ch) * a.M;
    double2* twl = lds + (size_t)tc * sc;
    double2 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * nt;
        const int c = i & (tc - 1), k1 = i >> lgc, n2 = n2_0 + c;
        v[it] = (k1 < N1 && n2 < N2) ? src[(int64_t)k1 * N2 + n2] : make_double2(0.0, 0.0);
    }
    stage_table<IT>(twl, a.tw, N1, N2, nt);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * nt;
        const int c = i & (tc - 1), k1 = i >> lgc;
        if (k1 < N1) lds[(size_t)c * sc + k1] = v[it];
    }
    __syncthreads();
    fft_wave_any<R7, LM, L1>(lds + (size_t)(threadIdx.x >> 6) * sc, twl, m.f1, threadIdx.x & 63, +1);
    __syncthreads();
    const int64_t b0 = 2 * pair, b1 = 2 * pair + 1;
    double* y0 = a.Y + (b0 * 2 + ch) * a.ylen;
    double* y1 = a.Y + (b1 * 2 + ch) * a.ylen;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * nt;
        const int c = i & (tc - 1), n1 = i >> lgc, n2 = n2_0 + c;
        if (n1 < N1 && n2 < N2) {
            const int64_t idx = (int64_t)N2 * n1 + n2;
            const double2 x = lds[(size_t)c * sc + n1];
            if (b0 < a.n_blocks) y0[idx] = x.x;
            if (b1 < a.n_blocks) y1[idx] = x.y;
        }
    }
}

// Pass C for n = 2 sr and N1 even, fused with the seam sum: a block runs one column tile of one
// channel through a chain of consecutive pairs p0 .. p1-1 (m.chain per block), preceded by pair
// p0-1 again when p0 > 0.  Rows n1 < N1/2 of a pair's inverse columns hold the first half of each
// block's window (i = idx < sr), rows n1 + N1/2 the second: the pair's odd output segment 2p+1 =
// y_2p[i + sr] + y_2p+1[i] (hi.x + lo.y) lies inside the pair, and the even segment 2p =
// y_2p-1[i + sr] + y_2p[i] adds the previous pair's hi.y, which this thread computed for the same
// (column, row) one step earlier and holds in registers.  Sums in pass D's order (0 + F + E),
// rounded once; no block window goes through HBM (Y), and no seam pass runs.
template <bool R7, int LM, int L1>
__device__ __forceinline__ void pass_c_chain_body(const MrArgs& m) {
    constexpr int IT = LM / 64;
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const PassArgs& a = m.p;
    const int nt = blockDim.x, tc = nt >> 6, lgc = __builtin_ctz(tc), N1 = a.N1, N2 = a.N2, half = N1 >> 1;
    const int ch = blockIdx.y & 1;
    const int64_t p0 = a.emit_from + (int64_t)(blockIdx.y >> 1) * m.chain;
    const int64_t p1 = p0 + m.chain < a.n_pairs ? p0 + m.chain : a.n_pairs;
    const int n2_0 = xcd_tile(blockIdx.x, gridDim.x) * tc, sc = mr_col_stride(N1, tc);
    double2* twl = lds + (size_t)tc * sc;
    const int64_t sr = a.sr;
    float* out = ch == 0 ? a.out_l : a.out_r;
    CONV_PROF_DECL
    CONV_PROF_MARK(0);
    stage_table<IT>(twl, a.tw, N1, N2, nt);
    double2 v[IT];
    double fprev[IT];  // hi.y of the previous pair at this thread's (column, row) slots
    const int64_t pstart = p0 > 0 ? p0 - 1 : 0;
    auto load = [&](int64_t pair) {
        const double2* src = a.S + ((size_t)pair * 3 + 1 + ch) * a.M;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = threadIdx.x + it * nt;
            const int c = i & (tc - 1), k1 = i >> lgc, n2 = n2_0 + c;
            v[it] = (k1 < N1 && n2 < N2) ? src[(int64_t)k1 * N2 + n2] : make_double2(0.0, 0.0);
        }
    };
    load(pstart);
#pragma unroll
    for (int it = 0; it < IT; ++it) fprev[it] = 0.0;
    for (int64_t pair = pstart; pair < p1; ++pair) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = threadIdx.x + it * nt;
            const int c = i & (tc - 1), k1 = i >> lgc;
            if (k1 < N1) lds[(size_t)c * sc + k1] = v[it];
        }
        __syncthreads();
#if ARX_CONV_PROF
        if (pair == pstart) CONV_PROF_MARK(1);
#endif
        if (pair + 1 < p1) load(pair + 1);  // in flight during this pair's FFT
        fft_wave_any<R7, LM, L1>(lds + (size_t)(threadIdx.x >> 6) * sc, twl, m.f1, threadIdx.x & 63, +1);
        __syncthreads();
#if ARX_CONV_PROF
        if (pair == pstart) CONV_PROF_MARK(2);
#endif
        const int64_t b1 = 2 * pair + 1;
        const bool odd = b1 < a.n_blocks;  // the pair's second block exists
        const bool emit = pair >= p0;     // pair p0 - 1 only supplies fprev
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = threadIdx.x + it * nt;
            const int c = i & (tc - 1), n1 = i >> lgc, n2 = n2_0 + c;
            if (n1 < half && n2 < N2) {
                const int64_t idx = (int64_t)N2 * n1 + n2;
                const double2 lo = lds[(size_t)c * sc + n1], hi = lds[(size_t)c * sc + n1 + half];
                if (emit) {
                    const int64_t te = 2 * pair * sr + idx, to = b1 * sr + idx;
                    if (te < a.len) {
                        double acc = 0.0;
                        acc += fprev[it];  // F_p-1 (zero for p = 0)
                        acc += lo.x;       // E_p
                        out[te] = (float)(acc * a.scale);
                    }
                    if (to < a.len) {
                        double acc = 0.0;
                        acc += hi.x;
                        if (odd) acc += lo.y;
                        out[to] = (float)(acc * a.scale);
                    }
                }
                fprev[it] = odd ? hi.y : 0.0;
            }
        }
        __syncthreads();  // the tile is rewritten by the next pair
    }
    if (p1 == a.n_pairs && a.tail) {  // the segment after the last pair: F_last alone
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = threadIdx.x + it * nt;
            const int c = i & (tc - 1), n1 = i >> lgc, n2 = n2_0 + c;
            if (n1 < half && n2 < N2) {
                const int64_t idx = (int64_t)N2 * n1 + n2, t = 2 * p1 * sr + idx;
                if (t < a.len) {
                    double acc = 0.0;
                    acc += fprev[it];
                    out[t] = (float)(acc * a.scale);
                }
            }
        }
    }
    CONV_PROF_MARK(3);
    CONV_PROF_FLUSH(2);
}
// The compile-time plans (L1 > 0) fit in 168 VGPRs = 3 waves per SIMD without spilling; left to
// itself the compiler took 169 (2 waves), so the C3 launch's 640 four-wave blocks (2.5 waves per
// SIMD) ran in two rounds (8.5 us entry skew, tools/conv_phases.py).  The run-time plans keep the
// unconstrained allocation (168 would spill there).
template <bool R7, int LM, int L1>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(3))) void pass_c_chain3(MrArgs m) {
    pass_c_chain_body<R7, LM, L1>(m);
}
template <bool R7, int LM, int L1>
__global__ __launch_bounds__(512) void pass_c_chain(MrArgs m) {
    pass_c_chain_body<R7, LM, L1>(m);
}

}  // namespace

}  // namespace arx
