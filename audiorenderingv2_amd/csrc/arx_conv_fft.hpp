// arx_conv_fft.hpp -- the f64 FFT device code the convolutions share (arx_conv_kernels.hpp, the
// file / live kernels; arx_conv_stream.hip, the streaming ones): complex helpers, the radix-4/2
// Stockham FFT of a workgroup in LDS (lds_fft_t), the one-wave 512- and 256-point FFTs, and the
// one-wave mixed-radix (8/4/2/3/5/7) FFTs with run-time (fft_mr_wave) or compile-time
// (fft_ct_stages) plans.  Part of the convolution kernels' identity (build.py CONV_KERNEL_FILES).
#pragma once

#include <hip/hip_runtime.h>

namespace arx {

constexpr int kMaxRadices = 12;

// The radices of a mixed-radix sub-FFT of length L, in stage order (factor7, arx_conv.hip)
struct Factors {
    int32_t L;
    int32_t count;
    int32_t r[kMaxRadices];
};

namespace {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
// multiply by sign*i
__device__ __forceinline__ double2 mul_si(double2 a, int sign) {
    return sign < 0 ? make_double2(a.y, -a.x) : make_double2(-a.y, a.x);
}
__device__ __forceinline__ double2 twiddle(const double2* __restrict__ tw, int32_t M, int64_t e, int sign) {
    const double2 w = tw[e & (M - 1)];
    return sign < 0 ? w : make_double2(w.x, -w.y);
}

// Twiddle sources for lds_fft: W_M^e from one table of M entries, or (TwSplit) the product of two
// small LDS tables hi[e >> lgLo] = W_M^(e & ~(2^lgLo - 1)) and lo[e & (2^lgLo - 1)] = W_M^(e mod 2^lgLo),
// for transforms whose full table would not fit in LDS beside the data.
struct TwFlat {
    const double2* tw;
    int32_t M;
    __device__ double2 operator()(int64_t e, int sign) const { return twiddle(tw, M, e, sign); }
};
struct TwSplit {
    const double2* hi;
    const double2* lo;
    int32_t lgLo, M;
    __device__ double2 operator()(int64_t e, int sign) const {
        const int64_t m = e & (M - 1);
        const double2 w = cmul(hi[m >> lgLo], lo[m & ((1 << lgLo) - 1)]);
        return sign < 0 ? w : make_double2(w.x, -w.y);
    }
};

// In-place Stockham FFT of length L = 2^lg on buf[0..L) (LDS), executed by the nt
// threads t in [0, nt) of this group; every thread of the workgroup must call it (it
// contains __syncthreads()).  Twiddle W_L^e = tw[e * (M/L)].
__device__ void lds_fft(double2* buf, int L, int lg, int sign, int t, int nt, const double2* __restrict__ tw,
                        int32_t M);
template <class TW>
__device__ void lds_fft_t(double2* buf, int L, int lg, int sign, int t, int nt, const TW& twf, int32_t M) {
    const int mstep = M >> lg;  // M / L
    int Ns = 1;
    int stages4 = lg >> 1;
    for (int s = 0; s < stages4; ++s) {
        const int quarter = L >> 2;
        double2 v[4][4];
        int jj[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = t + b * nt;
            jj[b] = j;
            if (j < quarter) {
                const int k = j & (Ns - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double2 x = buf[j + r * quarter];
                    if (r > 0) x = cmul(x, twf((int64_t)r * k * (L / (Ns * 4)) * mstep, sign));
                    v[b][r] = x;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = jj[b];
            if (j < quarter) {
                const int k = j & (Ns - 1);
                const double2 a0 = cadd(v[b][0], v[b][2]);
                const double2 a1 = csub(v[b][0], v[b][2]);
                const double2 a2 = cadd(v[b][1], v[b][3]);
                const double2 a3 = mul_si(csub(v[b][1], v[b][3]), sign);
                const int d = (j - k) * 4 + k;  // (j/Ns)*Ns*4 + j%Ns
                buf[d] = cadd(a0, a2);
                buf[d + Ns] = cadd(a1, a3);
                buf[d + 2 * Ns] = csub(a0, a2);
                buf[d + 3 * Ns] = csub(a1, a3);
            }
        }
        __syncthreads();
        Ns <<= 2;
    }
    if (lg & 1) {  // final radix-2 stage
        const int half = L >> 1;
        double2 v[8][2];
        int jj[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int j = t + b * nt;
            jj[b] = j;
            if (j < half) {
                const int k = j & (Ns - 1);
                v[b][0] = buf[j];
                v[b][1] = cmul(buf[j + half], twf((int64_t)k * (L / (Ns * 2)) * mstep, sign));
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int j = jj[b];
            if (j < half) {
                const int k = j & (Ns - 1);
                const int d = (j - k) * 2 + k;
                buf[d] = cadd(v[b][0], v[b][1]);
                buf[d + Ns] = csub(v[b][0], v[b][1]);
            }
        }
        __syncthreads();
    }
}

__device__ void lds_fft(double2* buf, int L, int lg, int sign, int t, int nt, const double2* __restrict__ tw,
                        int32_t M) {
    lds_fft_t(buf, L, lg, sign, t, nt, TwFlat{tw, M}, M);
}

// ---- 512-point FFTs (the 48 kHz plans): one wave per row / column, radix-8 in registers ----
// Stockham radix-8 over 3 stages: each lane holds 8 elements (j + 64 r), so the row is loaded
// and stored coalesced, the first stage starts from registers, the last one ends in them
// (natural order), and only 2 LDS exchanges per FFT remain -- versus 5 stages x 2 block
// barriers with half the threads idle in the generic radix-4 path.  A wave's LDS operations
// execute in order, so the exchanges inside one wave need no block barrier.
__device__ __forceinline__ double2 mul_w8(double2 a, int sign) {  // * e^(sign i pi/4)
    const double c = 0.70710678118654752440;
    return sign < 0 ? make_double2(c * (a.x + a.y), c * (a.y - a.x)) : make_double2(c * (a.x - a.y), c * (a.x + a.y));
}
__device__ __forceinline__ double2 mul_w83(double2 a, int sign) {  // * e^(sign 3 i pi/4)
    const double c = 0.70710678118654752440;
    return sign < 0 ? make_double2(c * (a.y - a.x), -c * (a.x + a.y)) : make_double2(-c * (a.x + a.y), c * (a.x - a.y));
}
// in-place 8-point DFT, y[q] = sum_r x[r] e^(sign 2 pi i r q / 8)
__device__ __forceinline__ void dft8(double2* x, int sign) {
    double2 a[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        a[r] = cadd(x[r], x[r + 4]);
        b[r] = csub(x[r], x[r + 4]);
    }
    b[1] = mul_w8(b[1], sign);
    b[2] = mul_si(b[2], sign);
    b[3] = mul_w83(b[3], sign);
    // 4-point DFTs of a (even outputs) and b (odd outputs)
    const double2 a0 = cadd(a[0], a[2]), a1 = csub(a[0], a[2]), a2 = cadd(a[1], a[3]), a3 = mul_si(csub(a[1], a[3]), sign);
    const double2 b0 = cadd(b[0], b[2]), b1 = csub(b[0], b[2]), b2 = cadd(b[1], b[3]), b3 = mul_si(csub(b[1], b[3]), sign);
    x[0] = cadd(a0, a2);
    x[4] = csub(a0, a2);
    x[2] = cadd(a1, a3);
    x[6] = csub(a1, a3);
    x[1] = cadd(b0, b2);
    x[5] = csub(b0, b2);
    x[3] = cadd(b1, b3);
    x[7] = csub(b1, b3);
}
// 512-point FFT of the row held as x[r] = element j + 64 r (lane j of the wave); result in the
// same layout.  buf: the wave's 512-element LDS scratch; twl: W_512^e in LDS.
__device__ __forceinline__ void fft512_wave(double2* x, double2* buf, const double2* twl, int j, int sign) {
    dft8(x, sign);  // stage 1 (Ns = 1): no twiddles
#pragma unroll
    for (int q = 0; q < 8; ++q) buf[8 * j + q] = x[q];
    __builtin_amdgcn_wave_barrier();
    {  // stage 2 (Ns = 8)
        const int k = j & 7;
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = buf[j + 64 * r];
#pragma unroll
        for (int r = 1; r < 8; ++r) x[r] = cmul(x[r], twiddle(twl, 512, 8 * r * k, sign));
        dft8(x, sign);
        const int d = (j - k) * 8 + k;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 8; ++q) buf[d + 8 * q] = x[q];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = buf[j + 64 * r];  // stage 3 (Ns = 64): k = j
#pragma unroll
    for (int r = 1; r < 8; ++r) x[r] = cmul(x[r], twiddle(twl, 512, r * j, sign));
    dft8(x, sign);
    __builtin_amdgcn_wave_barrier();
}

// ---- 256-point FFTs (the 16 kHz plans, M = 2^16 = 256 x 256): one wave per row / column,
// four radix-4 Stockham stages, each lane one butterfly per stage on elements j + 64 r (the
// lane's registers), so the first stage starts from registers, the last one ends in them in
// natural order, and 3 in-wave LDS exchanges remain.
__device__ __forceinline__ void dft4(double2* x, int sign) {
    const double2 a0 = cadd(x[0], x[2]), a1 = csub(x[0], x[2]), a2 = cadd(x[1], x[3]), a3 = mul_si(csub(x[1], x[3]), sign);
    x[0] = cadd(a0, a2);
    x[1] = cadd(a1, a3);
    x[2] = csub(a0, a2);
    x[3] = csub(a1, a3);
}
__device__ __forceinline__ void fft256_wave(double2* x, double2* buf, const double2* twl, int j, int sign) {
    dft4(x, sign);  // Ns = 1: no twiddles
#pragma unroll
    for (int q = 0; q < 4; ++q) buf[4 * j + q] = x[q];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int Ns = 4; Ns <= 16; Ns *= 4) {
        const int k = j & (Ns - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = buf[j + 64 * r];
#pragma unroll
        for (int r = 1; r < 4; ++r) x[r] = cmul(x[r], twiddle(twl, 256, (64 / Ns) * r * k, sign));
        dft4(x, sign);
        const int d = (j - k) * 4 + k;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; ++q) buf[d + Ns * q] = x[q];
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = buf[j + 64 * r];  // Ns = 64: k = j
#pragma unroll
    for (int r = 1; r < 4; ++r) x[r] = cmul(x[r], twiddle(twl, 256, r * j, sign));
    dft4(x, sign);
    __builtin_amdgcn_wave_barrier();
}

// L-point wave FFT of x[r] = element j + 64 r (L = 256 or 512)
template <int L>
__device__ __forceinline__ void fft_wave(double2* x, double2* buf, const double2* twl, int j, int sign) {
    if constexpr (L == 512)
        fft512_wave(x, buf, twl, j, sign);
    else
        fft256_wave(x, buf, twl, j, sign);
}

// ---- mixed-radix sub-FFTs (the direct path): one wave per row / column in LDS, Stockham stages of
// radix 8, 4, 2, 3, 5, 7 ----
// y[q] = sum_r x[r] e^(sign 2 pi i r q / R) for odd prime R, with the cos / sin of 2 pi m / R
template <int R>
struct OddDft;
template <>
struct OddDft<3> {
    static constexpr double c[3] = {1.0, -0.5, -0.5};
    static constexpr double s[3] = {0.0, 0.86602540378443864676, -0.86602540378443864676};
};
template <>
struct OddDft<5> {
    static constexpr double c[5] = {1.0, 0.30901699437494742410, -0.80901699437494742410, -0.80901699437494742410,
                                    0.30901699437494742410};
    static constexpr double s[5] = {0.0, 0.95105651629515357212, 0.58778525229247312917, -0.58778525229247312917,
                                    -0.95105651629515357212};
};
template <>
struct OddDft<7> {
    static constexpr double c[7] = {1.0, 0.62348980185873353053, -0.22252093395631440429, -0.90096886790241912624,
                                    -0.90096886790241912624, -0.22252093395631440429, 0.62348980185873353053};
    static constexpr double s[7] = {0.0, 0.78183148246802980871, 0.97492791218182360702, 0.43388373911755812048,
                                    -0.43388373911755812048, -0.97492791218182360702, -0.78183148246802980871};
};

template <int R>
__device__ __forceinline__ void dft_radix(double2* x, int sign) {
    if constexpr (R == 2) {
        const double2 a = x[0], b = x[1];
        x[0] = cadd(a, b);
        x[1] = csub(a, b);
    } else if constexpr (R == 4) {
        dft4(x, sign);
    } else if constexpr (R == 8) {
        dft8(x, sign);
    } else {  // odd prime: pair r with R - r
        constexpr int H = R / 2;
        double2 a[H + 1], b[H + 1];
#pragma unroll
        for (int r = 1; r <= H; ++r) {
            a[r] = cadd(x[r], x[R - r]);
            b[r] = csub(x[r], x[R - r]);
        }
        double2 y0 = x[0];
#pragma unroll
        for (int r = 1; r <= H; ++r) y0 = cadd(y0, a[r]);
        double2 y[R];
#pragma unroll
        for (int q = 1; q <= H; ++q) {
            double2 t = x[0], u = make_double2(0.0, 0.0);
#pragma unroll
            for (int r = 1; r <= H; ++r) {
                const int m = (r * q) % R;
                t.x += OddDft<R>::c[m] * a[r].x;
                t.y += OddDft<R>::c[m] * a[r].y;
                u.x += OddDft<R>::s[m] * b[r].x;
                u.y += OddDft<R>::s[m] * b[r].y;
            }
            const double2 iu = mul_si(u, sign);  // sign * i * u
            y[q] = cadd(t, iu);
            y[R - q] = csub(t, iu);
        }
        x[0] = y0;
#pragma unroll
        for (int q = 1; q < R; ++q) x[q] = y[q];
    }
}

// LDS slot of element i of a sub-FFT buffer between its first two stages when SW: the elements'
// 8-element blocks XOR-swizzled (block k's slots permuted by k mod 8; a tail short of a whole block
// stays put).  The first stage of an even length stores with stride R in {2, 4, 8}: unswizzled, the 8
// lanes of a ds_write_b128 group land on one or two 128-B bank rows (up to 8-way conflicts); swizzled
// they cover all 8.  The second stage reads through the same map and stores in natural order.
template <bool SW>
__device__ __forceinline__ int lds_ix(int i, int L8) {
    return (SW && i < L8) ? (i ^ ((i >> 3) & 7)) : i;
}

// One Stockham stage of radix R over buf[0..L) (LDS, this wave's row / column), Ns = product of
// the earlier radices; twl = W_L^e.  Every lane first reads all its butterflies, then writes.
// SWI / SWO: the input / output is in the lds_ix swizzled order.
template <int R, int LM, bool SWI, bool SWO>
__device__ __forceinline__ void mr_stage(double2* buf, const double2* twl, int L, int Ns, int j, int sign) {
    constexpr int kMaxB = (LM / R + 63) / 64;  // butterflies per lane for L <= LM
    const int nb = L / R, step = L / (Ns * R), L8 = L & ~7;
    double2 v[kMaxB][R];
#pragma unroll
    for (int i = 0; i < kMaxB; ++i) {
        const int b = j + 64 * i;
        if (b < nb) {
            const int k = b % Ns;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                double2 x = buf[lds_ix<SWI>(b + q * nb, L8)];
                if (q > 0) {
                    const double2 w = twl[q * k * step];
                    x = cmul(x, sign < 0 ? w : make_double2(w.x, -w.y));
                }
                v[i][q] = x;
            }
            dft_radix<R>(v[i], sign);
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < kMaxB; ++i) {
        const int b = j + 64 * i;
        if (b < nb) {
            const int k = b % Ns;
            const int d = (b - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; ++q) buf[lds_ix<SWO>(d + q * Ns, L8)] = v[i][q];
        }
    }
    __builtin_amdgcn_wave_barrier();
}

template <bool R7, int LM, bool SWI, bool SWO>
__device__ __forceinline__ void mr_stage_r(int r, double2* buf, const double2* twl, int L, int Ns, int j, int sign) {
    switch (r) {
        case 8: mr_stage<8, LM, SWI, SWO>(buf, twl, L, Ns, j, sign); break;
        case 4: mr_stage<4, LM, SWI, SWO>(buf, twl, L, Ns, j, sign); break;
        case 2: mr_stage<2, LM, SWI, SWO>(buf, twl, L, Ns, j, sign); break;
        case 3: mr_stage<3, LM, SWI, SWO>(buf, twl, L, Ns, j, sign); break;
        case 5: mr_stage<5, LM, SWI, SWO>(buf, twl, L, Ns, j, sign); break;
        default:
            if constexpr (R7) mr_stage<7, LM, SWI, SWO>(buf, twl, L, Ns, j, sign);
            break;
    }
}

// In-place FFT of buf[0..f.L) by one wave (lane j), natural order in and out.  R7: the plan has
// radix-7 stages (their 7-point DFT costs ~20 VGPRs in every kernel that may run one).  An even
// length starts with its radix-2^k stages (factor7), so its first stage stores swizzled (lds_ix).
template <bool R7, int LM>
__device__ __forceinline__ void fft_mr_wave(double2* buf, const double2* twl, const Factors& f, int j, int sign) {
    const bool even = (f.L & 1) == 0;
    int Ns = 1;
    for (int s = 0; s < f.count; ++s) {
        if (even && s == 0)
            mr_stage_r<false, LM, false, true>(f.r[s], buf, twl, f.L, Ns, j, sign);
        else if (even && s == 1)
            mr_stage_r<R7, LM, true, false>(f.r[s], buf, twl, f.L, Ns, j, sign);
        else
            mr_stage_r<R7, LM, false, false>(f.r[s], buf, twl, f.L, Ns, j, sign);
        Ns *= f.r[s];
    }
}

// Compile-time plans for the sub-FFT lengths of the usual IRs (300 x 320 at 48 kHz, 160 x 200 at
// 16 kHz, 315 x 280 at 44.1 kHz, 250 x 256 at 32 kHz): the same radix order as factor7, but every
// stage's R, Ns and butterfly count are constants, so the index arithmetic (b mod Ns, twiddle
// exponents, guards) folds away -- it was most of the generic stages' VALU work.
constexpr int ct_radix(int L, int s) {
    int v = L, t = 0;
    while (v % 2 == 0) {
        v /= 2;
        ++t;
    }
    int idx = 0;
    for (; t >= 3; t -= 3, ++idx)
        if (idx == s) return 8;
    if (t == 2 && idx++ == s) return 4;
    if (t == 1 && idx++ == s) return 2;
    for (int q = 3; q <= 7; q += 2)
        while (v % q == 0) {
            v /= q;
            if (idx++ == s) return q;
        }
    return 0;  // past the last stage
}
constexpr int ct_ns(int L, int s) {
    int ns = 1;
    for (int i = 0; i < s; ++i) ns *= ct_radix(L, i);
    return ns;
}

template <int R, int NS, int L, bool SWI, bool SWO>
__device__ __forceinline__ void mr_stage_ct(double2* buf, const double2* twl, int j, int sign) {
    constexpr int nb = L / R, step = L / (NS * R), kB = (nb + 63) / 64;
    double2 v[kB][R];
#pragma unroll
    for (int i = 0; i < kB; ++i) {
        const int b = j + 64 * i;
        if (nb % 64 == 0 || i < kB - 1 || b < nb) {
            const int k = b % NS;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                double2 x = buf[lds_ix<SWI>(b + q * nb, L & ~7)];
                if (q > 0 && NS > 1) {
                    const double2 w = twl[q * k * step];
                    x = cmul(x, sign < 0 ? w : make_double2(w.x, -w.y));
                }
                v[i][q] = x;
            }
            dft_radix<R>(v[i], sign);
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < kB; ++i) {
        const int b = j + 64 * i;
        if (nb % 64 == 0 || i < kB - 1 || b < nb) {
            const int k = b % NS;
            const int d = (b - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; ++q) buf[lds_ix<SWO>(d + q * NS, L & ~7)] = v[i][q];
        }
    }
    __builtin_amdgcn_wave_barrier();
}

template <int L, int S>
__device__ __forceinline__ void fft_ct_stages(double2* buf, const double2* twl, int j, int sign) {
    if constexpr (ct_radix(L, S) != 0) {
        constexpr bool sw = L % 2 == 0;  // swizzled between the first two stages (lds_ix)
        mr_stage_ct<ct_radix(L, S), ct_ns(L, S), L, sw && S == 1, sw && S == 0>(buf, twl, j, sign);
        fft_ct_stages<L, S + 1>(buf, twl, j, sign);
    }
}

// mr_stage_ct over two independent buffers at once (pass B's two inverse row FFTs): the same
// indices and twiddles, twice the independent work between a lane's LDS round trips.
template <int R, int NS, int L, bool SWI, bool SWO>
__device__ __forceinline__ void mr_stage_ct2(double2* buf0, double2* buf1, const double2* twl, int j, int sign) {
    constexpr int nb = L / R, step = L / (NS * R), kB = (nb + 63) / 64;
    double2 v[kB][R], u[kB][R];
#pragma unroll
    for (int i = 0; i < kB; ++i) {
        const int b = j + 64 * i;
        if (nb % 64 == 0 || i < kB - 1 || b < nb) {
            const int k = b % NS;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                double2 x = buf0[lds_ix<SWI>(b + q * nb, L & ~7)];
                double2 y = buf1[lds_ix<SWI>(b + q * nb, L & ~7)];
                if (q > 0 && NS > 1) {
                    const double2 w = twl[q * k * step];
                    const double2 ws = sign < 0 ? w : make_double2(w.x, -w.y);
                    x = cmul(x, ws);
                    y = cmul(y, ws);
                }
                v[i][q] = x;
                u[i][q] = y;
            }
            dft_radix<R>(v[i], sign);
            dft_radix<R>(u[i], sign);
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < kB; ++i) {
        const int b = j + 64 * i;
        if (nb % 64 == 0 || i < kB - 1 || b < nb) {
            const int k = b % NS;
            const int d = (b - k) * R + k;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                buf0[lds_ix<SWO>(d + q * NS, L & ~7)] = v[i][q];
                buf1[lds_ix<SWO>(d + q * NS, L & ~7)] = u[i][q];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

template <int L, int S>
__device__ __forceinline__ void fft_ct_stages2(double2* buf0, double2* buf1, const double2* twl, int j, int sign) {
    if constexpr (ct_radix(L, S) != 0) {
        constexpr bool sw = L % 2 == 0;
        mr_stage_ct2<ct_radix(L, S), ct_ns(L, S), L, sw && S == 1, sw && S == 0>(buf0, buf1, twl, j, sign);
        fft_ct_stages2<L, S + 1>(buf0, buf1, twl, j, sign);
    }
}

// Two in-place FFTs of the same length by one wave (interleaved for a compile-time plan).
template <bool R7, int LM, int L>
__device__ __forceinline__ void fft2_wave_any(double2* buf0, double2* buf1, const double2* twl, const Factors& f, int j,
                                              int sign) {
    if constexpr (L > 0) {
        fft_ct_stages2<L, 0>(buf0, buf1, twl, j, sign);
    } else {
        fft_mr_wave<R7, LM>(buf0, twl, f, j, sign);
        fft_mr_wave<R7, LM>(buf1, twl, f, j, sign);
    }
}

// In-place FFT of one row / column by one wave: the compile-time plan when L > 0, else the
// run-time plan f (R7 / LM: see fft_mr_wave).
template <bool R7, int LM, int L>
__device__ __forceinline__ void fft_wave_any(double2* buf, const double2* twl, const Factors& f, int j, int sign) {
    if constexpr (L > 0)
        fft_ct_stages<L, 0>(buf, twl, j, sign);
    else
        fft_mr_wave<R7, LM>(buf, twl, f, j, sign);
}

// dst[i] = src[i * stride], i < count <= 64 IT, by the nt >= 64 threads (all loads issued before
// the LDS stores)
template <int IT>
__device__ __forceinline__ void stage_table(double2* dst, const double2* __restrict__ src, int count, int stride,
                                            int nt) {
    double2 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * nt;
        v[it] = i < count ? src[(size_t)i * stride] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i = threadIdx.x + it * nt;
        if (i < count) dst[i] = v[it];
    }
}

// host: lg of the power of two >= v (the plans' FFT lengths)
int ilog2(int64_t v) {
    int l = 0;
    while (((int64_t)1 << l) < v) ++l;
    return l;
}

}  // namespace

}  // namespace arx
