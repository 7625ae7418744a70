// arx_conv_stream_common.hpp -- what the streaming convolution's kernels (arx_conv_stream.hip) and the
// walk-through convolution's (arx_conv_walk.hip) share: the workgroup size of their single-workgroup
// LDS FFTs, the twiddle tables those stage in LDS, the LDS they need, and the plan's sizes, scale and
// twiddle table.  Both files run lds_fft_t (arx_conv_fft.hpp) with these, so a block has the same bits
// from either.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "arx_conv_fft.hpp"

namespace arx {
namespace {

constexpr int kStreamThreads = 1024;  // lds_fft needs >= N/16 threads

// The stream kernels' twiddles: W_N^e = hi[e >> 6] * lo[e & 63] from two small tables staged in LDS
// after the N-point buffer (a global table lookup per butterfly put an L2 round trip into every
// stage of these single-workgroup FFTs).
__device__ __forceinline__ TwSplit stream_twiddles(double2* lds, int32_t N, int32_t lgN, const double2* __restrict__ tw) {
    const int lgLo = lgN < 6 ? lgN : 6;
    double2* hi = lds + N;
    double2* lo = hi + (N >> lgLo);
    for (int i = threadIdx.x; i < (N >> lgLo); i += kStreamThreads) hi[i] = tw[(size_t)i << lgLo];
    for (int i = threadIdx.x; i < (1 << lgLo); i += kStreamThreads) lo[i] = tw[i];
    return TwSplit{hi, lo, lgLo, N};
}
static size_t stream_lds(int32_t N) { return ((size_t)N + (size_t)(N >> 4) + 64) * sizeof(double2); }

// A plan's sizes for ir_len frames in blocks of `block`: N = the power of two >= 2 * block (at least
// 16), P = ceil(ir_len / block), and the output scale (unnormalised IFFT, / (ir_len/2)).
struct StreamShape {
    int32_t B, N, lgN, P;
    double scale;
};
static StreamShape stream_shape(int32_t ir_len, int32_t block) {
    StreamShape s;
    s.B = block;
    s.lgN = std::max(ilog2(2 * (int64_t)block), 4);
    s.N = 1 << s.lgN;
    s.P = (int32_t)(((int64_t)ir_len + block - 1) / block);
    s.scale = (double)ir_len / ((double)s.N * (double)(ir_len / 2));
    return s;
}

// W_N^e, e < N (the table stream_twiddles splits).
static std::vector<double2> stream_twiddle_table(int32_t N) {
    std::vector<double2> tw((size_t)N);
    const long double two_pi = 6.283185307179586476925286766559L;
    for (int64_t e = 0; e < N; ++e) {
        const long double ang = two_pi * (long double)e / (long double)N;
        tw[(size_t)e] = make_double2((double)cosl(ang), -(double)sinl(ang));
    }
    return tw;
}

}  // namespace
}  // namespace arx
