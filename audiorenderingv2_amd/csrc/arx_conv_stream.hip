// arx_conv_stream.hip -- streaming convolution for gfx950 (the FFT device code: arx_conv_fft.hpp).
//
// Streaming convolution for the RtAudio duplex callback: uniformly
// partitioned overlap-save (UPOLS) in f64, replacing the reference's per-callback full-length
// circular convolution (AudioRenderer.cpp:593-661, kernels.cu:345-377) whose 2*ir_len outputs the
// CircularBuffer then wraps onto itself (main.cpp:189-195).  Per block of B frames:
//   fwd  X_b = FFT_N(last N input samples)                   (one workgroup, LDS, N <= 8192)
//   mac  Z   = sum_p X_(b-p) * G_p,  G_p = FFT_N(hL_p + i hR_p), h_p = h[pB, (p+1)B) zero padded
//   inv  y_L + i y_R = IFFT_N(Z)[N-B, N)                     (one workgroup, LDS)
// N = the power of two >= 2B, P = ceil(ir_len / B).  Because h_L and h_R are real, one complex
// spectrum per partition (G_p) and one inverse FFT serve both ears.  Output: B frames zipped L/R,
// scaled like the reference's live path, ir_len / (ir_len/2) x the linear convolution
// (normalizeBuffers, kernels.cu:450-467), but without the circular wrap and the CircularBuffer
// aliasing.  The frequency-domain delay line keeps input spectra, so a new IR (a moving listener)
// needs no restart.  Without a crossfade it takes over at the next block boundary (a step from
// x * h_old to x * h_new within one sample); with one (stream_set_fade) the plan keeps the previous
// block's partition spectra as well, and the first block of a new IR -- a transition block -- is
// computed with both sets from the same delay line and blended in the time domain:
//   mac2 Z_prev, Z_cur = sum_p X_(b-p) * {G_prev, G_cur}_p   (X read once)
//   inv  y_prev, y_cur by one workgroup each;  y = fma(w[i], y_cur - y_prev, y_prev), i < F;  y_cur after
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "arx_conv_fft.hpp"
#include "arx_conv_stream_common.hpp"
#include "arx_kernels.hpp"

namespace arx {

struct StreamPlan {
    int32_t B = 0, N = 0, lgN = 0, P = 0, n = 0;
    int64_t blocks = 0;           // processed since reset (slot of block b = b % P)
    double2* d_tw = nullptr;      // W_N^e
    double2* d_G = nullptr;       // P * N partition spectra (G_cur)
    double2* d_Gprev = nullptr;   // the previous block's, once a crossfade was enabled
    double2* d_X = nullptr;       // P * N input spectra ring (frequency-domain delay line)
    double2* d_Z = nullptr;       // 2 * N accumulated spectra: [0, N) plain / previous IR, [N, 2N) current IR
    double* d_w = nullptr;        // B crossfade weights (the first fade of them in use), with d_Gprev
    double* d_yprev = nullptr;    // 2 * B: the previous IR's first fade output frames, zipped (transition blocks)
    int32_t fade = 0;             // crossfade frames, 0 = hard switch
    std::vector<double> h_w;      // the upload's source
    double* d_hist = nullptr;     // N - B input history
    double scale = 0.0;
};

namespace {

// G_p = FFT_N(hL[pB + i] + i hR[pB + i], i < B, zero padded): one workgroup per partition.
__global__ __launch_bounds__(kStreamThreads) void stream_ir_kernel(const float* __restrict__ hl,
                                                                   const float* __restrict__ hr, int32_t n,
                                                                   int32_t B, int32_t N, int32_t lgN,
                                                                   const double2* __restrict__ tw,
                                                                   double2* __restrict__ G) {
    extern __shared__ double2 buf[];
    const int p = blockIdx.x;
    for (int i = threadIdx.x; i < N; i += kStreamThreads) {
        const int64_t k = (int64_t)p * B + i;
        buf[i] = (i < B && k < n) ? make_double2((double)hl[k], (double)hr[k]) : make_double2(0.0, 0.0);
    }
    const TwSplit twf = stream_twiddles(buf, N, lgN, tw);
    __syncthreads();
    lds_fft_t(buf, N, lgN, -1, threadIdx.x, kStreamThreads, twf, N);
    for (int i = threadIdx.x; i < N; i += kStreamThreads) G[(size_t)p * N + i] = buf[i];
}

// X_b = FFT_N([history (N - B), block (B)]), history <- the window's last N - B samples.
__global__ __launch_bounds__(kStreamThreads) void stream_fwd_kernel(const double* __restrict__ in, int32_t n_in,
                                                                    double* __restrict__ hist, int32_t B, int32_t N,
                                                                    int32_t lgN, const double2* __restrict__ tw,
                                                                    double2* __restrict__ X) {
    extern __shared__ double2 buf[];
    const int H = N - B;
    for (int i = threadIdx.x; i < N; i += kStreamThreads) {
        double v;
        if (i < H) v = hist[i];
        else v = (i - H < n_in) ? in[i - H] : 0.0;
        buf[i] = make_double2(v, 0.0);
    }
    const TwSplit twf = stream_twiddles(buf, N, lgN, tw);
    __syncthreads();
    for (int i = threadIdx.x; i < H; i += kStreamThreads) hist[i] = buf[i + B].x;
    lds_fft_t(buf, N, lgN, -1, threadIdx.x, kStreamThreads, twf, N);  // (its first barrier orders the reads above)
    for (int i = threadIdx.x; i < N; i += kStreamThreads) X[i] = buf[i];
}

// Z[k] = sum_p X_((b - p) mod P)[k] * G_p[k]: one thread per bin, coalesced over k.
__global__ __launch_bounds__(256) void stream_mac_kernel(const double2* __restrict__ X, const double2* __restrict__ G,
                                                         int32_t P, int32_t N, int32_t newest,
                                                         double2* __restrict__ Z) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    double2 acc = make_double2(0.0, 0.0);
    int slot = newest;
    for (int p = 0; p < P; ++p) {
        const double2 x = X[(size_t)slot * N + k];
        const double2 g = G[(size_t)p * N + k];
        acc.x = fma(x.x, g.x, fma(-x.y, g.y, acc.x));
        acc.y = fma(x.x, g.y, fma(x.y, g.x, acc.y));
        slot = slot == 0 ? P - 1 : slot - 1;
    }
    Z[k] = acc;
}

// The transition block's MAC: Z[k] against G_prev and Z[N + k] against G_cur in one pass over the
// X ring.  Per accumulator the partition order and the fmas are stream_mac_kernel's, so Z[N + k] has
// the bits the plain MAC would give with G_cur (and Z[k] too when the two sets are equal).
__global__ __launch_bounds__(256) void stream_mac2_kernel(const double2* __restrict__ X,
                                                          const double2* __restrict__ Gprev,
                                                          const double2* __restrict__ Gcur, int32_t P, int32_t N,
                                                          int32_t newest, double2* __restrict__ Z) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    double2 a0 = make_double2(0.0, 0.0), a1 = make_double2(0.0, 0.0);
    int slot = newest;
    for (int p = 0; p < P; ++p) {
        const double2 x = X[(size_t)slot * N + k];
        const double2 g0 = Gprev[(size_t)p * N + k];
        const double2 g1 = Gcur[(size_t)p * N + k];
        a0.x = fma(x.x, g0.x, fma(-x.y, g0.y, a0.x));
        a0.y = fma(x.x, g0.y, fma(x.y, g0.x, a0.y));
        a1.x = fma(x.x, g1.x, fma(-x.y, g1.y, a1.x));
        a1.y = fma(x.x, g1.y, fma(x.y, g1.x, a1.y));
        slot = slot == 0 ? P - 1 : slot - 1;
    }
    Z[k] = a0;
    Z[(size_t)N + k] = a1;
}

// y_L + i y_R = IFFT_N(Z)[N - B, N), zipped and scaled.
__global__ __launch_bounds__(kStreamThreads) void stream_inv_kernel(const double2* __restrict__ Z, int32_t B,
                                                                    int32_t N, int32_t lgN,
                                                                    const double2* __restrict__ tw, double scale,
                                                                    double* __restrict__ out) {
    extern __shared__ double2 buf[];
    for (int i = threadIdx.x; i < N; i += kStreamThreads) buf[i] = Z[i];
    const TwSplit twf = stream_twiddles(buf, N, lgN, tw);
    __syncthreads();
    lds_fft_t(buf, N, lgN, +1, threadIdx.x, kStreamThreads, twf, N);
    for (int i = threadIdx.x; i < B; i += kStreamThreads) {
        const double2 v = buf[N - B + i];
        out[2 * i] = v.x * scale;
        out[2 * i + 1] = v.y * scale;
    }
}

// The transition block's inverse, two workgroups, one per spectrum (two N = 8192 buffers do not fit
// one CU's LDS, and one workgroup doing both in turn takes 1.39 x the plain block):
// workgroup 1 writes y_cur = IFFT_N(Z[N, 2N))[N - B, N) to out exactly as stream_inv_kernel would,
// workgroup 0 the first F frames of y_prev = IFFT_N(Z[0, N))[N - B, N), scaled too, to yprev.
__global__ __launch_bounds__(kStreamThreads) void stream_inv2_kernel(const double2* __restrict__ Z, int32_t B,
                                                                     int32_t N, int32_t lgN,
                                                                     const double2* __restrict__ tw, double scale,
                                                                     int32_t F, double* __restrict__ yprev,
                                                                     double* __restrict__ out) {
    extern __shared__ double2 buf[];
    const bool cur = blockIdx.x == 1;
    const double2* __restrict__ z = Z + (cur ? (size_t)N : 0);
    for (int i = threadIdx.x; i < N; i += kStreamThreads) buf[i] = z[i];
    const TwSplit twf = stream_twiddles(buf, N, lgN, tw);
    __syncthreads();
    lds_fft_t(buf, N, lgN, +1, threadIdx.x, kStreamThreads, twf, N);
    double* __restrict__ dst = cur ? out : yprev;
    const int n = cur ? B : F;
    for (int i = threadIdx.x; i < n; i += kStreamThreads) {
        const double2 v = buf[N - B + i];
        dst[2 * i] = v.x * scale;
        dst[2 * i + 1] = v.y * scale;
    }
}

// out[i] <- fma(w[i], y_cur - y_prev, y_prev) on the first F frames (one thread per ear of a frame).
// The difference stays unfused (fp contract off): y_cur == y_prev then leaves exactly y_prev.
__global__ __launch_bounds__(256) void stream_blend_kernel(const double* __restrict__ yprev, const double* __restrict__ w,
                                                           int32_t F, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * F) return;
    const double p = yprev[i];
    out[i] = fma(w[i >> 1], out[i] - p, p);
}

}  // namespace

StreamPlan* stream_plan_create(int32_t ir_len, int32_t block, int device, char* err, size_t errlen) {
    auto bad = [&](const char* m) -> StreamPlan* {
        if (err && errlen) std::snprintf(err, errlen, "%s", m);
        return nullptr;
    };
    if (ir_len <= 0 || block <= 0 || block > 4096) return bad("stream block must be in [1, 4096] frames");
    StreamPlan* p = new StreamPlan();
    const StreamShape sh = stream_shape(ir_len, block);
    p->B = block;
    p->lgN = sh.lgN;
    p->N = sh.N;
    p->P = sh.P;
    p->n = ir_len;
    p->scale = sh.scale;
    hipSetDevice(device);
    const std::vector<double2> tw = stream_twiddle_table(p->N);
    const size_t spec = (size_t)p->P * p->N * sizeof(double2);
    if (hipMalloc(&p->d_tw, (size_t)p->N * sizeof(double2)) != hipSuccess || hipMalloc(&p->d_G, spec) != hipSuccess ||
        hipMalloc(&p->d_X, spec) != hipSuccess || hipMalloc(&p->d_Z, 2 * (size_t)p->N * sizeof(double2)) != hipSuccess ||
        hipMalloc(&p->d_hist, (size_t)(p->N - p->B + 1) * sizeof(double)) != hipSuccess ||
        hipMemcpy(p->d_tw, tw.data(), (size_t)p->N * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(p->d_G, 0, spec) != hipSuccess) {
        stream_plan_destroy(p);
        return bad("device allocation failed");
    }
    if (stream_reset(p, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        stream_plan_destroy(p);
        return bad("stream reset failed");
    }
    return p;
}

void stream_plan_destroy(StreamPlan* p) {
    if (!p) return;
    hipFree(p->d_tw);
    hipFree(p->d_G);
    hipFree(p->d_Gprev);
    hipFree(p->d_w);
    hipFree(p->d_yprev);
    hipFree(p->d_X);
    hipFree(p->d_Z);
    hipFree(p->d_hist);
    delete p;
}

hipError_t stream_reset(StreamPlan* p, hipStream_t s) {
    p->blocks = 0;
    hipError_t e = hipMemsetAsync(p->d_X, 0, (size_t)p->P * p->N * sizeof(double2), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_hist, 0, (size_t)(p->N - p->B + 1) * sizeof(double), s);
    return e;
}

hipError_t stream_set_fade(StreamPlan* p, int32_t fade_frames, const double* h_w, hipStream_t s) {
    if (fade_frames < 0 || fade_frames > p->B || (fade_frames > 0 && !h_w)) return hipErrorInvalidValue;
    if (fade_frames > 0) {
        const size_t spec = (size_t)p->P * p->N * sizeof(double2);
        if (!p->d_w && hipMalloc(&p->d_w, (size_t)p->B * sizeof(double)) != hipSuccess) return hipErrorOutOfMemory;
        if (!p->d_yprev && hipMalloc(&p->d_yprev, 2 * (size_t)p->B * sizeof(double)) != hipSuccess) return hipErrorOutOfMemory;
        if (!p->d_Gprev) {
            if (hipMalloc(&p->d_Gprev, spec) != hipSuccess) return hipErrorOutOfMemory;
            const hipError_t e = hipMemsetAsync(p->d_Gprev, 0, spec, s);
            if (e != hipSuccess) return e;
        }
        p->h_w.assign(h_w, h_w + fade_frames);  // kept: the copy below may read it after this call returns
        const hipError_t e =
            hipMemcpyAsync(p->d_w, p->h_w.data(), (size_t)fade_frames * sizeof(double), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
    }
    p->fade = fade_frames;
    return hipSuccess;
}

hipError_t stream_set_ir(StreamPlan* p, const float* d_ir_left, const float* d_ir_right, bool keep_previous,
                         hipStream_t s) {
    (void)hipGetLastError();  // report this launch's error, not a stale one
    if (keep_previous) {
        if (!p->d_Gprev) return hipErrorInvalidValue;
        std::swap(p->d_G, p->d_Gprev);  // the set the last block used becomes G_prev; the other is rebuilt
    }
    hipLaunchKernelGGL(stream_ir_kernel, dim3(p->P), dim3(kStreamThreads), stream_lds(p->N), s, d_ir_left,
                       d_ir_right, p->n, p->B, p->N, p->lgN, p->d_tw, p->d_G);
    return hipGetLastError();
}

hipError_t stream_run(StreamPlan* p, const double* d_in, int64_t n_in, double* d_out_interleaved, hipStream_t s) {
    (void)hipGetLastError();  // report this launch's error, not a stale one
    if (n_in < 0 || n_in > p->B) return hipErrorInvalidValue;
    const int32_t slot = (int32_t)(p->blocks % p->P);
    const size_t lds = stream_lds(p->N);
    hipLaunchKernelGGL(stream_fwd_kernel, dim3(1), dim3(kStreamThreads), lds, s, d_in, (int32_t)n_in, p->d_hist, p->B,
                       p->N, p->lgN, p->d_tw, p->d_X + (size_t)slot * p->N);
    hipLaunchKernelGGL(stream_mac_kernel, dim3((unsigned)((p->N + 255) / 256)), dim3(256), 0, s, p->d_X, p->d_G, p->P,
                       p->N, slot, p->d_Z);
    hipLaunchKernelGGL(stream_inv_kernel, dim3(1), dim3(kStreamThreads), lds, s, p->d_Z, p->B, p->N, p->lgN, p->d_tw,
                       p->scale, d_out_interleaved);
    ++p->blocks;
    return hipGetLastError();
}

hipError_t stream_run_xfade(StreamPlan* p, const double* d_in, int64_t n_in, double* d_out_interleaved, hipStream_t s) {
    (void)hipGetLastError();  // report this launch's error, not a stale one
    if (n_in < 0 || n_in > p->B || p->fade <= 0 || p->fade > p->B || !p->d_Gprev || !p->d_w || !p->d_yprev)
        return hipErrorInvalidValue;
    const int32_t slot = (int32_t)(p->blocks % p->P);
    const size_t lds = stream_lds(p->N);
    hipLaunchKernelGGL(stream_fwd_kernel, dim3(1), dim3(kStreamThreads), lds, s, d_in, (int32_t)n_in, p->d_hist, p->B,
                       p->N, p->lgN, p->d_tw, p->d_X + (size_t)slot * p->N);
    hipLaunchKernelGGL(stream_mac2_kernel, dim3((unsigned)((p->N + 255) / 256)), dim3(256), 0, s, p->d_X, p->d_Gprev,
                       p->d_G, p->P, p->N, slot, p->d_Z);
    hipLaunchKernelGGL(stream_inv2_kernel, dim3(2), dim3(kStreamThreads), lds, s, p->d_Z, p->B, p->N, p->lgN, p->d_tw,
                       p->scale, p->fade, p->d_yprev, d_out_interleaved);
    hipLaunchKernelGGL(stream_blend_kernel, dim3((unsigned)((2 * p->fade + 255) / 256)), dim3(256), 0, s, p->d_yprev,
                       p->d_w, p->fade, d_out_interleaved);
    ++p->blocks;
    return hipGetLastError();
}

int32_t stream_plan_block(const StreamPlan* p) { return p ? p->B : 0; }
int64_t stream_plan_blocks(const StreamPlan* p) { return p ? p->blocks : 0; }
int32_t stream_plan_fade(const StreamPlan* p) { return p ? p->fade : 0; }
int32_t stream_plan_partitions(const StreamPlan* p) { return p ? p->P : 0; }
int32_t stream_plan_fft(const StreamPlan* p) { return p ? p->N : 0; }

}  // namespace arx
