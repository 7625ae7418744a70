// arx_band_synth.hip -- band synthesis (arx_combine_bands, include/arx.h): each band's IR filtered with that
// band's FIR filter, the bands summed, one f32 IR pair written -- a direct form, because its bits are defined.
//
// A workgroup owns kTile consecutive outputs of one ear; a lane owns kR consecutive ones and keeps their kR
// accumulators of the current band in registers.  Bands run outermost (their sums are added in band order),
// a band's taps in chunks of up to kChunk, ascending.  Per chunk the workgroup stages in LDS, as f64, the
// chunk's taps and the input window its outputs need (the tile plus the chunk's halo; every global read
// clamped to [0, ir_len), zero outside); the next chunk's share is fetched into registers while this one's
// fmas run.  With d counting down from the chunk's last tap offset, output j of
// lane l reads window element l*kR + j + d: the window is kept as rows of kR elements, d = q*kR + r puts the
// kR outputs' operands into rows l+q and l+q+1, and a lane walks q downwards with those two rows in
// registers -- one row read per kR taps (kR*kR fmas), not one read per fma.  The rows and taps of kU steps
// are read together, so that later steps' reads are in flight while the first step's fmas run.  Rows have a
// pitch of kR + 2 doubles: 16-B aligned for ds_read_b128, and the 16 lanes of each of its groups land on 16
// distinct bank quads.  Tap reads are wave-uniform LDS broadcasts, staged so that a step's kR taps start on
// a 32-B boundary.
#include <hip/hip_runtime.h>

#include "arx_kernels.hpp"

namespace arx {
namespace {

constexpr int kR = 4;                 // outputs per lane
constexpr int kThreads = 64;          // one wave: 48 kHz x 2 s x 2 ears is 750 workgroups for 256 CUs x 4 SIMDs
constexpr int kTile = kR * kThreads;  // outputs per workgroup
constexpr int kChunk = 1024;          // taps staged at once (a multiple of kR)
constexpr int kPitch = kR + 2;        // doubles per window row in LDS
constexpr int kRows = kThreads + (kChunk - 1) / kR + 1;  // window rows 0 .. kThreads - 1 + (kChunk - 1) / kR + 1
constexpr int kU = 4;                 // steps whose LDS reads are issued together
static_assert(kR == 4, "rows and tap groups are read as two double2");
static_assert(kChunk % kR == 0, "a chunk is whole rows");

struct Row {
    double v[kR];
};
__device__ inline Row read4(const double* p) {  // p is 16-B aligned
    const double2 lo = *reinterpret_cast<const double2*>(p), hi = *reinterpret_cast<const double2*>(p + 2);
    return Row{{lo.x, lo.y, hi.x, hi.y}};
}

// kR taps g (ascending) against the rows a (l+q) and b (l+q+1): tap i pairs output j with element kR-1-i+j
__device__ inline void step(const Row& g, const Row& a, const Row& b, double (&acc)[kR]) {
#pragma unroll
    for (int i = 0; i < kR; ++i)
#pragma unroll
        for (int j = 0; j < kR; ++j) {
            const int e = kR - 1 - i + j;
            acc[j] = __builtin_fma(g.v[i], e < kR ? a.v[e] : b.v[e - kR], acc[j]);
        }
}

// A chunk of a band's taps, k0 .. k0 + kn - 1, as one workgroup sees it.  Window element w is input
// m = wbase + w; output j of lane l at tap k0 + kk reads w = l*kR + j + (kn-1-kk).  Tap kk is staged at
// gs[pad + kk], so that the whole steps' taps start at a multiple of kR.  live: some input of the window lies
// in [0, ir_len) -- a chunk whose window is all zeros leaves every accumulator's bits alone and is skipped.
struct Chunk {
    int kn, q0, r0, rows, pad;
    int64_t wbase;
    bool live;
};
__device__ inline Chunk chunk_of(const BandSynthArgs& p, int64_t n0, int k0) {
    Chunk ch;
    ch.kn = min(kChunk, p.taps - k0);
    ch.q0 = (ch.kn - 1) / kR;
    ch.r0 = (ch.kn - 1) % kR;
    ch.rows = kThreads + ch.q0 + 1;
    ch.pad = kR - 1 - ch.r0;
    ch.wbase = n0 + (p.taps - 1) / 2 - k0 - (ch.kn - 1);
    ch.live = ch.wbase < p.ir_len && ch.wbase + (int64_t)ch.rows * kR > 0;
    return ch;
}

// A lane's share of a chunk's window and taps on its way from global memory to LDS.
constexpr int kStageX = kRows * kR / kThreads, kStageG = kChunk / kThreads;
static_assert(kRows * kR % kThreads == 0 && kChunk % kThreads == 0, "whole rounds of the workgroup");
struct Staged {
    float x[kStageX];
    double g[kStageG];
};
// every global read clamped to the band's [0, ir_len) and to the chunk's taps
__device__ inline void fetch(const BandSynthArgs& p, const float* ir, int band, int k0, const Chunk& ch, int l, Staged& st) {
    const float* const x = ir + (int64_t)band * p.ir_len;
    const double* const g = p.filters + (int64_t)band * p.taps + k0;
#pragma unroll
    for (int i = 0; i < kStageX; ++i) {
        const int w = l + i * kThreads;
        const int64_t m = ch.wbase + w;
        st.x[i] = (w < ch.rows * kR && m >= 0 && m < p.ir_len) ? x[m] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < kStageG; ++i) {
        const int kk = l + i * kThreads;
        st.g[i] = kk < ch.kn ? g[kk] : 0.0;
    }
}
__device__ inline void store(const Chunk& ch, int l, const Staged& st, double* xs, double* gs) {
#pragma unroll
    for (int i = 0; i < kStageX; ++i) {
        const int w = l + i * kThreads;
        if (w < ch.rows * kR) xs[(w / kR) * kPitch + (w % kR)] = (double)st.x[i];
    }
#pragma unroll
    for (int i = 0; i < kStageG; ++i) {
        const int kk = l + i * kThreads;
        if (kk < ch.kn) gs[ch.pad + kk] = st.g[i];
    }
}

__global__ __launch_bounds__(kThreads) void band_synth_kernel(BandSynthArgs p) {
    __shared__ __align__(16) double xs[kRows * kPitch];
    __shared__ __align__(32) double gs[kChunk + kR];
    const int l = (int)threadIdx.x;
    const int ear = (int)blockIdx.y;
    const float* const ir = ear ? p.ir_right : p.ir_left;
    float* const out = ear ? p.out_right : p.out_left;
    const int64_t n0 = (int64_t)blockIdx.x * kTile;
    Staged st;
    bool have = false;  // st holds the chunk at hand, fetched while the one before was computed
    double s[kR];
    for (int band = 0; band < p.n_bands; ++band) {
        double acc[kR];
#pragma unroll
        for (int j = 0; j < kR; ++j) acc[j] = 0.0;
        for (int k0 = 0; k0 < p.taps; k0 += kChunk) {
            const Chunk ch = chunk_of(p, n0, k0);
            if (!ch.live) continue;
            if (!have) fetch(p, ir, band, k0, ch, l, st);
            __syncthreads();  // the chunk before has been read
            store(ch, l, st, xs, gs);
            __syncthreads();
            // the next live chunk, of this band or the next, is fetched while this one is computed
            int nb = band, nk = k0;
            for (have = false; !have;) {
                nk += kChunk;
                if (nk >= p.taps) {
                    nk = 0;
                    if (++nb >= p.n_bands) break;
                }
                have = chunk_of(p, n0, nk).live;
            }
            if (have) fetch(p, ir, nb, nk, chunk_of(p, n0, nk), l, st);
            const int q0 = ch.q0, r0 = ch.r0;
            const double* row = xs + (l + q0) * kPitch;
            Row a = read4(row), b = read4(row + kPitch);
            // the first, possibly partial, step: d = q0*kR + r0 down to q0*kR
#pragma unroll
            for (int r = kR - 1; r >= 0; --r) {
                if (r <= r0) {
                    const double gk = gs[kR - 1 - r];  // = gs[pad + (r0 - r)]
#pragma unroll
                    for (int j = 0; j < kR; ++j) acc[j] = __builtin_fma(gk, r + j < kR ? a.v[r + j] : b.v[r + j - kR], acc[j]);
                }
            }
            // whole steps, kU at a time: their rows and taps are read together, ahead of the fmas
            const double* gp = gs + kR;
            int q = q0 - 1;
            for (; q >= kU - 1; q -= kU) {
                Row x_[kU], g_[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    x_[u] = read4(row - (u + 1) * kPitch);
                    g_[u] = read4(gp + u * kR);
                }
                step(g_[0], x_[0], a, acc);
#pragma unroll
                for (int u = 1; u < kU; ++u) step(g_[u], x_[u], x_[u - 1], acc);
                a = x_[kU - 1];
                row -= kU * kPitch;
                gp += kU * kR;
            }
            for (; q >= 0; --q) {
                b = a;
                row -= kPitch;
                a = read4(row);
                step(read4(gp), a, b, acc);
                gp += kR;
            }
        }
#pragma unroll
        for (int j = 0; j < kR; ++j) s[j] = band == 0 ? acc[j] : s[j] + acc[j];
    }
#pragma unroll
    for (int j = 0; j < kR; ++j) {
        const int64_t n = n0 + (int64_t)l * kR + j;
        if (n < p.ir_len) out[n] = (float)s[j];
    }
}

}  // namespace

hipError_t launch_band_synth(const BandSynthArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.ir_len + kTile - 1) / kTile), 2);
    hipLaunchKernelGGL(band_synth_kernel, grid, dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace arx
