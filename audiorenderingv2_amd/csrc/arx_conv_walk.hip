// arx_conv_walk.hip -- walk-through convolution for gfx950: a whole signal against a per-block IR
// schedule in one pass (arx_convolute_walk, include/arx.h).
//
// The arithmetic of every output block is the streaming convolution's (arx_conv_stream.hip): the same
// N-point LDS FFTs by 1024 threads, the same fma nest over the partitions p = 0 .. P-1, the same scale and
// the same blend, so the output has the bits of the loop of arx_set_ir_device + arx_stream_process_device
// over the blocks.  What differs is that the whole input is known, so nothing runs block after block:
//   ir    G_u[p] = FFT_N(h_u[pB, (p+1)B))         grid (P x distinct IRs the schedule names)
//   fwd   X_b    = FFT_N(in[(b+1)B - N, (b+1)B))  grid (blocks); outside [0, n_frames) reads as 0
//   mac   Z_i    = sum_p X_(b_i - p) * G_(u_i)[p] grid (tiles of items x bins), below
//   inv   y_i    = IFFT_N(Z_i)[N - B, N) * scale  grid (items)
//   blend out_b  = fma(w, y_cur - y_prev, y_prev) grid (fade x transition blocks)
// An item is (block, IR): every block is one with its own IR, and a transition block (its IR differs
// from the block before and a fade is on) is a second one with the previous block's IR, placed in front
// of it so that it continues the run of items of that IR.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "arx_conv_fft.hpp"
#include "arx_conv_stream_common.hpp"
#include "arx_kernels.hpp"

namespace arx {

namespace {

constexpr int kWalkAcc = 16;       // accumulators per lane of the MAC: the most items of one pass
constexpr int kWalkMacThreads = 256;

// stream_ir_kernel for distinct IR u = blockIdx.x / P, partition p = blockIdx.x % P.
__global__ __launch_bounds__(kStreamThreads) void walk_ir_kernel(const float* __restrict__ hl_all,
                                                                 const float* __restrict__ hr_all, int32_t n, int32_t B,
                                                                 int32_t N, int32_t lgN, int32_t P,
                                                                 const double2* __restrict__ tw, double2* __restrict__ G) {
    extern __shared__ double2 buf[];
    const int u = blockIdx.x / P;
    const int p = blockIdx.x - u * P;
    const float* __restrict__ hl = hl_all + (size_t)u * n;
    const float* __restrict__ hr = hr_all + (size_t)u * n;
    for (int i = threadIdx.x; i < N; i += kStreamThreads) {
        const int64_t k = (int64_t)p * B + i;
        buf[i] = (i < B && k < n) ? make_double2((double)hl[k], (double)hr[k]) : make_double2(0.0, 0.0);
    }
    const TwSplit twf = stream_twiddles(buf, N, lgN, tw);
    __syncthreads();
    lds_fft_t(buf, N, lgN, -1, threadIdx.x, kStreamThreads, twf, N);
    double2* __restrict__ g = G + (size_t)blockIdx.x * N;
    for (int i = threadIdx.x; i < N; i += kStreamThreads) g[i] = buf[i];
}

// X_b of block b = blockIdx.x: the window the stream's history and block would hold at that point --
// the N input frames that end with the block, zero before frame 0 and from n_frames on.
__global__ __launch_bounds__(kStreamThreads) void walk_fwd_kernel(const double* __restrict__ in, int64_t n_frames,
                                                                  int32_t B, int32_t N, int32_t lgN,
                                                                  const double2* __restrict__ tw,
                                                                  double2* __restrict__ X) {
    extern __shared__ double2 buf[];
    const int64_t first = ((int64_t)blockIdx.x + 1) * B - N;
    for (int i = threadIdx.x; i < N; i += kStreamThreads) {
        const int64_t f = first + i;
        buf[i] = make_double2((f >= 0 && f < n_frames) ? in[f] : 0.0, 0.0);
    }
    const TwSplit twf = stream_twiddles(buf, N, lgN, tw);
    __syncthreads();
    lds_fft_t(buf, N, lgN, -1, threadIdx.x, kStreamThreads, twf, N);
    double2* __restrict__ x = X + (size_t)blockIdx.x * N;
    for (int i = threadIdx.x; i < N; i += kStreamThreads) x[i] = buf[i];
}

// The walk MAC.  Workgroup (t, c): the items [t * tile, (t + 1) * tile) at the bins [256 c, 256 c + 256),
// one lane per bin, in passes of up to kWalkAcc items with one accumulator each.  Per accumulator the
// order is stream_mac_kernel's: p ascending from 0, acc = fma nest of X_(b - p) and G[p], a block before
// the first contributing +0 as the stream's zeroed ring does.  The items of a pass are consecutive, so
// their blocks span at most as many rows as the pass has items: a ring of `rows` (a power of two >=
// the pass) X rows per lane lives in LDS (each lane reads and writes only its own column, so no
// barrier), step p brings in the one row X_(bmin - p), and a pass reads items + P - 1 rows of X where
// items * P would be read one by one.  G[p] is loaded once per run of items of one IR (the IR of an
// item is uniform over the workgroup: a scalar branch).
__global__ __launch_bounds__(kWalkMacThreads) void walk_mac_kernel(const double2* __restrict__ X,
                                                                   const double2* __restrict__ G,
                                                                   const int32_t* __restrict__ item_block,
                                                                   const int32_t* __restrict__ item_ir, int32_t n_items,
                                                                   int32_t tile, int32_t rows, int32_t P, int32_t N,
                                                                   double2* __restrict__ Z) {
    extern __shared__ double2 win[];  // rows x 256
    const int k = blockIdx.y * kWalkMacThreads + threadIdx.x;
    if (k >= N) return;
    const int mask = rows - 1;
    double2* __restrict__ col = win + threadIdx.x;
    const int t0 = blockIdx.x * tile;
    const int t1 = min(t0 + tile, n_items);
    for (int s0 = t0; s0 < t1; s0 += kWalkAcc) {
        const int n = min(kWalkAcc, t1 - s0);
        int ib[kWalkAcc], ig[kWalkAcc];
#pragma unroll
        for (int i = 0; i < kWalkAcc; ++i) {
            ib[i] = i < n ? item_block[s0 + i] : 0;
            ig[i] = i < n ? item_ir[s0 + i] : -1;
        }
        const int bmin = item_block[s0], bmax = item_block[s0 + n - 1];
        double2 acc[kWalkAcc];
#pragma unroll
        for (int i = 0; i < kWalkAcc; ++i) acc[i] = make_double2(0.0, 0.0);
        for (int r = bmin + 1; r <= bmax; ++r) col[(r & mask) * kWalkMacThreads] = X[(size_t)r * N + k];
        double2 xin = X[(size_t)bmin * N + k];  // the row step p brings in: X_(bmin - p)
        for (int p = 0; p < P; ++p) {
            col[((bmin - p) & mask) * kWalkMacThreads] = xin;
            const int next = bmin - p - 1;  // asked for now, stored by the next step
            if (p + 1 < P) xin = next >= 0 ? X[(size_t)next * N + k] : make_double2(0.0, 0.0);
            double2 g = make_double2(0.0, 0.0);
#pragma unroll
            for (int i = 0; i < kWalkAcc; ++i) {
                if (i < n) {
                    if (i == 0 || ig[i] != ig[i - 1]) g = G[((size_t)ig[i] * P + p) * N + k];
                    const double2 x = col[((ib[i] - p) & mask) * kWalkMacThreads];
                    acc[i].x = fma(x.x, g.x, fma(-x.y, g.y, acc[i].x));
                    acc[i].y = fma(x.x, g.y, fma(x.y, g.x, acc[i].y));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kWalkAcc; ++i)
            if (i < n) Z[(size_t)(s0 + i) * N + k] = acc[i];
    }
}

// stream_inv_kernel / stream_inv2_kernel for item i = blockIdx.x: an item of a block's own IR writes the
// block's B frames to out, the previous IR's item of transition t its first F frames to yprev[t].
__global__ __launch_bounds__(kStreamThreads) void walk_inv_kernel(const double2* __restrict__ Z,
                                                                  const int32_t* __restrict__ item_block,
                                                                  const int32_t* __restrict__ item_trans, int32_t B,
                                                                  int32_t N, int32_t lgN, const double2* __restrict__ tw,
                                                                  double scale, int32_t F, double* __restrict__ yprev,
                                                                  double* __restrict__ out) {
    extern __shared__ double2 buf[];
    const double2* __restrict__ z = Z + (size_t)blockIdx.x * N;
    for (int i = threadIdx.x; i < N; i += kStreamThreads) buf[i] = z[i];
    const TwSplit twf = stream_twiddles(buf, N, lgN, tw);
    __syncthreads();
    lds_fft_t(buf, N, lgN, +1, threadIdx.x, kStreamThreads, twf, N);
    const int t = item_trans[blockIdx.x];
    const bool cur = t < 0;
    double* __restrict__ dst = cur ? out + 2 * (size_t)item_block[blockIdx.x] * B : yprev + 2 * (size_t)t * F;
    const int n = cur ? B : F;
    for (int i = threadIdx.x; i < n; i += kStreamThreads) {
        const double2 v = buf[N - B + i];
        dst[2 * i] = v.x * scale;
        dst[2 * i + 1] = v.y * scale;
    }
}

// stream_blend_kernel for transition t = blockIdx.x, on that block's first F frames.
__global__ __launch_bounds__(256) void walk_blend_kernel(const double* __restrict__ yprev, const double* __restrict__ w,
                                                         const int32_t* __restrict__ trans_block, int32_t B, int32_t F,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= 2 * F) return;
    const double p = yprev[2 * (size_t)blockIdx.x * F + i];
    double* __restrict__ o = out + 2 * (size_t)trans_block[blockIdx.x] * B;
    o[i] = fma(w[i >> 1], o[i] - p, p);
}

uint64_t up256(uint64_t v) { return (v + 255) & ~255ull; }

}  // namespace

WalkLayout walk_layout(int32_t ir_len, int32_t block, uint64_t irs_used, uint64_t n_blocks, uint64_t n_transitions,
                       int32_t fade) {
    const StreamShape sh = stream_shape(ir_len, block);
    WalkLayout l{};
    l.B = sh.B;
    l.N = sh.N;
    l.lgN = sh.lgN;
    l.P = sh.P;
    l.scale = sh.scale;
    const uint64_t spec = (uint64_t)sh.N * sizeof(double2), items = n_blocks + n_transitions;
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t here = at;
        at += up256(bytes);
        return here;
    };
    l.tw = take(spec);
    l.w = take((uint64_t)fade * 8);
    l.G = take(irs_used * (uint64_t)sh.P * spec);
    l.X = take(n_blocks * spec);
    l.Z = take(items * spec);
    l.yprev = take(n_transitions * 2 * (uint64_t)fade * 8);
    l.irs = take(irs_used * 2 * (uint64_t)ir_len * 4);
    l.in = take(n_blocks * (uint64_t)block * 8);
    l.out = take(n_blocks * 2 * (uint64_t)block * 8);
    l.tables = take(items * 16);
    l.total = at;
    return l;
}

void walk_twiddle_table(int32_t N, std::vector<double>& out) {
    const std::vector<double2> tw = stream_twiddle_table(N);
    out.resize(2 * (size_t)N);
    std::memcpy(out.data(), tw.data(), out.size() * sizeof(double));
}

int32_t walk_tile_rows(int32_t tile) {
    int32_t rows = 1;
    while (rows < std::min(tile, kWalkAcc)) rows <<= 1;
    return rows;
}

hipError_t launch_walk(const WalkArgs& a, hipStream_t s) {
    (void)hipGetLastError();  // report this launch's error, not a stale one
    const WalkLayout& l = a.layout;
    if (a.n_blocks <= 0 || a.n_used <= 0 || a.n_transitions < 0 || a.tile < 1 || a.n_frames < 0 ||
        a.n_frames > (int64_t)a.n_blocks * l.B || (a.n_transitions > 0 && (a.fade < 1 || a.fade > l.B)) ||
        (int64_t)a.n_used * l.P > INT32_MAX || (int64_t)a.n_blocks + a.n_transitions > INT32_MAX)
        return hipErrorInvalidValue;
    char* base = static_cast<char*>(a.scratch);
    const double2* tw = reinterpret_cast<const double2*>(base + l.tw);
    double2* G = reinterpret_cast<double2*>(base + l.G);
    double2* X = reinterpret_cast<double2*>(base + l.X);
    double2* Z = reinterpret_cast<double2*>(base + l.Z);
    double* yprev = reinterpret_cast<double*>(base + l.yprev);
    double* out = reinterpret_cast<double*>(base + l.out);
    const float* irl = reinterpret_cast<const float*>(base + l.irs);
    const int32_t n_items = a.n_blocks + a.n_transitions;
    const int32_t* item_block = reinterpret_cast<const int32_t*>(base + l.tables);
    const int32_t* item_ir = item_block + n_items;
    const int32_t* item_trans = item_ir + n_items;
    const int32_t* trans_block = item_trans + n_items;
    const size_t lds = stream_lds(l.N);
    hipLaunchKernelGGL(walk_ir_kernel, dim3((unsigned)(a.n_used * l.P)), dim3(kStreamThreads), lds, s, irl,
                       irl + (size_t)a.n_used * a.ir_len, a.ir_len, l.B, l.N, l.lgN, l.P, tw, G);
    hipLaunchKernelGGL(walk_fwd_kernel, dim3((unsigned)a.n_blocks), dim3(kStreamThreads), lds, s,
                       reinterpret_cast<const double*>(base + l.in), a.n_frames, l.B, l.N, l.lgN, tw, X);
    const int32_t rows = walk_tile_rows(a.tile);
    const unsigned tiles = (unsigned)((n_items + a.tile - 1) / a.tile);
    hipLaunchKernelGGL(walk_mac_kernel, dim3(tiles, (unsigned)((l.N + kWalkMacThreads - 1) / kWalkMacThreads)),
                       dim3(kWalkMacThreads), (size_t)rows * kWalkMacThreads * sizeof(double2), s, X, G, item_block, item_ir,
                       n_items, a.tile, rows, l.P, l.N, Z);
    hipLaunchKernelGGL(walk_inv_kernel, dim3((unsigned)n_items), dim3(kStreamThreads), lds, s, Z, item_block, item_trans,
                       l.B, l.N, l.lgN, tw, l.scale, a.fade, yprev, out);
    if (a.n_transitions > 0)
        hipLaunchKernelGGL(walk_blend_kernel, dim3((unsigned)a.n_transitions, (unsigned)((2 * a.fade + 255) / 256)),
                           dim3(256), 0, s, yprev, reinterpret_cast<const double*>(base + l.w), trans_block, l.B, a.fade,
                           out);
    return hipGetLastError();
}

}  // namespace arx
