// arx_trace_device.hpp -- the device code of a closest-hit query, shared by the trace program
// (arx_trace.hip) and the replay family (arx_replay.hip): ray set-up, the node and leaf steps of
// the software traversal, the traversal stacks, the triangle test and shade().  Included by those
// two files only; everything has internal linkage, so each of them compiles its own copy.  Part of
// the trace kernel's identity (build.py TRACE_KERNEL_FILES).
#pragma once
#include <hip/hip_runtime.h>

#include "arx_layout.hpp"

#ifndef ARX_TRACE_BITFLOAT
#define ARX_TRACE_BITFLOAT 1  // 16-bit planes as the float 2^23 + q built by v_perm (0: u16 -> f32 conversions)
#endif
#ifndef ARX_TRACE_SIGNSEL
#define ARX_TRACE_SIGNSEL 1  // per-ray near/far plane selection in the 16-bit node step (0: min / max per slab)
#endif

namespace arx {
namespace {

#ifndef ARX_TRACE_NCACHE
#define ARX_TRACE_NCACHE 0
#endif
// Top-of-tree node cache: the 16-bit path copies quantized nodes [0, kNodeCache) (the top node, then
// the scene tree's breadth-first prefix, bfs_prefix_order) into LDS at launch and reads them from
// there.  Those nodes take a large share of the node steps (arx_debug_wide_stats [16..31]) and
// would otherwise be L1 hits that still cost the TD its per-lane cycles.  The node buffer always
// holds >= 1025 nodes (ensure_device_scene allocates n_nodes + 1024), so the copy stays in bounds.
constexpr int kNodeCache = ARX_TRACE_NCACHE;
static_assert(kNodeCache >= 0 && kNodeCache <= 1024, "node cache: at most the buffer's 1024 spare nodes");

// ------------------------------------------------------------------- RNG ---
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0;
        const uint32_t n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
    }
}

__device__ __forceinline__ float u01(uint32_t x) { return (float)((x >> 8) + 1u) * (1.0f / 16777216.0f); }

// cos/sin(2*pi*u), u in (0,1]: exact quadrant reduction in turns + fma Horner (same
// coefficients and order as the oracle, so the result is bitwise identical).
__device__ __forceinline__ void sincos_turns(double u, double& s_out, double& c_out) {
    const double a = 4.0 * u;
    const double q = floor(a);
    const double f = a - q;
    const int iq = ((int)q) & 3;
    const double r = f * 1.5707963267948966;
    const double r2 = r * r;
    double ps = -1.0 / 121645100408832000.0;
    ps = __fma_rn(ps, r2, 1.0 / 355687428096000.0);
    ps = __fma_rn(ps, r2, -1.0 / 1307674368000.0);
    ps = __fma_rn(ps, r2, 1.0 / 6227020800.0);
    ps = __fma_rn(ps, r2, -1.0 / 39916800.0);
    ps = __fma_rn(ps, r2, 1.0 / 362880.0);
    ps = __fma_rn(ps, r2, -1.0 / 5040.0);
    ps = __fma_rn(ps, r2, 1.0 / 120.0);
    ps = __fma_rn(ps, r2, -1.0 / 6.0);
    const double sr = __fma_rn(r * r2, ps, r);
    double pc = 1.0 / 2432902008176640000.0;
    pc = __fma_rn(pc, r2, -1.0 / 6402373705728000.0);
    pc = __fma_rn(pc, r2, 1.0 / 20922789888000.0);
    pc = __fma_rn(pc, r2, -1.0 / 87178291200.0);
    pc = __fma_rn(pc, r2, 1.0 / 479001600.0);
    pc = __fma_rn(pc, r2, -1.0 / 3628800.0);
    pc = __fma_rn(pc, r2, 1.0 / 40320.0);
    pc = __fma_rn(pc, r2, -1.0 / 720.0);
    pc = __fma_rn(pc, r2, 1.0 / 24.0);
    pc = __fma_rn(pc, r2, -1.0 / 2.0);
    const double cr = __fma_rn(r2, pc, 1.0);
    double c, s;
    if (iq == 0) {
        c = cr;
        s = sr;
    } else if (iq == 1) {
        c = -sr;
        s = cr;
    } else if (iq == 2) {
        c = -cr;
        s = -sr;
    } else {
        c = sr;
        s = -cr;
    }
    s_out = s;
    c_out = c;
}

// devicePrograms.cu:216-224 with Philox(seed, ray id) instead of curand(clock64(), tid).
__device__ __forceinline__ float3 ray_direction(uint64_t seed, uint64_t rid) {
    uint32_t c0 = (uint32_t)rid, c1 = (uint32_t)(rid >> 32), c2 = 0u, c3 = 0u;
    philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u1 = u01(c0);
    const float u2 = u01(c1);
    const double cz = 2.0 * (double)u2 - 1.0;
    const double sz = __dsqrt_rn(1.0 - cz * cz);
    double st, ct;
    sincos_turns((double)u1, st, ct);
    return make_float3((float)(sz * ct), (float)(sz * st), (float)cz);
}

// ------------------------------------------------------------ geometry ---
struct Ray {
    float o[3];      // origin
    float op[3];     // origin permuted (kx, ky, kz)
    float inv[3];    // safe reciprocal direction (box test only)
    float sx, sy, sz;
    int kx, ky, kz;
    uint32_t nsel[3];  // v_perm selectors per axis: the near plane (ARX_TRACE_SIGNSEL, node_step)
#if ARX_TRACE_BITFLOAT
    uint32_t fsel[3];  // ... and the far plane
#endif
};

__device__ __forceinline__ float sel3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__device__ __forceinline__ void setup_ray(Ray& r, float3 o, float3 d) {
    r.o[0] = o.x;
    r.o[1] = o.y;
    r.o[2] = o.z;
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const int kz = (ax > ay) ? ((ax > az) ? 0 : 2) : ((ay > az) ? 1 : 2);
    int kx = kz + 1;
    if (kx == 3) kx = 0;
    int ky = kx + 1;
    if (ky == 3) ky = 0;
    const float dkz = sel3(d.x, d.y, d.z, kz);
    if (dkz < 0.0f) {
        const int t = kx;
        kx = ky;
        ky = t;
    }
    r.kx = kx;
    r.ky = ky;
    r.kz = kz;
    r.sx = sel3(d.x, d.y, d.z, kx) / dkz;
    r.sy = sel3(d.x, d.y, d.z, ky) / dkz;
    r.sz = 1.0f / dkz;
    r.op[0] = sel3(o.x, o.y, o.z, kx);
    r.op[1] = sel3(o.x, o.y, o.z, ky);
    r.op[2] = sel3(o.x, o.y, o.z, kz);
    // Box-test reciprocals: v_rcp_f32 (1 ulp) instead of a correctly rounded division -- the
    // slab test only has to be conservative, and a 1e-7 relative error in t is far inside the
    // 1e-5 * max|coordinate| box padding; the closest hit comes from the exact triangle test.
    const float dd[3] = {d.x, d.y, d.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = dd[k];
        if (fabsf(v) < 1e-20f) v = (v < 0.0f) ? -1e-20f : 1e-20f;
        r.inv[k] = __builtin_amdgcn_rcpf(v);
#if ARX_TRACE_BITFLOAT
        // a (lo | hi << 16) plane word: near = lo for a positive reciprocal, hi for a negative one;
        // bytes 4-5 (lo) or 6-7 (hi) of {word, 2^23} under 2^23's upper bytes 2-3
        r.nsel[k] = r.inv[k] >= 0.0f ? 0x03020504u : 0x03020706u;
        r.fsel[k] = r.inv[k] >= 0.0f ? 0x03020706u : 0x03020504u;
#else
        // a (lo | hi << 16) plane word: keep for a positive reciprocal (lo is the near plane), swap
        // the halves for a negative one
        r.nsel[k] = r.inv[k] >= 0.0f ? 0x03020100u : 0x01000302u;
#endif
    }
}

// The closest hit so far of one query: t, triangle id (tie-break), the TriRec's unit (-1 none) and
// the test's V, W and det, so shade() needs no second triangle test.
struct Best {
    float t;
    int id;
    int unit;
    float v, w, det;
};

// Watertight ray/triangle test (Woop, Benthin, Wald 2013), t >= 0 (optixTrace tmin 0), and the
// closest-hit update (ties to the lowest id) for a lane where `valid`.  Vertex components are selected
// by (kx,ky,kz) then differenced against the permuted origin: the same values as A[k] = v[k] - o[k]
// indexed afterwards (oracle order).  Branch-free: the early exits of the textbook form and an
// if-based update left the compiler shuffling the Best fields between registers at every join
// (DESIGN.md section 6.3).
__device__ __forceinline__ void take_hit(const Ray& r, float4 p0, float4 p1, float4 p2, int unit, Best& b,
                                         bool valid) {
    const float Ax = sel3(p0.x, p0.y, p0.z, r.kx) - r.op[0];
    const float Ay = sel3(p0.x, p0.y, p0.z, r.ky) - r.op[1];
    const float Az = sel3(p0.x, p0.y, p0.z, r.kz) - r.op[2];
    const float Bx = sel3(p1.x, p1.y, p1.z, r.kx) - r.op[0];
    const float By = sel3(p1.x, p1.y, p1.z, r.ky) - r.op[1];
    const float Bz = sel3(p1.x, p1.y, p1.z, r.kz) - r.op[2];
    const float Cx = sel3(p2.x, p2.y, p2.z, r.kx) - r.op[0];
    const float Cy = sel3(p2.x, p2.y, p2.z, r.ky) - r.op[1];
    const float Cz = sel3(p2.x, p2.y, p2.z, r.kz) - r.op[2];
    const float ax = Ax - r.sx * Az;
    const float ay = Ay - r.sy * Az;
    const float bx = Bx - r.sx * Bz;
    const float by = By - r.sy * Bz;
    const float cx = Cx - r.sx * Cz;
    const float cy = Cy - r.sy * Cz;
    const float U = cx * by - cy * bx;
    const float V = ax * cy - ay * cx;
    const float W = bx * ay - by * ax;
    const bool edge = !(((U < 0.0f) | (V < 0.0f) | (W < 0.0f)) & ((U > 0.0f) | (V > 0.0f) | (W > 0.0f)));
    const float det = U + V + W;
    const float az = r.sz * Az;
    const float bz = r.sz * Bz;
    const float cz = r.sz * Cz;
    const float T = U * az + V * bz + W * cz;
    const float t = T / det;
    const int id = __float_as_int(p1.w);
    const bool take = valid & edge & (det != 0.0f) & (t >= 0.0f) & ((t < b.t) | ((t == b.t) & (id < b.id)));
    b.t = take ? t : b.t;
    b.id = take ? id : b.id;
    b.unit = take ? unit : b.unit;
    b.v = take ? V : b.v;
    b.w = take ? W : b.w;
    b.det = take ? det : b.det;
}

// glm-style helpers (glm::dot is x*x + y*y + z*z left to right)
__device__ __forceinline__ float dot3(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 add3(float3 a, float3 b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ float3 scale3(float s, float3 a) { return make_float3(s * a.x, s * a.y, s * a.z); }

__device__ __forceinline__ void hist_add(unsigned long long* h, int k, float e, double inv_unit) {
    const long long q = __double2ll_rn((double)e * inv_unit);
    if (q != 0) atomicAdd(h + k, (unsigned long long)q);
}

// Per-lane ray state (PRD, PRD.h:5-14, minus the pointer plumbing).
struct RayState {
    float3 pos, dir;
    float e, dist;
    int depth;
};

// Loop guard of __raygen__renderFrame (devicePrograms.cu:233-236).
__device__ __forceinline__ bool wants_query(const TraceArgs& a, const RayState& s) {
    return s.dist < a.dist_limit && s.e > a.energy_thres && s.depth >= 0 && (uint32_t)s.depth < a.max_bounces;
}

__device__ __forceinline__ void ray_init(const TraceArgs& a, RayState& s, uint64_t rid) {
    // ray_direction(a.seed, rid), precomputed by the launcher's pre-pass (dirs_kernel)
    const float4 d = reinterpret_cast<const float4*>(a.dirs)[rid - a.ray_begin];
    s.dir = make_float3(d.x, d.y, d.z);
    s.pos = make_float3(a.emitter[0], a.emitter[1], a.emitter[2]);
    s.e = a.e0;
    s.dist = 0.0f;
    s.depth = 0;
    if (!(s.dir.x != 0.0f || s.dir.y != 0.0f || s.dir.z != 0.0f)) s.depth = -1;  // :230, no trace
}

// __closesthit__radiance (devicePrograms.cu:62-180) for TriRec `hit`, or __miss__radiance
// (:186-190) when hit < 0.  r is the ray the query was traced with.  HIST false (the path cache's recording
// instance): a hit on a receiver-marked triangle ends the ray and counts as everywhere else, but adds
// nothing to the histogram, which that instance does not have.
template <bool HIST = true>
__device__ __forceinline__ void shade(const TraceArgs& a, const float4* __restrict__ tbase, RayState& s, const Ray& r,
                                      const Best& best, uint32_t& n_rx, uint32_t& n_miss) {
    const int hit = best.unit;
    if (hit < 0) {
        ++n_miss;
        s.depth = -1;
        return;
    }
    const float4* tp = tbase + hit;  // hit = the triangle's 16-B unit (leaf_step)
    const float4 p0 = tp[0], p1 = tp[1], p2 = tp[2];
    const float3 P1 = make_float3(p0.x, p0.y, p0.z);
    const float3 P2 = make_float3(p1.x, p1.y, p1.z);
    const float3 P3 = make_float3(p2.x, p2.y, p2.z);
    const float ab = p0.w;
    // Ng = normalize(cross(P2-P1, P3-P1))  (:75-77)
    const float3 U = sub3(P2, P1), V = sub3(P3, P1);
    const float3 cr = make_float3(U.y * V.z - V.y * U.z, U.z * V.x - V.z * U.x, U.x * V.y - V.x * U.y);
    const float hv = best.v, hw = best.w, hdet = best.det;
    const float bu = hv / hdet;
    const float bv = hw / hdet;
    const float w0 = (1.0f - bu) - bv;
    const float3 P = add3(add3(scale3(w0, P1), scale3(bu, P2)), scale3(bv, P3));  // :81
    const float3 seg = sub3(P, s.pos);
    s.dist += sqrtf(dot3(seg, seg));  // :83
    float e = s.e;
    if (ab < 0.0f) {  // receiver chord weighting, r = 1 (:91-122)
        const float3 center = make_float3(a.center[0], a.center[1], a.center[2]);
        const float3 nd = scale3(1.0f / sqrtf(dot3(s.dir, s.dir)), s.dir);
        const float3 oc = sub3(P, center);
        const float qa = dot3(nd, nd);
        const float qb = 2.0f * dot3(oc, nd);
        const float qc = dot3(oc, oc) - 1.0f;
        const float disc = qb * qb - (4.0f * qa) * qc;
        if (disc <= 0.0f) {
            e = 0.0f;
        } else {
            const float sq = sqrtf(disc);
            const float t1 = (-qb - sq) / (2.0f * qa);
            const float t2 = (-qb + sq) / (2.0f * qa);
            const float3 i1 = add3(P, scale3(t1, nd));
            const float3 i2 = add3(P, scale3(t2, nd));
            const float3 di = sub3(i1, i2);
            e = e * sqrtf(dot3(di, di));
        }
    }
    if (ab == -1.0f || ab == -2.0f) {  // receiver halves (:128-170)
        ++n_rx;
        const int k = (int)roundf((s.dist / (float)kSpeedOfSound) * (float)a.sample_rate);
        if (HIST && k < a.ir_len) {
            unsigned long long* hl = a.hist;
            unsigned long long* hr = a.hist + a.ir_len;
            unsigned long long* own = (ab == -1.0f) ? hl : hr;
            unsigned long long* other = (ab == -1.0f) ? hr : hl;
            hist_add(own, k, e, a.inv_unit);
            if (!a.is_mono) {
                const int kk = (k + a.delay < a.ir_len) ? k + a.delay : k;
                hist_add(other, kk, e * (1.0f - a.hrtf), a.inv_unit);
            }
        }
        s.depth = -1;
    } else {  // specular reflection + absorption (:173-175)
        // reflection about the unnormalised normal, dir - (2 (dir . cr) / (cr . cr)) cr: the same
        // mirror as with normalize(cr) (:75-77, :173) for one division, no square root
        const float s2 = (2.0f * dot3(s.dir, cr)) / dot3(cr, cr);
        s.dir = sub3(s.dir, scale3(s2, cr));
        e = e * (1.0f - ab);
        ++s.depth;
    }
    s.e = e;
    s.pos = add3(P, scale3(1e-3f, s.dir));  // :179
}

__device__ __forceinline__ void flush_counters(const TraceArgs& a, uint32_t n_q, uint32_t n_rx, uint32_t n_miss,
                                               int lane) {
    unsigned int vq = n_q, vr = n_rx, vm = n_miss;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        vq += __shfl_xor(vq, off, 64);
        vr += __shfl_xor(vr, off, 64);
        vm += __shfl_xor(vm, off, 64);
    }
    if ((lane & 63) == 0) {
        if (vq) atomicAdd(a.counters + 0, (unsigned long long)vq);
        if (vr) atomicAdd(a.counters + 1, (unsigned long long)vr);
        if (vm) atomicAdd(a.counters + 2, (unsigned long long)vm);
    }
}
// ------------------------------------------------------------ traversal ---
// Per-lane state of one closest-hit query over the two-level BVH (node 0 = top node).
// node: the lane's next stack entry -- >= 0 an inner node, <= -2 a pending leaf
// ~(first*16 + count), -1 done.  Empty children carry a 0-triangle leaf code (kEmptyChildCode).
struct Trav {
    Best best;  // closest hit so far
    int node;
    int sp;    // stack depth
};

// Traversal stack of one lane.  LDS: ROWS entries at stk[slot * BLOCK + lane].  Global (trees
// deeper than the LDS rows): a column of bvh_depth + 1 entries at gstack[slot * lanes + gid],
// coalesced across the wave like the LDS rows.  A stack holds at most one entry per tree level,
// so rows > bvh_depth never overflows.
// Both give the step two accessors: below(sp) reads the entry a pop would take (slot sp - 1; any
// value when sp == 0) and put(sp, v) writes slot sp, the one above the top.
//   LdsStack: slot s lives in row s + 1 and row 0 is a dummy, so below(sp) is row sp and put(sp) is
//   row sp + 1: one address for both (the write's +1 row is the instruction's offset), no clamps --
//   the launcher takes this stack only for trees with bvh_depth + 1 <= ROWS, and a stack holds at
//   most one entry per level.
//   kSentinel: below(0) is -1 (LdsStack's dummy row, written once per launch), so a pop needs no
//   empty-stack test.
template <int BLOCK, int ROWS>
struct LdsStack {
    static constexpr bool kSentinel = true;
    int* base;  // &stk[lane]
    __device__ __forceinline__ int below(int sp) const { return base[sp * BLOCK]; }
    __device__ __forceinline__ void put(int sp, int v) const { base[(sp + 1) * BLOCK] = v; }
};
struct GlobalStack {
    static constexpr bool kSentinel = false;
    int* base;  // &gstack[gid]
    uint64_t stride;
    int nrows;
    __device__ __forceinline__ int below(int sp) const { return base[(uint64_t)max(sp - 1, 0) * stride]; }
    __device__ __forceinline__ void put(int sp, int v) const { base[(uint64_t)min(sp, nrows - 1) * stride] = v; }
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, short stride = 0) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), stride, 0x7fffffff, 0x00020000);
}

// lanes in a wave mask, as a 32-bit scalar (two s_bcnt1_i32_b32): compares against it stay on the SALU
__device__ __forceinline__ uint32_t lanes32(unsigned long long m) {
    return (uint32_t)__builtin_popcount((uint32_t)m) + (uint32_t)__builtin_popcount((uint32_t)(m >> 32));
}
#ifndef ARX_TRACE_IDXEN
#define ARX_TRACE_IDXEN 1  // QNode2 loads indexed by node (idxen, a 32-B stride resource): no address VALU (C3 -1.6 %, profiles/r05/ab_idxen.txt); 0: byte offsets
#endif
typedef int arx_i32x4 __attribute__((ext_vector_type(4)));
// buffer_load_dwordx4 ... idxen: address = base + vindex * stride + voffset + inst offset (the
// hardware's structured-buffer addressing; clang has no builtin for it, the LLVM intrinsic is bound
// by name as composable_kernel's amd_buffer_addressing.hpp does for the raw forms)
__device__ arx_i32x4 arx_struct_buffer_load_b128(__amdgpu_buffer_rsrc_t rsrc, int vindex, int voffset, int soffset,
                                                 int aux) __asm("llvm.amdgcn.struct.ptr.buffer.load.v4i32");
#ifndef ARX_TRACE_SFETCH
#define ARX_TRACE_SFETCH 0  // design experiment: the wave leader's node by one scalar load (see node_step)
#endif
typedef int arx_i32x8 __attribute__((ext_vector_type(8)));
// s_buffer_load_dwordx8 (a scalar LOAD through the scalar data cache; the descriptor as 4 SGPRs)
__device__ arx_i32x8 arx_s_buffer_load_b256(arx_i32x4 rsrc, int offset, int aux) __asm("llvm.amdgcn.s.buffer.load.v8i32");
// the quantized nodes' descriptor as four scalars (the scalar-load experiment, ARX_TRACE_SFETCH)
__device__ __forceinline__ arx_i32x4 qnodes_rsrc4(const QNode2* qnodes) {
    const unsigned long long qa = (unsigned long long)qnodes;
    arx_i32x4 qrs;
    qrs.x = (int)(uint32_t)qa;
    qrs.y = (int)((qa >> 32) & 0xffffu);
    qrs.z = 0x7fffffff;
    qrs.w = 0x00020000;
    return qrs;
}
__device__ __forceinline__ uint4 node_half(__amdgpu_buffer_rsrc_t rs, int node, int half) {
#if ARX_TRACE_IDXEN
    const arx_i32x4 v = arx_struct_buffer_load_b128(rs, node, half * 16, 0, 0);
    return make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
#else
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, node * (int)sizeof(QNode2) + half * 16, 0, 0));
#endif
}

// One branch-free node step: test both children of t.node, continue with the nearer hit child,
// push the farther one, or pop when neither is hit.  Entries are popped at the end of a step,
// so the only guard is t.node >= 0; everything inside is a select (bitwise & / | on the bools:
// && / || compile back to exec-mask branches).
//   Q16: 32-B QNode2 (two 16-B buffer loads).  A slab plane is grid.origin + q * grid.scale, so
//        t = q * (scale*inv) + (origin - o)*inv: the caller passes ix = scale*inv and
//        oix = (o - origin)*inv per axis, and each plane is one u16 -> f32 conversion and one fma.
//        Conservative: the f32 error of that form is below 5 * 2^-24 * (grid extent) * |inv| for
//        origins on the grid, far below the 0.1-step outward margin of every quantized plane
//        (quantize_nodes16; the launcher checks the emitter is on the grid).
//   f32: the coded BvhNode (56 of its 64 B), ix = inv, oix = o*inv.
//   SKIP0: child 0 counts as missed whatever its box (replay_kernel enters the receiver sub-tree by a
//   step on the top node that leaves the scene, child 0, alone).
template <int FMT, typename Stack, bool PIN = true, bool SKIP0 = false>
__device__ __forceinline__ void node_step(const Ray& r, float oix, float oiy, float oiz, Trav& t, const Stack& stk,
                                          __amdgpu_buffer_rsrc_t rs, const uint4* __restrict__ ncache,
                                          arx_i32x4 qrs) {
    constexpr bool Q16 = FMT == kFmtQ16;
    // the pop candidate is read first, so its latency hides under the node fetch (slot sp - 1 is
    // not touched by this step's write to slot sp)
    const int sp = t.sp;
    const int sp_pop = max(sp - 1, 0);
    int top = stk.below(sp);
    const float ix = r.inv[0], iy = r.inv[1], iz = r.inv[2];
    float4 na, nb, nc;
    int c0, c1;
    uint4 A = make_uint4(0u, 0u, 0u, 0u), B = A;
    if constexpr (Q16) {
        if constexpr (kNodeCache > 0) {
            // every lane reads the LDS copy (clamped index; a few cycles per wave) and only the
            // lanes below the cached prefix skip the global fetch: separate registers for the two,
            // so the LDS reads never wait behind the buffer loads
            const bool cached = t.node < kNodeCache;
            uint4 Ag = make_uint4(0u, 0u, 0u, 0u), Bg = Ag;
            if (!cached) {
                const int off = t.node * (int)sizeof(QNode2);
                Ag = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
                Bg = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0));
            }
            const int ci = 2 * min(t.node, kNodeCache - 1);
            const uint4 Al = ncache[ci], Bl = ncache[ci + 1];
            A = make_uint4(cached ? Al.x : Ag.x, cached ? Al.y : Ag.y, cached ? Al.z : Ag.z, cached ? Al.w : Ag.w);
            B = make_uint4(cached ? Bl.x : Bg.x, cached ? Bl.y : Bg.y, cached ? Bl.z : Bg.z, cached ? Bl.w : Bg.w);
        } else {
#if ARX_TRACE_SFETCH
            // the wave leader's node (the first lane stepping) by one scalar load, no vector-memory
            // (TD) work; only the lanes at another node issue the two 16-B vector loads
            const int lead = __builtin_amdgcn_readfirstlane(t.node);
            const arx_i32x8 sn = arx_s_buffer_load_b256(qrs, lead * (int)sizeof(QNode2), 0);
            if (t.node != lead) {
                A = node_half(rs, t.node, 0);
                B = node_half(rs, t.node, 1);
            } else {
                A = make_uint4((uint32_t)sn.s0, (uint32_t)sn.s1, (uint32_t)sn.s2, (uint32_t)sn.s3);
                B = make_uint4((uint32_t)sn.s4, (uint32_t)sn.s5, (uint32_t)sn.s6, (uint32_t)sn.s7);
            }
#else
            A = node_half(rs, t.node, 0);
            B = node_half(rs, t.node, 1);
#endif
        }
        na = make_float4((float)(A.x & 0xffffu), (float)(A.x >> 16), (float)(A.y & 0xffffu), (float)(A.y >> 16));
        nb = make_float4((float)(B.x & 0xffffu), (float)(B.x >> 16), (float)(B.y & 0xffffu), (float)(B.y >> 16));
        nc = make_float4((float)(A.z & 0xffffu), (float)(A.z >> 16), (float)(B.z & 0xffffu), (float)(B.z >> 16));
        c0 = (int)A.w;
        c1 = (int)B.w;
    } else {
        const int off = t.node * (int)sizeof(BvhNode);
        na = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        nb = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0));
        nc = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 32, 0, 0));
        const int2 d = __builtin_bit_cast(int2, __builtin_amdgcn_raw_buffer_load_b64(rs, off + 48, 0, 0));
        c0 = d.x;
        c1 = d.y;
    }
    float tn0, tf0, tn1, tf1;
    if constexpr (Q16 && ARX_TRACE_SIGNSEL) {
        // near / far planes picked per ray (the reciprocal's sign) by a byte permute of each plane
        // word: no min / max per slab.  The fma is monotone in q, so the near plane's t is the
        // min of the two and the result is the min / max form's, bit for bit; an empty child's
        // (1, 0) planes come out near > far on either sign.
#if ARX_TRACE_BITFLOAT
        // Each plane straight from its bits: v_perm puts the near (far) 16-bit half under the
        // exponent byte of 2^23, giving the float 2^23 + q exactly, and oix here is
        // C = fma(2^23, ix, (o - origin) * inv) (trace_kernel): t = fma(2^23 + q, ix, -C) is
        // q * ix - (o - origin) * inv up to C's rounding, <= 0.504 step, which the kQ16Margin
        // outward rounding of every plane covers (arx_layout.hpp).  No int -> float conversions.
        auto pl = [](uint32_t w, uint32_t sel) { return __uint_as_float(__builtin_amdgcn_perm(w, 0x4B000000u, sel)); };
        const float nx0 = __builtin_fmaf(pl(A.x, r.nsel[0]), ix, -oix), fx0 = __builtin_fmaf(pl(A.x, r.fsel[0]), ix, -oix);
        const float ny0 = __builtin_fmaf(pl(A.y, r.nsel[1]), iy, -oiy), fy0 = __builtin_fmaf(pl(A.y, r.fsel[1]), iy, -oiy);
        const float nz0 = __builtin_fmaf(pl(A.z, r.nsel[2]), iz, -oiz), fz0 = __builtin_fmaf(pl(A.z, r.fsel[2]), iz, -oiz);
        const float nx1 = __builtin_fmaf(pl(B.x, r.nsel[0]), ix, -oix), fx1 = __builtin_fmaf(pl(B.x, r.fsel[0]), ix, -oix);
        const float ny1 = __builtin_fmaf(pl(B.y, r.nsel[1]), iy, -oiy), fy1 = __builtin_fmaf(pl(B.y, r.fsel[1]), iy, -oiy);
        const float nz1 = __builtin_fmaf(pl(B.z, r.nsel[2]), iz, -oiz), fz1 = __builtin_fmaf(pl(B.z, r.fsel[2]), iz, -oiz);
#else
        const uint32_t ax = __builtin_amdgcn_perm(A.x, A.x, r.nsel[0]), ay = __builtin_amdgcn_perm(A.y, A.y, r.nsel[1]);
        const uint32_t az = __builtin_amdgcn_perm(A.z, A.z, r.nsel[2]), bxw = __builtin_amdgcn_perm(B.x, B.x, r.nsel[0]);
        const uint32_t byw = __builtin_amdgcn_perm(B.y, B.y, r.nsel[1]), bzw = __builtin_amdgcn_perm(B.z, B.z, r.nsel[2]);
        const float nx0 = __builtin_fmaf((float)(ax & 0xffffu), ix, -oix), fx0 = __builtin_fmaf((float)(ax >> 16), ix, -oix);
        const float ny0 = __builtin_fmaf((float)(ay & 0xffffu), iy, -oiy), fy0 = __builtin_fmaf((float)(ay >> 16), iy, -oiy);
        const float nz0 = __builtin_fmaf((float)(az & 0xffffu), iz, -oiz), fz0 = __builtin_fmaf((float)(az >> 16), iz, -oiz);
        const float nx1 = __builtin_fmaf((float)(bxw & 0xffffu), ix, -oix), fx1 = __builtin_fmaf((float)(bxw >> 16), ix, -oix);
        const float ny1 = __builtin_fmaf((float)(byw & 0xffffu), iy, -oiy), fy1 = __builtin_fmaf((float)(byw >> 16), iy, -oiy);
        const float nz1 = __builtin_fmaf((float)(bzw & 0xffffu), iz, -oiz), fz1 = __builtin_fmaf((float)(bzw >> 16), iz, -oiz);
#endif
        tn0 = fmaxf(fmaxf(fmaxf(nx0, ny0), nz0), 0.0f);
        tf0 = fminf(fminf(fminf(fx0, fy0), fz0), t.best.t);
        tn1 = fmaxf(fmaxf(fmaxf(nx1, ny1), nz1), 0.0f);
        tf1 = fminf(fminf(fminf(fx1, fy1), fz1), t.best.t);
    } else {
        const float x00 = __builtin_fmaf(na.x, ix, -oix), x01 = __builtin_fmaf(na.y, ix, -oix);
        const float y00 = __builtin_fmaf(na.z, iy, -oiy), y01 = __builtin_fmaf(na.w, iy, -oiy);
        const float z00 = __builtin_fmaf(nc.x, iz, -oiz), z01 = __builtin_fmaf(nc.y, iz, -oiz);
        const float x10 = __builtin_fmaf(nb.x, ix, -oix), x11 = __builtin_fmaf(nb.y, ix, -oix);
        const float y10 = __builtin_fmaf(nb.z, iy, -oiy), y11 = __builtin_fmaf(nb.w, iy, -oiy);
        const float z10 = __builtin_fmaf(nc.z, iz, -oiz), z11 = __builtin_fmaf(nc.w, iz, -oiz);
        tn0 = fmaxf(fmaxf(fminf(x00, x01), fminf(y00, y01)), fmaxf(fminf(z00, z01), 0.0f));
        tf0 = fminf(fminf(fmaxf(x00, x01), fmaxf(y00, y01)), fminf(fmaxf(z00, z01), t.best.t));
        tn1 = fmaxf(fmaxf(fminf(x10, x11), fminf(y10, y11)), fmaxf(fminf(z10, z11), 0.0f));
        tf1 = fminf(fminf(fmaxf(x10, x11), fmaxf(y10, y11)), fminf(fmaxf(z10, z11), t.best.t));
    }
    const bool h0 = SKIP0 ? false : tn0 <= tf0, h1 = tn1 <= tf1;
    const bool near1 = h1 & (!h0 | (tn1 < tn0));
    const int c_near = near1 ? c1 : c0;
    const int c_far = near1 ? c0 : c1;
    stk.put(sp, c_far);  // above the top of the stack unless pushed
    // PIN: an empty asm keeps the pop read unconditional (no branch around it); the small-launch
    // instance leaves it to the compiler, which keeps it unconditional too, without the asm's s_nop
    if constexpr (PIN) asm volatile("" : "+v"(top));
    const bool any = h0 | h1, both = h0 & h1;
    if constexpr (Stack::kSentinel) {  // row 0 holds -1: a pop of the empty stack ends the query
        // near1 -> c1; else h0 -> c0; else neither child was hit (near1 is false only with !h1 or h0)
        t.node = near1 ? c1 : (h0 ? c0 : top);
        t.sp = sp + (h0 ? 0 : -1) + (int)h1;  // push, continue or pop; -1 only once the query is done
    } else {
        t.node = any ? c_near : (sp > 0 ? top : -1);
        t.sp = any ? (both ? sp + 1 : sp) : sp_pop;
    }
}

// CW4 step (arx_layout.hpp): one 32-B node = two 16-B loads for four children.  Plane q of axis k
// is 4*o_k + q*2^e_k grid quanta, so t = fma(q, ix*2^e, fma(o, 4*ix, -oix)) (ix*2^e exact): the
// Q16 slab arithmetic with the frame folded in.  The hit children are sorted by entry distance
// (a 5-exchange network), the nearest is taken and the others are pushed farthest first.  Up to
// three pushes per step: the stack rows above ROWS live in the global overflow column (deep
// trees; the hot path never touches it while every lane's stack stays below ROWS - 3).
__device__ __forceinline__ void cas(float& ka, int& va, float& kb, int& vb) {
    const bool sw = kb < ka;
    const float k0 = sw ? kb : ka, k1 = sw ? ka : kb;
    const int v0 = sw ? vb : va, v1 = sw ? va : vb;
    ka = k0;
    kb = k1;
    va = v0;
    vb = v1;
}

template <int S>
__device__ __forceinline__ float w4_plane(const uint32_t (&w)[5]) {
    return (float)((w[S / 5] >> (6 * (S % 5))) & 63u);
}

template <int C>
__device__ __forceinline__ float w4_child(const uint32_t (&w)[5], float sx, float bx, float sy, float by, float sz,
                                          float bz, float best_t, float& tf_out) {
    const float x0 = __builtin_fmaf(w4_plane<6 * C + 0>(w), sx, bx), x1 = __builtin_fmaf(w4_plane<6 * C + 1>(w), sx, bx);
    const float y0 = __builtin_fmaf(w4_plane<6 * C + 2>(w), sy, by), y1 = __builtin_fmaf(w4_plane<6 * C + 3>(w), sy, by);
    const float z0 = __builtin_fmaf(w4_plane<6 * C + 4>(w), sz, bz), z1 = __builtin_fmaf(w4_plane<6 * C + 5>(w), sz, bz);
    tf_out = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), best_t));
    return fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
}

template <int BLOCK, int ROWS>
struct W4Stack {
    static constexpr bool kSentinel = false;
    int* lds;        // &stk[lane]
    int* glob;       // &gstack[gid]: rows ROWS.. (overflow)
    uint64_t stride;
    __device__ __forceinline__ int read(int slot) const {
        return slot < ROWS ? lds[slot * BLOCK] : glob[(uint64_t)(slot - ROWS) * stride];
    }
    __device__ __forceinline__ void write(int slot, int v) const {
        if (slot < ROWS) lds[slot * BLOCK] = v;
        else glob[(uint64_t)(slot - ROWS) * stride] = v;
    }
    __device__ __forceinline__ int below(int sp) const { return read(max(sp - 1, 0)); }
};

template <typename Stack>
__device__ __forceinline__ void node_step_w4(const Ray& r, float oix, float oiy, float oiz, Trav& t, const Stack& stk,
                                             __amdgpu_buffer_rsrc_t rs) {
    const int sp = t.sp;
    const int sp_pop = max(sp - 1, 0);
    int top = stk.read(sp_pop);
    const int off = t.node * 16;
    const uint4 A = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
    const uint4 B = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 0));
    const float ix = r.inv[0], iy = r.inv[1], iz = r.inv[2];
    const float sx = __builtin_ldexpf(ix, (int)(A.x >> 28));
    const float sy = __builtin_ldexpf(iy, (int)((A.y >> 14) & 15u));
    const float sz = __builtin_ldexpf(iz, (int)((A.y >> 18) & 15u));
    const float bx = __builtin_fmaf((float)(A.x & 0x3FFFu), 4.0f * ix, -oix);
    const float by = __builtin_fmaf((float)((A.x >> 14) & 0x3FFFu), 4.0f * iy, -oiy);
    const float bz = __builtin_fmaf((float)(A.y & 0x3FFFu), 4.0f * iz, -oiz);
    const uint32_t meta = A.y >> 22;  // bits 30..31 are zero
    const uint32_t w[5] = {A.z, A.w, B.x, B.y, B.z};
    const int base = (int)B.w;
    const float inf = __builtin_huge_valf();
    float tf0, tf1, tf2, tf3;
    const float tn0 = w4_child<0>(w, sx, bx, sy, by, sz, bz, t.best.t, tf0);
    const float tn1 = w4_child<1>(w, sx, bx, sy, by, sz, bz, t.best.t, tf1);
    const float tn2 = w4_child<2>(w, sx, bx, sy, by, sz, bz, t.best.t, tf2);
    const float tn3 = w4_child<3>(w, sx, bx, sy, by, sz, bz, t.best.t, tf3);
    const uint32_t m0 = meta & 3u, m1 = (meta >> 2) & 3u, m2 = (meta >> 4) & 3u, m3 = (meta >> 6) & 3u;
    float k0 = ((tn0 <= tf0) & (m0 != 0u)) ? tn0 : inf;
    float k1 = ((tn1 <= tf1) & (m1 != 0u)) ? tn1 : inf;
    float k2 = ((tn2 <= tf2) & (m2 != 0u)) ? tn2 : inf;
    float k3 = ((tn3 <= tf3) & (m3 != 0u)) ? tn3 : inf;
    // child codes: inner slots come first (node at base + 2c), then the leaves' triangles
    const int i1 = m1 == 1u, i2 = m2 == 1u, i3 = m3 == 1u;
    const int n_inner = (int)(m0 == 1u) + i1 + i2 + i3;
    const int l0 = m0 >= 2u ? (int)m0 - 1 : 0, l1 = m1 >= 2u ? (int)m1 - 1 : 0, l2 = m2 >= 2u ? (int)m2 - 1 : 0;
    const int lb = base + 2 * n_inner;
    int c0 = m0 == 1u ? base : ~(lb * 4 + l0);
    int c1 = i1 ? base + 2 : ~((lb + 3 * l0) * 4 + l1);
    int c2 = i2 ? base + 4 : ~((lb + 3 * (l0 + l1)) * 4 + l2);
    int c3 = i3 ? base + 6 : ~((lb + 3 * (l0 + l1 + l2)) * 4 + (m3 >= 2u ? (int)m3 - 1 : 0));
    cas(k0, c0, k1, c1);
    cas(k2, c2, k3, c3);
    cas(k0, c0, k2, c2);
    cas(k1, c1, k3, c3);
    cas(k1, c1, k2, c2);
    const int hits = (int)(k0 < inf) + (int)(k1 < inf) + (int)(k2 < inf) + (int)(k3 < inf);
    // pushes above the top (the farthest deepest): hits 4 -> c3 c2 c1, 3 -> c2 c1, 2 -> c1
    stk.write(sp, hits == 4 ? c3 : (hits == 3 ? c2 : c1));
    stk.write(sp + 1, hits == 4 ? c2 : c1);
    stk.write(sp + 2, c1);
    asm volatile("" : "+v"(top));
    const int popped = sp > 0 ? top : -1;
    t.node = hits > 0 ? c0 : popped;
    t.sp = hits > 0 ? sp + hits - 1 : sp_pop;
}

// Leaf step, run by every lane of a leaf phase with no divergent branch: lanes
// without a pending leaf, and the second record of a one-triangle leaf, load through a buffer
// offset past the resource's range, which returns zeros without a memory access, and their tests
// are masked off.  Straight-line code lets the closest-hit state stay in its registers (the
// divergent form made the compiler copy it in and out at every join).
__device__ __forceinline__ float4 tri_unit(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}
template <int FMT, typename Stack>
__device__ __forceinline__ void leaf_step(__amdgpu_buffer_rsrc_t trs, const Ray& r, Trav& t, const Stack& stk) {
    const bool lf = t.node <= -2;
    const int v = ~t.node;
    const int unit = FMT == kFmtW4 ? (v >> 2) : 3 * (v >> 4);
    const int count = lf ? (FMT == kFmtW4 ? (v & 3) : (v & 15)) : 0;
    constexpr uint32_t kNoLoad = 0x80000000u;  // > num_records (0x7fffffff): zeros, no access
    const uint32_t o0 = count > 0 ? (uint32_t)unit * 16u : kNoLoad;
    const uint32_t o1 = count > 1 ? (uint32_t)(unit + 3) * 16u : kNoLoad;
    const float4 p0 = tri_unit(trs, o0), p1 = tri_unit(trs, o0 + 16u), p2 = tri_unit(trs, o0 + 32u);
    const float4 q0 = tri_unit(trs, o1), q1 = tri_unit(trs, o1 + 16u), q2 = tri_unit(trs, o1 + 32u);
    take_hit(r, p0, p1, p2, unit, t.best, count > 0);
    take_hit(r, q0, q1, q2, unit + 3, t.best, count > 1);
    // A leaf of more than 2 triangles (only below the builder's depth cap) continues as the same leaf
    // two triangles on, instead of a loop here: the step stays loop-free (a divergent loop in it
    // made the compiler move the closest-hit state into other registers and back at every join).
    const bool more = count > 2;
    const int rest = FMT == kFmtW4 ? ~((unit + 6) * 4 + (count - 2)) : ~(((unit / 3) + 2) * 16 + (count - 2));
    const int sp = t.sp;
    int top = stk.below(sp);
    asm volatile("" : "+v"(top));
    if constexpr (Stack::kSentinel) {
        t.node = lf ? (more ? rest : top) : t.node;
        t.sp = (lf & !more) ? sp - 1 : sp;
    } else {
        t.node = lf ? (more ? rest : (sp > 0 ? top : -1)) : t.node;
        t.sp = (lf & !more) ? max(sp - 1, 0) : sp;
    }
}

}  // namespace
}  // namespace arx
