// arx_replay.hip -- the replay family: frames answered from the records of trace_kernel<RECORD>
// (arx_trace.hip) and the receiver sub-tree alone.  replay_kernel replays every query of every ray
// (the path cache); filter_kernel + replay_cand_kernel replay only the queries whose segment meets
// the receiver's box (the path filter); filter_multi_kernel + cand_work_kernel +
// replay_cand_multi_kernel do that for a chunk of listeners in one call; band_replay_kernel replays
// every query once for several absorption tables (frequency bands); band_base_kernel +
// band_cand_multi_kernel do the chunk of listeners for every band at once.  The band kernels' DIRECTED
// instantiations start a ray's bands from e0 times its row of a gain plane (a source pattern,
// arx_directivity.hpp); the others are the kernels as they were, and the launchers take them without a plane.
// Their AIR instantiations weight a receiver deposit by the bin's row of an attenuation table (air absorption,
// include/arx.h); the launchers take them only with a table.
//
// Every query here is the same arithmetic on the same bits as the traced frame's (arx_trace_device.hpp's functions),
// and each step the kernels share -- the kernel set-up, the record read, the receiver query, a candidate's entry,
// state and chain, the bands' alive mask, the filter's meta plane, box, prelude and output -- exists once, below.
// Three places keep a copy of their own, because sharing it changed their machine code: receiver_ctx's meta plane,
// band_replay_kernel's alive update, the two multi kernels' work-item walk.  Not part of the trace kernel's
// identity (build.py TRACE_KERNEL_FILES): an edit here leaves the stored trace profiles valid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "arx_bands.hpp"
#include "arx_cand_plan.hpp"
#include "arx_kernels.hpp"
#include "arx_layout.hpp"
#include "arx_trace_device.hpp"

#ifndef ARX_REPLAY_BLOCK
#define ARX_REPLAY_BLOCK 256  // replay_kernel's block; design experiments only (build.py --exp)
#endif
#ifndef ARX_CAND_BLOCKS
#define ARX_CAND_BLOCKS 2048  // replay_cand_kernel's blocks at most; design experiments only (build.py --exp)
#endif

namespace arx {
namespace {

// What a replay kernel sets up once: the LDS stack (with its sentinel row), node_step's top-of-tree
// copy, the node and triangle descriptors, and the planes of the recording -- the records, and with
// FilterArgs the filter's segment / state / meta planes (arx_layout.hpp).
template <int BLOCK>
struct ReceiverCtx {
    using Stack = LdsStack<BLOCK, kLdsStack>;
    Stack stk;
    const uint4* ncache;
    __amdgpu_buffer_rsrc_t nrs, trs;
    arx_i32x4 qrs;
    const float4* tbase;
    uint64_t n;  // rays of the recording
    const float4* __restrict__ rec_hit;
    const float2* __restrict__ rec_bary;
    const float4* __restrict__ seg;
    const float4* __restrict__ state;
    const unsigned short* __restrict__ meta;
};

// Called once by every lane of the block, before any divergence (it holds a barrier when the build
// has a node cache), and once per kernel: the stack and the node copy are this function's own
// __shared__ arrays, one per BLOCK, so a second call in a kernel would hand out the same stack.
template <int BLOCK>
__device__ __forceinline__ ReceiverCtx<BLOCK> receiver_ctx(const TraceArgs& a) {
    __shared__ int stk_lds[(kLdsStack + 1) * BLOCK];
    __shared__ uint4 ncache[kNodeCache > 0 ? 2 * kNodeCache : 1];  // node_step's top-of-tree copy, as in trace_kernel
    if constexpr (kNodeCache > 0) {
        const uint4* q = reinterpret_cast<const uint4*>(a.qnodes);
        for (int i = threadIdx.x; i < 2 * kNodeCache; i += BLOCK) ncache[i] = q[i];
        __syncthreads();
    }
    ReceiverCtx<BLOCK> c;
    c.stk.base = stk_lds + threadIdx.x;
    stk_lds[threadIdx.x] = -1;  // the dummy row under the stack (LdsStack::kSentinel)
    c.ncache = ncache;
    c.nrs = buffer_rsrc(a.qnodes, ARX_TRACE_IDXEN ? (short)sizeof(QNode2) : (short)0);
    c.qrs = qnodes_rsrc4(a.qnodes);
    c.tbase = reinterpret_cast<const float4*>(a.tris);
    c.trs = buffer_rsrc(c.tbase);
    c.n = a.ray_end - a.ray_begin;
    c.rec_hit = reinterpret_cast<const float4*>(a.rec);
    c.rec_bary = reinterpret_cast<const float2*>(c.rec_hit + (uint64_t)a.max_bounces * c.n);
    c.seg = nullptr;
    c.state = nullptr;
    c.meta = nullptr;
    return c;
}
// The filter's per-ray plane, behind the segment and state planes of a recording of n rays.
__device__ __forceinline__ const unsigned short* filter_meta_plane(const TraceArgs& a, const FilterArgs& f, uint64_t n) {
    return reinterpret_cast<const unsigned short*>(reinterpret_cast<const float4*>(f.planes) +
                                                   (path_filter_seg_rows(a.max_bounces) + (uint64_t)a.max_bounces) * n);
}
template <int BLOCK>
__device__ __forceinline__ ReceiverCtx<BLOCK> receiver_ctx(const TraceArgs& a, const FilterArgs& f) {
    ReceiverCtx<BLOCK> c = receiver_ctx<BLOCK>(a);
    c.seg = reinterpret_cast<const float4*>(f.planes);
    c.state = c.seg + path_filter_seg_rows(a.max_bounces) * c.n;
    c.meta = reinterpret_cast<const unsigned short*>(c.state + (uint64_t)a.max_bounces * c.n);  // the meta plane
    return c;
}

// The cached scene-only closest hit of record `at` (bounce * n + slot), as trace_kernel<RECORD> stored it.
template <int BLOCK>
__device__ __forceinline__ void load_record(const ReceiverCtx<BLOCK>& c, uint64_t at, Best& best) {
    const float4 h = c.rec_hit[at];
    const float2 b = c.rec_bary[at];
    best.t = h.x;
    best.id = __float_as_int(h.y);
    best.unit = __float_as_int(h.z);
    best.v = h.w;
    best.w = b.x;
    best.det = b.y;
}

// One closest-hit query over a receiver sub-tree alone, starting from the hit already in `best`: for
// the active lanes setup_ray, the grid form of the slab planes (trace_kernel's, on the same bits) and
// one step on node `top` with its child 0 forced off (node 0: the scene; a listener's own top node:
// empty) -- on to the receiver's root or done, so a segment that misses the receiver's box costs that
// one step.  Then, for the whole wave, the sub-tree: node steps while any lane has one, then the
// pending leaves.  The loop's ballots are wave-wide: every lane of the wave must call this from
// uniform control flow, each with its own `active`.
template <int BLOCK>
__device__ __forceinline__ void receiver_query(const ReceiverCtx<BLOCK>& c, const TraceArgs& a, bool active,
                                               const RayState& s, int top, Ray& r, Best& best) {
    using Stack = typename ReceiverCtx<BLOCK>::Stack;
    // The traversal's state stays local and the caller keeps only the hit, so that the closest-hit
    // registers are not copied at the callers' loop joins (profiles/r14/replay_split.json).
    Trav t;
    t.best = best;
    float oix = 0.f, oiy = 0.f, oiz = 0.f;
    t.node = -1;
    t.sp = 0;
    if (active) {
        setup_ray(r, s.pos, s.dir);
        oix = (r.o[0] - a.qgrid.origin[0]) * r.inv[0];
        oiy = (r.o[1] - a.qgrid.origin[1]) * r.inv[1];
        oiz = (r.o[2] - a.qgrid.origin[2]) * r.inv[2];
        r.inv[0] *= a.qgrid.scale[0];
        r.inv[1] *= a.qgrid.scale[1];
        r.inv[2] *= a.qgrid.scale[2];
#if ARX_TRACE_SIGNSEL && ARX_TRACE_BITFLOAT
        oix = __builtin_fmaf(8388608.0f, r.inv[0], oix);
        oiy = __builtin_fmaf(8388608.0f, r.inv[1], oiy);
        oiz = __builtin_fmaf(8388608.0f, r.inv[2], oiz);
#endif
        t.node = top;
        node_step<kFmtQ16, Stack, false, true>(r, oix, oiy, oiz, t, c.stk, c.nrs, c.ncache, c.qrs);
    }
    while (true) {
        const unsigned long long m_node = __ballot(t.node >= 0);
        const unsigned long long m_leaf = __ballot(t.node <= -2);
        if ((m_node | m_leaf) == 0ull) break;
        if (m_node != 0ull) {
            if (t.node >= 0) node_step<kFmtQ16, Stack, false>(r, oix, oiy, oiz, t, c.stk, c.nrs, c.ncache, c.qrs);
        } else {
            leaf_step<kFmtQ16>(c.trs, r, t, c.stk);
        }
    }
    best = t.best;
}

// The path cache's replay (arx_capi_path_cache.cpp, PathCache): a frame of a key whose scene-only closest
// hits trace_kernel<RECORD> stored.  A ray's path through the static scene does not depend on the
// listener; the receiver enters a query only as one more candidate for the closest hit, take_hit's
// lexicographic minimum of (t, id) does not depend on the order candidates are tested in, and a
// receiver hit ends the ray.  So each query here is the cached hit, a closest-hit query over the
// receiver sub-tree alone that starts from it, and the same shade(): the histogram and the counters
// come out bit for bit as the full traversal's.  The receiver sub-tree is entered by one step on the
// top node with child 0 (the scene) forced off: a segment that misses the receiver's box costs that
// one step.  One ray per lane, slot = lane's global index into the cache's own direction copy
// (a.dirs); a plain grid, every lane's work about the same, so no pool and no persistent waves.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void replay_kernel(TraceArgs a) {
    const ReceiverCtx<BLOCK> c = receiver_ctx<BLOCK>(a);
    const int lane = threadIdx.x;
    const uint64_t slot = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t n_q = 0, n_rx = 0, n_miss = 0;
    RayState s;
    s.depth = -1;
    bool active = false;
    if (slot < c.n) {
        ray_init(a, s, a.ray_begin + slot);
        active = wants_query(a, s);
    }
    Ray r;
    Best best;
    while (__ballot(active) != 0ull) {
        if (active) {
            // (fetching the next bounce's record a query ahead measured even: the load is not what a
            // query waits for, profiles/r10/ab_path_cache.txt)
            load_record(c, (uint64_t)s.depth * c.n + slot, best);
            ++n_q;
        }
        receiver_query(c, a, active, s, 0, r, best);
        if (active) {
            shade(a, c.tbase, s, r, best, n_rx, n_miss);
            active = wants_query(a, s);
        }
    }
    flush_counters(a, n_q, n_rx, n_miss, lane);
}

// ------------------------------------------------------ frequency bands ---
// arx_render_bands: NB bands answered by one walk over a ray's records.  A band is the scene with
// another absorption per triangle (BandArgs::table, by global triangle id); absorption enters shade()
// only through e = e * (1 - ab) and, via wants_query, through when e > energy_thres stops the ray.  So the
// geometry of a query -- hit point, distance, chord, bin, reflection, next origin -- is run once, in
// shade()'s operation order on the same bits, and only the energy is carried per band.
//
// band_shade is shade() for the recording's own ray (s, whose energy keeps following the scene's
// absorption: the walk's loop guard) and for the bands in `alive`: a receiver half adds each live band's
// energy to that band's [L | R] by shade()'s delay / hrtf / is_mono rules, a miss counts for each, anything
// else multiplies e[b] by 1 - table[id][b].  A dead band's energy is still multiplied (no branch per
// band); nothing reads it again.
// A reflection's absorption per band: e[b] times 1 - table[id][b], the row in one or two 16-B loads.  id
// is a scene triangle's, below n_tris (the clamp keeps a bad record inside the table).
template <int NB>
__device__ __forceinline__ void band_absorb(const BandArgs& ba, int tri_id, float (&e)[NB]) {
    static_assert(NB == 4 || NB == 8, "a table row is one or two 16-B loads");
    const uint64_t id = min((uint64_t)(uint32_t)tri_id, (uint64_t)ba.n_tris - 1u);
    const float4* __restrict__ row = reinterpret_cast<const float4*>(ba.table) + id * (NB / 4);
    float tb[NB];
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
        const float4 t = row[q];
        tb[4 * q + 0] = t.x;
        tb[4 * q + 1] = t.y;
        tb[4 * q + 2] = t.z;
        tb[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) e[b] = e[b] * (1.0f - tb[b]);
}

// The bands that live: the table's at a ray's start; before every query those with e[b] > energy_thres still.
template <int NB>
__device__ __forceinline__ uint32_t band_alive_init(int32_t n_bands) { return (1u << min(n_bands, NB)) - 1u; }
template <int NB>
__device__ __forceinline__ uint32_t band_alive_update(const float (&e)[NB], float thres, uint32_t alive) {
#pragma unroll
    for (int b = 0; b < NB; ++b) alive &= (e[b] > thres) ? ~0u : ~(1u << b);
    return alive;
}

// A directed source (BandArgs::gain, arx_directivity.hpp): the energies a ray's bands start from, e0 times the
// slot's row of the gain plane -- one or two 16-B loads, once per ray.  Gains lie in [0, 1] and the f32 product
// by one is monotone, so e[b] <= e0 and the induction above band_replay_kernel holds as it stands: every query a
// directed band runs has a record.  A band whose start fails e[b] > energy_thres never lives and counts nothing.
// slot is below the recording's rays (the plane's rows).
template <int NB>
__device__ __forceinline__ void band_start_directed(const TraceArgs& a, const BandArgs& ba, uint64_t slot, float (&e)[NB]) {
    static_assert(NB == 4 || NB == 8, "a plane row is one or two 16-B loads");
    const float4* __restrict__ row = reinterpret_cast<const float4*>(ba.gain) + slot * (NB / 4);
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
        const float4 g = row[q];
        e[4 * q + 0] = a.e0 * g.x;
        e[4 * q + 1] = a.e0 * g.y;
        e[4 * q + 2] = a.e0 * g.z;
        e[4 * q + 3] = a.e0 * g.w;
    }
}

// Air absorption (BandArgs::air, include/arx.h): what the bands deposit in bin k, ea[b] = e[b] * att[k][b], one
// f32 product each, the table's row k in one or two 16-B loads.  Every band's product is formed, live or not (a
// dead band's is not read): with the products inside the per-band branches the compiler moves the loads in
// there too, split into dwords, each waited for on its own.  The caller holds 0 <= k < a.ir_len, the table's
// rows: a dropped hit reads nothing.
template <int NB>
__device__ __forceinline__ void band_air_deposits(const BandArgs& ba, int k, const float (&e)[NB], float (&ea)[NB]) {
    static_assert(NB == 4 || NB == 8, "a table row is one or two 16-B loads");
    const float4* __restrict__ row = reinterpret_cast<const float4*>(ba.air) + (uint64_t)k * (NB / 4);
    float4 t[NB / 4];
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) t[q] = row[q];
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
        ea[4 * q + 0] = e[4 * q + 0] * t[q].x;
        ea[4 * q + 1] = e[4 * q + 1] * t[q].y;
        ea[4 * q + 2] = e[4 * q + 2] * t[q].z;
        ea[4 * q + 3] = e[4 * q + 3] * t[q].w;
    }
}

// AIR: a receiver deposit of band b is e[b] * att[k][b], one f32 product, for both ears at the hit's own bin k
// (the interaural delay is the head's, not the path's).  The carried e[b] is untouched -- air weights arrivals
// and never ends a ray -- so the counters and the induction above band_replay_kernel stand as they are.
template <int NB, bool AIR>
__device__ __forceinline__ void band_shade(const TraceArgs& a, const BandArgs& ba, const float4* __restrict__ tbase,
                                           RayState& s, const Best& best, float (&e)[NB], uint32_t alive,
                                           uint32_t& rx, uint32_t& miss) {
    const int hit = best.unit;
    if (hit < 0) {
        miss |= alive;
        s.depth = -1;
        return;
    }
    const float4* tp = tbase + hit;
    const float4 p0 = tp[0], p1 = tp[1], p2 = tp[2];
    const float3 P1 = make_float3(p0.x, p0.y, p0.z);
    const float3 P2 = make_float3(p1.x, p1.y, p1.z);
    const float3 P3 = make_float3(p2.x, p2.y, p2.z);
    const float ab = p0.w;
    const float3 U = sub3(P2, P1), V = sub3(P3, P1);
    const float3 cr = make_float3(U.y * V.z - V.y * U.z, U.z * V.x - V.z * U.x, U.x * V.y - V.x * U.y);
    const float hv = best.v, hw = best.w, hdet = best.det;
    const float bu = hv / hdet;
    const float bv = hw / hdet;
    const float w0 = (1.0f - bu) - bv;
    const float3 P = add3(add3(scale3(w0, P1), scale3(bu, P2)), scale3(bv, P3));
    const float3 seg = sub3(P, s.pos);
    s.dist += sqrtf(dot3(seg, seg));
    float es = s.e;
    if (ab < 0.0f) {  // receiver chord weighting: the chord once, every energy times it
        const float3 center = make_float3(a.center[0], a.center[1], a.center[2]);
        const float3 nd = scale3(1.0f / sqrtf(dot3(s.dir, s.dir)), s.dir);
        const float3 oc = sub3(P, center);
        const float qa = dot3(nd, nd);
        const float qb = 2.0f * dot3(oc, nd);
        const float qc = dot3(oc, oc) - 1.0f;
        const float disc = qb * qb - (4.0f * qa) * qc;
        if (disc <= 0.0f) {
            es = 0.0f;
#pragma unroll
            for (int b = 0; b < NB; ++b) e[b] = 0.0f;
        } else {
            const float sq = sqrtf(disc);
            const float t1 = (-qb - sq) / (2.0f * qa);
            const float t2 = (-qb + sq) / (2.0f * qa);
            const float3 i1 = add3(P, scale3(t1, nd));
            const float3 i2 = add3(P, scale3(t2, nd));
            const float3 di = sub3(i1, i2);
            const float chord = sqrtf(dot3(di, di));
            es = es * chord;
#pragma unroll
            for (int b = 0; b < NB; ++b) e[b] = e[b] * chord;
        }
    }
    if (ab == -1.0f || ab == -2.0f) {  // receiver halves: every live band ends here
        rx |= alive;
        const int k = (int)roundf((s.dist / (float)kSpeedOfSound) * (float)a.sample_rate);
        if (k < a.ir_len) {
            const int kk = (k + a.delay < a.ir_len) ? k + a.delay : k;
            const uint64_t own = (ab == -1.0f) ? 0u : (uint64_t)a.ir_len;
            const uint64_t other = (ab == -1.0f) ? (uint64_t)a.ir_len : 0u;
            float ea[NB];
            // k >= 0, for the row as for the histogram below: s.dist is a sum of square roots, so roundf's argument
            // is >= 0 or NaN, which the conversion takes to 0; +inf converts to INT_MAX and fails k < ir_len
            if constexpr (AIR) band_air_deposits<NB>(ba, k, e, ea);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if ((alive >> b) & 1u) {  // alive holds bits below n_bands only: inside the bands' block
                    unsigned long long* h = ba.hist + (uint64_t)b * 2u * (uint64_t)a.ir_len;
                    float eb = e[b];
                    if constexpr (AIR) eb = ea[b];
                    hist_add(h + own, k, eb, a.inv_unit);
                    if (!a.is_mono) hist_add(h + other, kk, eb * (1.0f - a.hrtf), a.inv_unit);
                }
            }
        }
        s.depth = -1;
    } else {  // specular reflection, and each band's own absorption
        const float s2 = (2.0f * dot3(s.dir, cr)) / dot3(cr, cr);
        s.dir = sub3(s.dir, scale3(s2, cr));
        es = es * (1.0f - ab);
        band_absorb<NB>(ba, best.id, e);
        ++s.depth;
    }
    s.e = es;
    s.pos = add3(P, scale3(1e-3f, s.dir));
}

// band_replay_kernel, a lane per recorded slot on replay_kernel's plain grid.  The walk is the
// recording's own loop (wants_query with the scene's energy); a band lives while its own loop guard
// holds -- distance and depth are the walk's, so that is e[b] > energy_thres at every query -- and counts
// queries only while it lives.  Every band's absorption is at least the scene's on every triangle
// (arx_band_table_check), f32 1 - ab and the product by a non-negative e are monotone under rounding, so
// e[b] never exceeds the recorded ray's energy at the same bounce: a live band's query always has a
// record.  A lane leaves once no band lives.  Per band the histogram and the three counters are those of
// replay_kernel on a scene that carries the band's absorption.
template <int BLOCK, int NB, bool DIRECTED, bool AIR>
__global__ __launch_bounds__(BLOCK) void band_replay_kernel(TraceArgs a, BandArgs ba) {
    const ReceiverCtx<BLOCK> c = receiver_ctx<BLOCK>(a);
    const int lane = threadIdx.x;
    const uint64_t slot = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    float e[NB];
    uint32_t n_q[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        e[b] = a.e0;
        n_q[b] = 0u;
    }
    uint32_t alive = 0u, rx = 0u, miss = 0u;  // a bit per band
    RayState s;
    s.depth = -1;
    bool active = false;
    if (slot < c.n) {
        ray_init(a, s, a.ray_begin + slot);
        active = wants_query(a, s);
        if (active) alive = band_alive_init<NB>(ba.n_bands);
        if constexpr (DIRECTED) band_start_directed<NB>(a, ba, slot, e);
    }
    Ray r;
    Best best;
    while (__ballot(active) != 0ull) {
        if (active) {
#pragma unroll
            for (int b = 0; b < NB; ++b) alive &= (e[b] > a.energy_thres) ? ~0u : ~(1u << b);  // band_alive_update, in place
            active = alive != 0u;
        }
        if (active) {
            load_record(c, (uint64_t)s.depth * c.n + slot, best);
#pragma unroll
            for (int b = 0; b < NB; ++b) n_q[b] += (alive >> b) & 1u;
        }
        receiver_query(c, a, active, s, 0, r, best);
        if (active) {
            band_shade<NB, AIR>(a, ba, c.tbase, s, best, e, alive, rx, miss);
            active = wants_query(a, s);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b >= ba.n_bands) break;  // the same for every lane
        a.counters = ba.counters + (uint64_t)b * kBandCounterWords;
        flush_counters(a, n_q[b], (rx >> b) & 1u, (miss >> b) & 1u, lane);
    }
}

// ------------------------------------------------------- the path filter ---
// A filtered replay: the recording also stored what every query started from (arx_layout.hpp), so the
// queries of a ray no longer depend on each other, and a frame needs only those whose segment can
// touch the receiver.  filter_kernel finds them, replay_cand_kernel runs them.
//
// filter_kernel, a lane per slot on a plain grid: the ray's rows of the segment plane, each read once
// (the previous row stays in registers), segment [pos_b, pos_b+1] against the receiver's box, one bit
// per bounce.  Always candidates: a last query that missed (its segment has no end) or that ended on a
// receiver-marked triangle of the scene (its shading needs a.center), and every query of a ray the
// recording flagged (kFilterWild).  No atomic anywhere: a block compacts its candidate rays into its own
// stretch of the frame set's list and leaves a 16-B head -- how many, their candidate queries, and the
// summed query counts of its rays without a candidate, which replay_cand_kernel adds to the frame's counters.
//
// The box is the f32 box of the top node's receiver child (cnodes[0], written by the receiver refit on
// the same stream, so it follows the listener with no host copy), grown by a.grow on every side.  Why
// that is enough -- the one place where exactness is argued and not inherited:
//   - The traced frame ends a ray on the receiver in query b only if take_hit accepted a receiver
//     triangle at some t <= best.t, best.t being the scene-only hit the record holds: the point
//     X = pos_b + t * dir_b of the segment [pos_b, Q], Q = pos_b + best.t * dir_b.
//   - X lies in that triangle up to the triangle test's rounding: t is the barycentric mean of the
//     vertices' depths along the ray's major axis, so X is off the triangle by a few ulps of the
//     coordinates' magnitude M times at most sqrt(3) (the major axis holds >= 1/sqrt(3) of |dir|),
//     far below 1e-5 * M; and the triangle lies inside the box, which the refit pads by 1e-5 * M.
//   - The stored segment ends at E = P + 1e-3 * dir', not at Q.  The recording checked, for this very
//     query, |Q - E| <= kFilterEndSlack = 2^-8 m on every axis (else the ray is kFilterWild) -- no bound on
//     |dir| or on how well t and the barycentric P agree is assumed.  X = pos_b + u (Q - pos_b), u in
//     [0, 1], so the stored segment's point pos_b + u (E - pos_b) is within 2^-8 m of X per axis.
//   - So a box grown by 2^-8 m plus the rounding above is met by the stored segment whenever the
//     receiver can be hit.  kFilterMargin is 2^-7 m: twice that; the box is about 2 m wide, the slack costs nothing.
//   - The slab test's own rounding: u = (plane - p) * rcp(d) carries a relative error below 2^-21
//     (two subtractions, a 1-ulp reciprocal, a product), which is the exact u of a plane moved by
//     |plane - p| * 2^-21 <= 2^-20 * M.  The host adds 2^-18 * M to a.grow, M from the grid that holds
//     the scene, the emitter and the receiver.  A NaN anywhere compares as "candidate".
__device__ __forceinline__ bool segment_meets_box(float4 p, float4 q, const float (&lo)[3], const float (&hi)[3]) {
    const float pp[3] = {p.x, p.y, p.z}, qq[3] = {q.x, q.y, q.z};
    float un = 0.0f, uf = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float d = qq[k] - pp[k];
        if (fabsf(d) < 1e-20f) d = (d < 0.0f) ? -1e-20f : 1e-20f;
        const float inv = __builtin_amdgcn_rcpf(d);
        const float u0 = (lo[k] - pp[k]) * inv, u1 = (hi[k] - pp[k]) * inv;
        un = fmaxf(un, fminf(u0, u1));
        uf = fminf(uf, fmaxf(u0, u1));
    }
    return !(un > uf);
}

// The receiver's box as the filter takes it: the f32 box of a top node's receiver child (child 1), grown.
__device__ __forceinline__ void receiver_box(const BvhNode& top, float grow, float (&lo)[3], float (&hi)[3]) {
    lo[0] = top.b[0] - grow; lo[1] = top.b[2] - grow; lo[2] = top.c[2] - grow;
    hi[0] = top.b[1] + grow; hi[1] = top.b[3] + grow; hi[2] = top.c[3] + grow;
}
// A filter lane's ray: its meta word (0 for an idle lane), the queries it ran, and the wave's longest
// count, which bounds the segment loop so that every lane's loads stay unconditional.
struct FilterRay { uint32_t m, count, cmax; };
__device__ __forceinline__ FilterRay filter_ray_prelude(const TraceArgs& a, bool have, uint64_t slot,
                                                        const unsigned short* __restrict__ meta) {
    FilterRay fr;
    fr.m = have ? meta[slot] : 0u;
    fr.count = min(fr.m & (uint32_t)kFilterCount, min(a.max_bounces, kFilterMaxBounces));
    uint32_t cmax = fr.count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, (uint32_t)__shfl_xor((int)cmax, off, 64));
    fr.cmax = __builtin_amdgcn_readfirstlane(cmax);
    return fr;
}
// The queries that are candidates whatever the box says: a flagged last query, every query of a wild ray.
__device__ __forceinline__ unsigned long long filter_fix_mask(uint32_t m, uint32_t count, unsigned long long mask) {
    if (count > 0u) {
        const unsigned long long last = 1ull << (count - 1u), all = last | (last - 1ull);
        if (m & (kFilterMiss | kFilterMarked)) mask |= last;
        if (m & kFilterWild) mask = all;
    }
    return mask;
}

// The filter's output for one listener, with no atomic anywhere.  (One atomic per wave on a list cursor
// and the counters, 15 625 waves at C3 on two cache lines, was what bound this kernel: 0.26 ms for a 41 us
// read, profiles/r11/ab_path_filter.txt.)  The block compacts its candidates into its own stretch of the
// list, [blockIdx * BLOCK, ...): at most one entry per slot, so the stretch is the block's slots.  Its
// head holds how many, their queries, and the queries of the rays that need no replay, which the
// candidate kernel adds to the frame's counters with its own.  Two halves with the caller's
// __syncthreads() between them: filter_sums leaves each wave's partial sums in the listener's three
// [BLOCK / 64] LDS rows and returns the wave's candidate ballot; filter_store writes the entries and the head.
__device__ __forceinline__ unsigned long long filter_sums(unsigned long long mask, uint32_t count, uint32_t* w_cand,
                                                          uint32_t* w_cq, uint32_t* w_nq) {
    const bool cand = mask != 0ull;
    const unsigned long long ballot = __ballot(cand);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int cq = cand ? (unsigned int)__popcll(mask) : 0u, nq = cand ? 0u : count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cq += __shfl_xor(cq, off, 64);
        nq += __shfl_xor(nq, off, 64);
    }
    if (lane == 0) {
        w_cand[wave] = (uint32_t)__popcll(ballot);
        w_cq[wave] = cq;
        w_nq[wave] = nq;
    }
    return ballot;
}
template <int BLOCK>
__device__ __forceinline__ void filter_store(unsigned long long mask, unsigned long long ballot, uint64_t slot,
                                             FilterCand* list, void* heads, const uint32_t* w_cand,
                                             const uint32_t* w_cq, const uint32_t* w_nq) {
    constexpr int WAVES = BLOCK / 64;
    const int wave = threadIdx.x >> 6;
    uint32_t before = 0u, t_cand = 0u, t_cq = 0u, t_nq = 0u;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        before += w < wave ? w_cand[w] : 0u;
        t_cand += w_cand[w];
        t_cq += w_cq[w];
        t_nq += w_nq[w];
    }
    if (mask != 0ull) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
        FilterCand c;
        c.mask = mask;
        c.slot = (uint32_t)slot;
        c.pad = 0u;
        // before + rank < the block's candidates <= its slots below n, so inside the list's n entries
        list[(uint64_t)blockIdx.x * BLOCK + before + rank] = c;
    }
    // (a missed last query is always a candidate: no misses among the rays counted here)
    if (threadIdx.x == 0) reinterpret_cast<uint4*>(heads)[blockIdx.x] = make_uint4(t_cand, t_cq, t_nq, 0u);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void filter_kernel(TraceArgs a, FilterArgs f) {
    const uint64_t n = a.ray_end - a.ray_begin;
    const uint64_t gid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool have = gid < n;
    const uint64_t slot = have ? gid : n - 1;  // n >= 1 (launch_path_replay_filtered); idle lanes read in bounds
    const float4* __restrict__ seg = reinterpret_cast<const float4*>(f.planes);
    const unsigned short* __restrict__ meta = filter_meta_plane(a, f, n);
    // the receiver's box: the same address for every lane, so scalar loads, once per wave
    float lo[3], hi[3];
    receiver_box(a.cnodes[0], f.grow, lo, hi);
    const FilterRay fr = filter_ray_prelude(a, have, slot, meta);
    unsigned long long mask = 0ull;
    float4 p = seg[slot];
#pragma unroll 4
    for (uint32_t b = 0; b < fr.cmax; ++b) {
        // rows past the ray's last are not its own: it re-reads its last row (count <= max_bounces exists)
        const float4 q = seg[(uint64_t)min(b + 1u, fr.count) * n + slot];
        const bool hit = segment_meets_box(p, q, lo, hi);
        mask |= (hit && b < fr.count) ? (1ull << b) : 0ull;
        p = q;
    }
    mask = filter_fix_mask(fr.m, fr.count, mask);
    __shared__ uint32_t w_cand[BLOCK / 64], w_cq[BLOCK / 64], w_nq[BLOCK / 64];
    const unsigned long long ballot = filter_sums(mask, fr.count, w_cand, w_cq, w_nq);
    __syncthreads();
    filter_store<BLOCK>(mask, ballot, slot, f.list, f.heads, w_cand, w_cq, w_nq);
}

// What a chain starts from, entry i of `list` for the lanes that `have` one (zeros otherwise): its slot, clamped
// into the recording; the ray's meta word and count, clamped as the filter clamps it; its mask trimmed to that.
struct CandEntry { unsigned long long mask; uint64_t slot; uint32_t m, count; };
template <int BLOCK>
__device__ __forceinline__ CandEntry cand_entry(const ReceiverCtx<BLOCK>& c, const TraceArgs& a,
                                                const FilterCand* __restrict__ list, uint64_t i, bool have) {
    CandEntry ce = {0ull, 0, 0u, 0u};
    if (have) {
        const FilterCand e = list[i];
        ce.mask = e.mask;
        ce.slot = e.slot < c.n ? e.slot : c.n - 1;
        ce.m = c.meta[ce.slot];
    }
    ce.count = min(ce.m & (uint32_t)kFilterCount, min(a.max_bounces, kFilterMaxBounces));
    ce.mask &= ce.count > 0u ? ((1ull << (ce.count - 1u)) << 1) - 1ull : 0ull;  // bits of queries the ray ran
    return ce;
}
// A candidate query's start: the stored state of record `at` (bounce * n + slot) and the cached hit.
template <int BLOCK>
__device__ __forceinline__ void cand_state_load(const ReceiverCtx<BLOCK>& c, uint64_t at, RayState& s, Best& best) {
    const float4 sp = c.seg[at], sd = c.state[at];
    load_record(c, at, best);
    s.pos = make_float3(sp.x, sp.y, sp.z); s.dist = sp.w;
    s.dir = make_float3(sd.x, sd.y, sd.z); s.e = sd.w;
}
// One entry of a candidate list, entry i of `list` for the lanes that `have` one: the chain of its
// queries.  For each set bit, ascending: the stored state and the cached hit, then replay_kernel's
// query (receiver_query, entered at node `top`) on the same bits with the same functions.  If the receiver
// gave the closest hit, or this is the ray's flagged last query, shade() runs and the ray ends; else
// nothing is shaded, the next query's state being stored already.  A ray that does not end here ran its
// recorded count of queries.  Wave-wide like receiver_query: every lane of the wave calls it, from
// uniform control flow.
template <int BLOCK>
__device__ __forceinline__ void cand_chain(const ReceiverCtx<BLOCK>& c, const TraceArgs& a,
                                           const FilterCand* __restrict__ list, uint64_t i, bool have, int top,
                                           uint32_t& n_q, uint32_t& n_rx, uint32_t& n_miss) {
    const uint64_t n = c.n;
    auto [mask, slot, m, count] = cand_entry(c, a, list, i, have);
    bool active = mask != 0ull, ended = false;
    Ray r;
    Best best;
    while (__ballot(active) != 0ull) {
        RayState s;
        s.depth = -1;
        int unit0 = -1;
        if (active) {
            const uint32_t b = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            cand_state_load(c, (uint64_t)b * n + slot, s, best);
            s.depth = (int)b;
            unit0 = best.unit;
        }
        receiver_query(c, a, active, s, top, r, best);
        if (active) {
            const bool flagged = (uint32_t)s.depth + 1u == count && (m & (kFilterMiss | kFilterMarked)) != 0u;
            if (best.unit != unit0 || flagged) {
                n_q += (uint32_t)s.depth + 1u;
                shade(a, c.tbase, s, r, best, n_rx, n_miss);
                ended = true;
                active = false;
            } else if (mask == 0ull) {
                active = false;
            }
        }
    }
    if (have && !ended) n_q += count;
}

// replay_cand_kernel: the candidate rays' chains (cand_chain), a 64-lane block per part -- 64 entries of a
// filter block's stretch of the list, a lane per candidate ray -- so a stretch full of candidates is sixteen
// waves' work, not one wave's sixteen rounds: the pool's slots are ordered longest first with the rays the
// receiver ended in front (launch_order_pool), so the candidates crowd into a few stretches.  The stretch's
// head says how many it holds (device memory: nothing waits on the host).
// Which block takes which part is found from the heads and not by position.  A grid with a block for each of
// a stretch's sixteen parts is 15 625 blocks at 1 M rays of which a few hundred hold candidates, and such a
// launch lasts as long as that many blocks take to come and go, whatever they do: 0.20 ms, against 0.10 ms
// for this one (profiles/r19/ab_cand_blocks.txt).  Here a fixed number of blocks (kCandBlocks) each read all
// the heads -- 16 B per stretch, kCandHeadsPerLane heads a lane and tile -- and number the parts that hold
// candidates in stretch order (arx_cand_plan.hpp): block j takes parts j, j + gridDim.x, ...; a block past
// the last part leaves before anything else is set up.  No list of work items, no device memory and no
// atomic for it: every block finds its own parts again from the heads.  The queries of the rays
// filter_kernel retired come in through the heads, tile t's added by block t % gridDim.x.
__global__ __launch_bounds__(64) void replay_cand_kernel(TraceArgs a, FilterArgs f) {
    constexpr int BLOCK = 64;
    const uint64_t n = a.ray_end - a.ray_begin;
    const uint32_t fblocks = (uint32_t)((n + kFilterBlock - 1) / kFilterBlock);  // < 2^27 (launch_path_replay_filtered)
    const uint4* __restrict__ heads = reinterpret_cast<const uint4*>(f.heads);
    const uint32_t lane = threadIdx.x;
    uint32_t n_q = 0, n_rx = 0, n_miss = 0;
    // how many parts there are, and this block's share of the heads' query counts
    uint32_t items = 0u;
    for (uint32_t t0 = 0u, t = 0u; t0 < fblocks; t0 += kCandTile, ++t) {
        const bool add = t % gridDim.x == blockIdx.x;
#pragma unroll
        for (uint32_t i = 0; i < kCandHeadsPerLane; ++i) {
            const uint32_t fb = t0 + lane * kCandHeadsPerLane + i;
            if (fb < fblocks) {
                const uint4 h = heads[fb];
                items += cand_parts(min(h.x, kFilterBlock));
                if (add) n_q += h.z;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) items += (uint32_t)__shfl_xor((int)items, off, 64);
    items = (uint32_t)__builtin_amdgcn_readfirstlane((int)items);
    if (blockIdx.x >= items) {
        flush_counters(a, n_q, 0u, 0u, threadIdx.x);
        return;
    }
    const ReceiverCtx<BLOCK> c = receiver_ctx<BLOCK>(a, f);
    uint32_t k = blockIdx.x, done = 0u;  // the block's next part; the parts of the tiles before this one
    for (uint32_t t0 = 0u; t0 < fblocks && k < items; t0 += kCandTile) {
        uint32_t cand[kCandHeadsPerLane], parts = 0u;
#pragma unroll
        for (uint32_t i = 0; i < kCandHeadsPerLane; ++i) {
            const uint32_t fb = t0 + lane * kCandHeadsPerLane + i;
            cand[i] = fb < fblocks ? min(heads[fb].x, kFilterBlock) : 0u;
            parts += cand_parts(cand[i]);
        }
        uint32_t incl = parts;  // inclusive scan within the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= (uint32_t)off) incl += v;
        }
        const uint32_t tile_parts = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        while (k < done + tile_parts) {  // part k lies in this tile: the first lane whose scan passes it holds it
            const uint32_t r = k - done;
            const int owner = __builtin_ctzll(__ballot(incl > r));
            const CandItem it = cand_lane_item(cand, r - (incl - parts));  // the owner's is the part
            const uint32_t fb = min(t0 + (uint32_t)owner * kCandHeadsPerLane + (uint32_t)__shfl((int)it.head, owner, 64), fblocks - 1u);
            const uint32_t base = (uint32_t)__shfl((int)it.part, owner, 64) * kCandPart;
            const uint32_t n_cand = (uint32_t)__shfl((int)it.n_cand, owner, 64);
            const uint64_t i = (uint64_t)fb * kFilterBlock + base + lane;
            cand_chain(c, a, f.list, i, base + lane < n_cand && i < n, 0, n_q, n_rx, n_miss);
            k += gridDim.x;
        }
        done += tile_parts;
    }
    flush_counters(a, n_q, n_rx, n_miss, threadIdx.x);
}

// ------------------------------------------------- a batch of listeners ---
// arx_render_listeners: many listeners answered from one recording.  Neither the records nor the filter's
// planes depend on the listener, so a listener is a box to cull the stored segments against and a receiver
// sub-tree to query; a chunk of them has its sub-trees placed side by side (ListenerEntry, arx_layout.hpp).
//
// filter_multi_kernel is filter_kernel with the segment in registers tested against F listeners' boxes:
// one read of the segment plane serves F listeners (blockIdx.y picks the F).  Per listener the arithmetic,
// the mask, the block's stretch of that listener's list and its head are filter_kernel's for that listener
// alone: the box is the same six floats of the listener's top node with the same grow, and the prelude,
// segment_meets_box, the mask's fix-up and the two halves of the output are the same functions, the
// compaction running per listener on its own ballot.  The boxes wait in LDS, six floats a listener, read
// by every lane at the same address.
template <int BLOCK, int F>
__global__ __launch_bounds__(BLOCK) void filter_multi_kernel(TraceArgs a, FilterArgs f,
                                                             const ListenerEntry* __restrict__ tbl, int32_t listeners) {
    const uint64_t n = a.ray_end - a.ray_begin;
    const uint64_t gid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool have = gid < n;
    const uint64_t slot = have ? gid : n - 1;  // n >= 1 (launch_listeners_replay); idle lanes read in bounds
    const float4* __restrict__ seg = reinterpret_cast<const float4*>(f.planes);
    const unsigned short* __restrict__ meta = filter_meta_plane(a, f, n);
    const int j0 = (int)blockIdx.y * F;  // this pass's listeners: [j0, min(j0 + F, listeners))
    __shared__ float box[F][6];
    if (threadIdx.x < F) {
        const int i = threadIdx.x;
        float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
        if (j0 + i < listeners) receiver_box(a.cnodes[tbl[j0 + i].top], f.grow, lo, hi);  // the slot's, as the refit left it
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            box[i][k] = lo[k];
            box[i][3 + k] = hi[k];
        }
    }
    __syncthreads();
    const FilterRay fr = filter_ray_prelude(a, have, slot, meta);
    unsigned long long mask[F];
#pragma unroll
    for (int i = 0; i < F; ++i) mask[i] = 0ull;
    float4 p = seg[slot];
#pragma unroll 2
    for (uint32_t b = 0; b < fr.cmax; ++b) {
        const float4 q = seg[(uint64_t)min(b + 1u, fr.count) * n + slot];
        const unsigned long long bit = b < fr.count ? (1ull << b) : 0ull;
#pragma unroll
        for (int i = 0; i < F; ++i) {
            const float lo[3] = {box[i][0], box[i][1], box[i][2]}, hi[3] = {box[i][3], box[i][4], box[i][5]};
            mask[i] |= segment_meets_box(p, q, lo, hi) ? bit : 0ull;
        }
        p = q;
    }
    // all F partial sums, one barrier, then all F outputs
    __shared__ uint32_t w_cand[F][BLOCK / 64], w_cq[F][BLOCK / 64], w_nq[F][BLOCK / 64];
    unsigned long long ballot[F];
#pragma unroll
    for (int i = 0; i < F; ++i) {
        mask[i] = filter_fix_mask(fr.m, fr.count, mask[i]);
        ballot[i] = filter_sums(mask[i], fr.count, w_cand[i], w_cq[i], w_nq[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < F; ++i) {
        if (j0 + i >= listeners) break;  // a ragged last pass (the same for the whole block)
        const ListenerEntry& e = tbl[j0 + i];
        filter_store<BLOCK>(mask[i], ballot[i], slot, e.list, e.heads, w_cand[i], w_cq[i], w_nq[i]);
    }
}

// cand_work_kernel, a block per listener: the listener's work items in stretch order -- for every stretch
// its first 64 entries (that item also adds the stretch's head) and every further 64 that hold a
// candidate -- as (stretch * 16 + part) words behind their count (ListenerEntry::work).  A block for
// each of a frame's 16 x stretches parts, the empty ones leaving, is with a chunk of listeners hundreds of
// thousands of blocks that only read a head, and dispatching them was what the chunk's candidate launch took
// (profiles/r12/listeners_kernel_stats.csv; one frame's replay_cand_kernel finds its parts from the heads in
// every block, with no list, for the same reason).  No atomic: a block-wide
// scan of the parts per stretch, tile after tile.
__global__ __launch_bounds__(1024) void cand_work_kernel(const ListenerEntry* __restrict__ tbl, uint32_t fblocks) {
    constexpr int BLOCK = 1024, WAVES = BLOCK / 64;
    const ListenerEntry& e = tbl[blockIdx.x];
    const uint4* __restrict__ heads = reinterpret_cast<const uint4*>(e.heads);
    __shared__ uint32_t w_sum[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t done = 0u;  // items of the tiles before this one (the same in every thread)
    for (uint32_t t0 = 0u; t0 < fblocks; t0 += BLOCK) {
        const uint32_t fb = t0 + threadIdx.x;
        uint32_t parts = 0u;
        if (fb < fblocks) parts = max(1u, (min(heads[fb].x, kFilterBlock) + 63u) / 64u);
        uint32_t incl = parts;  // inclusive scan within the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) w_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            before += w < wave ? w_sum[w] : 0u;
            total += w_sum[w];
        }
        const uint32_t at = done + before + incl - parts;  // <= 16 * fb: inside the 16 * fblocks words
        for (uint32_t c = 0u; c < parts; ++c) e.work[4u + at + c] = fb * 16u + c;
        done += total;
        __syncthreads();  // w_sum is written again by the next tile
    }
    if (threadIdx.x == 0) e.work[0] = done;
}

// replay_cand_multi_kernel is replay_cand_kernel with the listener taken from blockIdx.y: the histogram,
// the counters, shade()'s centre, the list and the heads come from the listener's table entry (the same for
// the whole block, so they stay scalar), and the query enters the listener's own top node instead of node 0
// -- child 0 empty and skipped, child 1 the slot's receiver root -- so it is the same arithmetic on the same
// boxes and triangles.  The per-ray chain is the same function, cand_chain.
// What differs is which block takes which 64 entries: a listener's blocks walk its work items
// (cand_work_kernel) gridDim.x apart, so neighbouring items -- the candidates crowd into few stretches --
// go to different blocks, and no block is launched only to leave.  A stretch's first item also adds the
// stretch's candidate rays to the listener's tally (e.cand).
__global__ __launch_bounds__(64) void replay_cand_multi_kernel(TraceArgs a, FilterArgs f,
                                                               const ListenerEntry* __restrict__ tbl) {
    constexpr int BLOCK = 64;
    const ListenerEntry& e = tbl[blockIdx.y];
    const uint64_t n = a.ray_end - a.ray_begin;
    const uint64_t fblocks = (n + kFilterBlock - 1) / kFilterBlock;
    const uint32_t n_items = min(e.work[0], (uint32_t)min(fblocks * (kFilterBlock / BLOCK), (uint64_t)0xffffffffu));
    if (blockIdx.x >= n_items) return;
    for (int k = 0; k < 3; ++k) a.center[k] = e.center[k];
    a.hist = e.hist;
    a.counters = e.counters;
    const FilterCand* list = e.list;
    const int top = e.top;
    const ReceiverCtx<BLOCK> c = receiver_ctx<BLOCK>(a, f);
    const int lane = threadIdx.x;
    uint32_t n_q = 0, n_rx = 0, n_miss = 0;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t word = e.work[4u + item];  // the same address for every lane, like the head
        const uint64_t fb = min((uint64_t)(word >> 4), fblocks - 1);
        const uint32_t base = (word & 15u) * BLOCK;
        const uint4 head = reinterpret_cast<const uint4*>(e.heads)[fb];
        const uint32_t n_cand = min(head.x, kFilterBlock);
        const uint64_t i = fb * kFilterBlock + base + lane;
        if (base == 0u && lane == 0) {
            n_q += head.z;
            if (head.x) atomicAdd(e.cand, (unsigned long long)head.x);
        }
        cand_chain(c, a, list, i, base + lane < n_cand && i < n, top, n_q, n_rx, n_miss);
    }
    flush_counters(a, n_q, n_rx, n_miss, lane);
}

// ------------------------------------------- a batch of listeners, per band ---
// arx_render_listener_bands: the listener batch's filtered replay carrying band_replay_kernel's energies.
// Two things a filtered band replay needs that a filtered frame does not, and where they come from:
//   - A candidate query's energy per band is the product over the ray's earlier hits.  Those are the
//     recorded triangle ids (a 16-B record load and one table row each: band_absorb); the position, distance
//     and direction before the candidate query are in the filter's planes.  So a candidate ray is walked
//     once from bounce 0 and only its candidate bounces run the receiver query (band_chain).
//   - A band's query count needs every ray.  base_b(ray), the queries band b makes along the ray's scene-only
//     recording, does not depend on the listener: band_base_kernel counts it once per call for every ray.  A
//     ray that a listener's receiver ends at query k took max(0, base_b - (k + 1)) queries of band b away,
//     and only a candidate ray can be ended; a flagged last query is the ray's last recorded query and cuts
//     nothing.  So per (listener, band): queries = sum of base_b over all rays - sum of the cuts of the ended.
//
// band_base_kernel, a lane per recorded slot on the plain grid: the ray's records for queries 0 .. count - 1
// (the meta word's count, clamped as the filter clamps it), the energies from a.e0 through band_absorb, a
// band alive -- and counting -- exactly as in band_replay_kernel.  The ray's counts go out packed, a byte per
// band (count <= 64), 8 B per ray; the sums go to the base counter block (ba.counters).
template <int BLOCK, int NB, bool DIRECTED>
__global__ __launch_bounds__(BLOCK) void band_base_kernel(TraceArgs a, FilterArgs f, BandArgs ba, uint2* __restrict__ counts) {
    const uint64_t n = a.ray_end - a.ray_begin;
    const uint64_t gid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool have = gid < n;
    const uint64_t slot = have ? gid : n - 1;  // n >= 1 (launch_band_base); idle lanes read in bounds
    const float4* __restrict__ rec_hit = reinterpret_cast<const float4*>(a.rec);
    const unsigned short* __restrict__ meta = filter_meta_plane(a, f, n);
    const FilterRay fr = filter_ray_prelude(a, have, slot, meta);
    float e[NB];
    uint32_t n_q[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        e[b] = a.e0;
        n_q[b] = 0u;
    }
    if constexpr (DIRECTED) band_start_directed<NB>(a, ba, slot, e);
    uint32_t alive = fr.count > 0u ? band_alive_init<NB>(ba.n_bands) : 0u;
    for (uint32_t q = 0; q < fr.count; ++q) {
        alive = band_alive_update<NB>(e, a.energy_thres, alive);
        if (alive == 0u) break;
#pragma unroll
        for (int b = 0; b < NB; ++b) n_q[b] += (alive >> b) & 1u;
        band_absorb<NB>(ba, __float_as_int(rec_hit[(uint64_t)q * n + slot].y), e);
    }
    if (have) {
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int b = 0; b < NB; ++b) w[b >> 2] |= n_q[b] << (8 * (b & 3));  // n_q <= count <= 64
        counts[slot] = make_uint2(w[0], w[1]);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b >= ba.n_bands) break;  // the same for every lane
        a.counters = ba.counters + (uint64_t)b * kBandCounterWords;
        flush_counters(a, n_q[b], 0u, 0u, threadIdx.x);
    }
}

// One entry of a listener's candidate list as a band chain (cand_chain's frame): the lane walks its ray's
// bounces from 0.  Before every bounce `alive` is updated exactly as band_replay_kernel updates it; a bounce
// outside the mask only multiplies the energies from the record's id; a bounce in the mask loads the stored
// state and the record and runs cand_chain's query.  If the receiver gave the closest hit, or this is the
// ray's flagged last query, band_shade runs into the listener's bands' block and the ray ends: its rx / miss
// bits per live band, and per band the queries it took away, from the ray's packed counts.  A ray that does
// not end contributes nothing, and nothing past its last candidate bounce is read.  Wave-wide like
// receiver_query.
template <int BLOCK, int NB, bool DIRECTED, bool AIR>
__device__ __forceinline__ void band_chain(const ReceiverCtx<BLOCK>& c, const TraceArgs& a, const BandArgs& ba,
                                           const FilterCand* __restrict__ list, uint64_t i, bool have, int top,
                                           const uint2* __restrict__ counts, uint32_t (&cut)[NB], uint32_t& rx,
                                           uint32_t& miss) {
    const uint64_t n = c.n;
    auto [mask, slot, m, count] = cand_entry(c, a, list, i, have);
    float e[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) e[b] = a.e0;
    if constexpr (DIRECTED) band_start_directed<NB>(a, ba, slot, e);  // cand_entry's slot: clamped into the recording
    bool active = mask != 0ull;
    uint32_t alive = active ? band_alive_init<NB>(ba.n_bands) : 0u;
    uint32_t q = 0u;  // the bounce the energies stand before
    rx = 0u;
    miss = 0u;
    Ray r;
    Best best;
    while (__ballot(active) != 0ull) {
        RayState s;
        s.depth = -1;
        int unit0 = -1;
        if (active) {
            const uint32_t target = (uint32_t)__builtin_ctzll(mask);
            for (;;) {
                alive = band_alive_update<NB>(e, a.energy_thres, alive);
                if (alive == 0u || q >= target) break;
                band_absorb<NB>(ba, __float_as_int(c.rec_hit[(uint64_t)q * n + slot].y), e);
                ++q;
            }
            active = alive != 0u;
        }
        if (active) {
            cand_state_load(c, (uint64_t)q * n + slot, s, best);
            s.depth = (int)q;
            unit0 = best.unit;
        }
        receiver_query(c, a, active, s, top, r, best);
        if (active) {
            const bool flagged = q + 1u == count && (m & (kFilterMiss | kFilterMarked)) != 0u;
            mask &= mask - 1ull;
            if (best.unit != unit0 || flagged) {
                band_shade<NB, AIR>(a, ba, c.tbase, s, best, e, alive, rx, miss);
                const uint2 pk = counts[slot];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const uint32_t base = ((b < 4 ? pk.x : pk.y) >> (8 * (b & 3))) & 0xffu;
                    cut[b] += base > q + 1u ? base - (q + 1u) : 0u;
                }
                active = false;
            } else if (mask == 0ull) {
                active = false;
            } else {  // the record stands: the scene's triangle reflects
                band_absorb<NB>(ba, best.id, e);
                ++q;
            }
        }
    }
}

// band_cand_multi_kernel is replay_cand_multi_kernel with band_chain for cand_chain: the listener from
// blockIdx.y, its work items gridDim.x apart, the entry's values scalar; e.hist and e.counters are the
// listener's bands' block (BandArgs' layout).  Per band the block leaves in counter word 0 the queries its
// ended rays took away (band_cut_kernel turns them into the frame's count), in words 1 and 2 the frame's
// receiver hits and misses.  rx and miss are a bit per ray and band: a ballot's population count, summed in
// scalar registers, lane 0 handing the wave's sum to flush_counters.
template <int NB, bool DIRECTED, bool AIR>
__global__ __launch_bounds__(64) void band_cand_multi_kernel(TraceArgs a, FilterArgs f, const ListenerEntry* __restrict__ tbl,
                                                             BandArgs ba, const uint2* __restrict__ counts) {
    constexpr int BLOCK = 64;
    const ListenerEntry& e = tbl[blockIdx.y];
    const uint64_t n = a.ray_end - a.ray_begin;
    const uint64_t fblocks = (n + kFilterBlock - 1) / kFilterBlock;
    const uint32_t n_items = min(e.work[0], (uint32_t)min(fblocks * (kFilterBlock / BLOCK), (uint64_t)0xffffffffu));
    if (blockIdx.x >= n_items) return;
    for (int k = 0; k < 3; ++k) a.center[k] = e.center[k];
    ba.hist = e.hist;
    ba.counters = e.counters;
    const FilterCand* list = e.list;
    const int top = e.top;
    const ReceiverCtx<BLOCK> c = receiver_ctx<BLOCK>(a, f);
    const int lane = threadIdx.x;
    uint32_t cut[NB], w_rx[NB], w_miss[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) cut[b] = w_rx[b] = w_miss[b] = 0u;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t word = e.work[4u + item];  // the same address for every lane, like the head
        const uint64_t fb = min((uint64_t)(word >> 4), fblocks - 1);
        const uint32_t base = (word & 15u) * BLOCK;
        const uint4 head = reinterpret_cast<const uint4*>(e.heads)[fb];
        const uint32_t n_cand = min(head.x, kFilterBlock);
        if (base == 0u && lane == 0 && head.x) atomicAdd(e.cand, (unsigned long long)head.x);
        const uint64_t i = fb * kFilterBlock + base + lane;
        uint32_t rx, miss;
        band_chain<BLOCK, NB, DIRECTED, AIR>(c, a, ba, list, i, base + lane < n_cand && i < n, top, counts, cut, rx, miss);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            w_rx[b] += (uint32_t)__popcll(__ballot((rx >> b) & 1u));
            w_miss[b] += (uint32_t)__popcll(__ballot((miss >> b) & 1u));
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b >= ba.n_bands) break;  // the same for every lane
        a.counters = ba.counters + (uint64_t)b * kBandCounterWords;
        flush_counters(a, cut[b], lane == 0 ? w_rx[b] : 0u, lane == 0 ? w_miss[b] : 0u, lane);
    }
}

// A chunk's query counts finished, a thread per (listener, band): the band's base total less what the
// listener's ended rays took away.
__global__ __launch_bounds__(256) void band_cut_kernel(const ListenerEntry* __restrict__ tbl, const unsigned long long* __restrict__ base,
                                                       int32_t n_bands, int32_t listeners) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= listeners * n_bands) return;
    unsigned long long* c = tbl[t / n_bands].counters + (uint64_t)(t % n_bands) * kBandCounterWords;
    c[0] = base[(uint64_t)(t % n_bands) * kBandCounterWords] - c[0];
}

}  // namespace

hipError_t launch_path_replay(const TraceArgs& a, hipStream_t s) {
    (void)hipGetLastError();
    if (!trace_can_cache(a, false) || !a.dirs || !a.tris || !a.hist || !a.counters || !a.rec)
        return hipErrorInvalidValue;
    if (a.clear_bins > 0 || a.clear_counters > 0) {
        const hipError_t e = launch_clear(a.hist, a.clear_bins, a.counters, a.clear_counters, s);
        if (e != hipSuccess) return e;
    }
    constexpr int RB = ARX_REPLAY_BLOCK;
    const uint64_t n_rays = a.ray_end - a.ray_begin;
    hipLaunchKernelGGL(replay_kernel<RB>, dim3((unsigned)((n_rays + RB - 1) / RB)), dim3(RB), 0, s, a);
    return hipGetLastError();
}

// The instantiation of a band kernel that deposits: the row width; without a gain plane and without an
// attenuation table the ones that never read those fields, with a plane the directed ones, with a table the
// AIR ones.  f takes the three as integral constants.
template <class F>
static void band_instantiation(const BandArgs& b, F&& f) {
    using W4 = std::integral_constant<int, 4>;
    using W8 = std::integral_constant<int, 8>;
    const auto by_air = [&](auto nb, auto directed) {
        if (b.air)
            f(nb, directed, std::true_type{});
        else
            f(nb, directed, std::false_type{});
    };
    const auto by_gain = [&](auto nb) {
        if (b.gain)
            by_air(nb, std::true_type{});
        else
            by_air(nb, std::false_type{});
    };
    if (band_width(b.n_bands) == 4)
        by_gain(W4{});
    else
        by_gain(W8{});
}

hipError_t launch_band_replay(const TraceArgs& a, const BandArgs& b, hipStream_t s) {
    (void)hipGetLastError();
    if (!trace_can_cache(a, false) || !a.dirs || !a.tris || !a.rec || !b.table || !b.hist || !b.counters || b.n_bands < 1 ||
        b.n_bands > kMaxBands || b.n_tris < 1 || a.ir_len < 1 || a.ray_end <= a.ray_begin)
        return hipErrorInvalidValue;
    const hipError_t e = launch_clear(b.hist, (uint64_t)b.n_bands * 2 * (uint64_t)a.ir_len, b.counters,
                                      b.n_bands * kBandCounterWords, s);
    if (e != hipSuccess) return e;
    constexpr int RB = ARX_REPLAY_BLOCK;
    const uint64_t n_rays = a.ray_end - a.ray_begin;
    const dim3 grid((unsigned)((n_rays + RB - 1) / RB));
    band_instantiation(b, [&](auto nb, auto directed, auto air) {
        hipLaunchKernelGGL((band_replay_kernel<RB, nb(), directed(), air()>), grid, dim3(RB), 0, s, a, b);
    });
    return hipGetLastError();
}

hipError_t launch_path_replay_filtered(const TraceArgs& a, const FilterArgs& f, hipStream_t s) {
    (void)hipGetLastError();
    if (!trace_can_cache(a, false) || !a.dirs || !a.tris || !a.hist || !a.counters || !a.rec || !a.cnodes || !f.planes ||
        !f.list || !f.heads || a.max_bounces < 1 || a.max_bounces > kFilterMaxBounces)
        return hipErrorInvalidValue;
    // (the clear folded into filter_kernel's lanes, as the direction pre-pass does it for a traced frame, took
    // the launch away and cost 4 % of the step: profiles/r19/ab_cand_blocks.txt)
    if (a.clear_bins > 0 || a.clear_counters > 0) {
        const hipError_t e = launch_clear(a.hist, a.clear_bins, a.counters, a.clear_counters, s);
        if (e != hipSuccess) return e;
    }
    constexpr int FB = (int)kFilterBlock;
    const uint64_t n_rays = a.ray_end - a.ray_begin;
    const uint64_t fblocks = (n_rays + FB - 1) / FB;
    // the candidate launch: a wave per 64 entries of a stretch at most, and a fixed number of blocks.  2 048:
    // at 1 M rays 1 024 and 2 048 are even and 4 096 is 4 % slower; with a fifth of the rays candidates
    // (over 3 300 parts) 1 024 is 40 % slower than 2 048 and 4 096 is 3 % faster (profiles/r19/ab_cand_blocks.txt)
    constexpr uint64_t kCandBlocks = ARX_CAND_BLOCKS;
    const uint64_t g2 = fblocks * (FB / 64);
    if (g2 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kernel<FB>, dim3((unsigned)fblocks), dim3(FB), 0, s, a, f);
    hipLaunchKernelGGL(replay_cand_kernel, dim3((unsigned)std::min<uint64_t>(g2, kCandBlocks)), dim3(64), 0, s, a, f);
    return hipGetLastError();
}

// A chunk's filter pass and its work items; *per: the candidate launch's blocks per listener.
static hipError_t launch_listeners_filter(const TraceArgs& a, const FilterArgs& f, const ListenerEntry* d_table,
                                          int32_t listeners, hipStream_t s, uint64_t* per) {
    if (!trace_can_cache(a, false) || !a.dirs || !a.tris || !a.rec || !a.cnodes || !f.planes || !d_table ||
        listeners < 1 || listeners > kListenerChunkMax || a.max_bounces < 1 || a.max_bounces > kFilterMaxBounces ||
        a.ray_end <= a.ray_begin)
        return hipErrorInvalidValue;
    constexpr int FB = (int)kFilterBlock;
    constexpr int F = (int)kListenerFilterWidth;
    const uint64_t n_rays = a.ray_end - a.ray_begin;
    const uint64_t fblocks = (n_rays + FB - 1) / FB;
    const uint64_t g2 = fblocks * (FB / 64);
    if (g2 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((filter_multi_kernel<FB, F>), dim3((unsigned)fblocks, (unsigned)((listeners + F - 1) / F)), dim3(FB), 0,
                       s, a, f, d_table, listeners);
    // the candidates: each listener's work items, then a fixed number of blocks that walk them
    hipLaunchKernelGGL(cand_work_kernel, dim3((unsigned)listeners), dim3(1024), 0, s, d_table, (uint32_t)fblocks);
    constexpr uint64_t kCandBlocks = 8192;  // of one wave each: what the device holds at once, and a half more
    *per = std::min<uint64_t>(g2, (kCandBlocks + (uint64_t)listeners - 1) / (uint64_t)listeners);
    return hipSuccess;
}

hipError_t launch_listeners_replay(const TraceArgs& a, const FilterArgs& f, const ListenerEntry* d_table,
                                   int32_t listeners, hipStream_t s) {
    (void)hipGetLastError();
    uint64_t per = 0;
    if (const hipError_t e = launch_listeners_filter(a, f, d_table, listeners, s, &per); e != hipSuccess) return e;
    hipLaunchKernelGGL(replay_cand_multi_kernel, dim3((unsigned)per, (unsigned)listeners), dim3(64), 0, s, a, f, d_table);
    return hipGetLastError();
}

static bool band_args_ok(const BandArgs& b) {
    return b.table && b.counters && b.n_bands >= 1 && b.n_bands <= kMaxBands && b.n_tris >= 1;
}

hipError_t launch_band_base(const TraceArgs& a, const FilterArgs& f, const BandArgs& b, void* counts, hipStream_t s) {
    (void)hipGetLastError();
    if (!trace_can_cache(a, false) || !a.rec || !f.planes || !band_args_ok(b) || !counts || a.max_bounces < 1 ||
        a.max_bounces > kFilterMaxBounces || a.ray_end <= a.ray_begin)
        return hipErrorInvalidValue;
    const hipError_t e = launch_clear(nullptr, 0, b.counters, b.n_bands * kBandCounterWords, s);
    if (e != hipSuccess) return e;
    constexpr int RB = ARX_REPLAY_BLOCK;
    const uint64_t n_rays = a.ray_end - a.ray_begin;
    const dim3 grid((unsigned)((n_rays + RB - 1) / RB));
    uint2* const out = static_cast<uint2*>(counts);
    const bool w4 = band_width(b.n_bands) == 4;
    if (!b.gain && w4)
        hipLaunchKernelGGL((band_base_kernel<RB, 4, false>), grid, dim3(RB), 0, s, a, f, b, out);
    else if (!b.gain)
        hipLaunchKernelGGL((band_base_kernel<RB, 8, false>), grid, dim3(RB), 0, s, a, f, b, out);
    else if (w4)
        hipLaunchKernelGGL((band_base_kernel<RB, 4, true>), grid, dim3(RB), 0, s, a, f, b, out);
    else
        hipLaunchKernelGGL((band_base_kernel<RB, 8, true>), grid, dim3(RB), 0, s, a, f, b, out);
    return hipGetLastError();
}

hipError_t launch_listener_bands_replay(const TraceArgs& a, const FilterArgs& f, const ListenerEntry* d_table,
                                        int32_t listeners, const BandArgs& b, const void* counts, hipStream_t s) {
    (void)hipGetLastError();
    if (!band_args_ok(b) || !counts) return hipErrorInvalidValue;
    uint64_t per = 0;
    if (const hipError_t e = launch_listeners_filter(a, f, d_table, listeners, s, &per); e != hipSuccess) return e;
    const dim3 grid((unsigned)per, (unsigned)listeners);
    const uint2* const in = static_cast<const uint2*>(counts);
    band_instantiation(b, [&](auto nb, auto directed, auto air) {
        hipLaunchKernelGGL((band_cand_multi_kernel<nb(), directed(), air()>), grid, dim3(64), 0, s, a, f, d_table, b, in);
    });
    hipLaunchKernelGGL(band_cut_kernel, dim3((unsigned)((listeners * b.n_bands + 255) / 256)), dim3(256), 0, s, d_table,
                       b.counters, b.n_bands, listeners);
    return hipGetLastError();
}

}  // namespace arx
