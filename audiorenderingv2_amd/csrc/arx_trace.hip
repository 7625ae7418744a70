// arx_trace.hip -- fused acoustic ray-trace kernel for gfx950 (MI355X).
//
// One lane carries one ray through all of its bounces (raygen -> closest hit -> shading ->
// histogram), replacing the OptiX pipeline of R/prebuild/obj_raytracer/devicePrograms.cu:
//   __raygen__renderFrame   :192-254  -> ray_init() + the refill loop of trace_kernel
//   optixTrace / RT cores   :240-251  -> node_step() / leaf_step(): software traversal of the
//                                        two-level BVH2 (16-bit quantized nodes), per-lane
//                                        stack, watertight triangle test
//   __closesthit__radiance  :62-180   -> shade()
//   __miss__radiance        :186-190  -> shade() with hit < 0
// Work distribution: persistent waves, each owning a static range of ray ids; a wave leaves
// its traversal loop when THRESH lanes wait for shading, shades them and refills retired lanes
// from its range.  The IR histogram is int64 fixed point (unit e0*2^-frac_bits) accumulated
// with 64-bit atomics: order-independent, bitwise reproducible and exactly summable across GPUs.
//
// Arithmetic is IEEE f32 with no contraction (built -ffp-contract=off) so that every ray follows
// bit for bit the path computed by the CPU oracle (oracle/arx_oracle.c).
//
// This file holds only the production kernel (one template; instances: quantized, f32 or CW4 nodes x
// LDS or global stack x ray-pool or small launch, and the pool's measuring instance, which feeds the
// longest-first order of the pool's direction slots: see launch_order_pool), its pre-pass and its
// launchers.  The query's device functions (setup_ray, node_step, leaf_step, shade) are in
// arx_trace_device.hpp; the kernels that replay this kernel's records are in arx_replay.hip.
// The round-1 design experiments (wide trees, octant copies,
// cooperative fetch, LDS node caches, ray pools, phased launches) are in
// the git history at commit 62a5de6 (audiorenderingv2_amd/csrc/arx_trace.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "arx_kernels.hpp"
#include "arx_layout.hpp"
#include "arx_trace_device.hpp"

namespace arx {
namespace {

#ifndef ARX_TRACE_BLOCK
#define ARX_TRACE_BLOCK 128
#endif
constexpr int kBlock = ARX_TRACE_BLOCK;

// Highest VGPR the trace kernel claims, so that its allocation (granule 8) admits exactly
// ARX_TRACE_WAVES waves per SIMD: 5 -> 88 VGPRs (512/88 = 5.8), 4 -> 104, 6 -> 80.  Every wave of
// a persistent launch owns an equal share of the rays, so a SIMD holding one wave more than the
// others sets the launch time; with 74 VGPRs the SIMDs of a CU took 6/6/4/4 of its 20 waves
// (+12 % on C3 against the same code at 88 VGPRs, tools/gpu_ab.sh, r02 log).
#ifndef ARX_TRACE_WAVES
#define ARX_TRACE_WAVES 5
#endif
#ifndef ARX_TRACE_COUNT
#define ARX_TRACE_COUNT 0  // 1: count node steps / leaf triangle tests into counters[4..5]
#endif
// Dynamic tail (launch_trace): launches with at least kDynMinRaysPerWave rays per wave put
// kDynShare/256 of their rays into the chunk pool of trace_kernel, kDynChunk rays per pool atomic.
// Small launches (about a ray per lane: C2, one 8-GPU rank's C5 shard) keep static ranges: there a
// chunk is a whole wave's work and the pool only lengthens the longest chains.
#ifndef ARX_TRACE_DYN_SHARE
#define ARX_TRACE_DYN_SHARE 128
#endif
#ifndef ARX_TRACE_DYN_CHUNK
#define ARX_TRACE_DYN_CHUNK 8
#endif
#ifndef ARX_TRACE_DYN_MIN
#define ARX_TRACE_DYN_MIN 96
#endif
constexpr int kDynShare = ARX_TRACE_DYN_SHARE, kDynChunk = ARX_TRACE_DYN_CHUNK, kDynMinRaysPerWave = ARX_TRACE_DYN_MIN;
#ifndef ARX_TRACE_PROF
#define ARX_TRACE_PROF 0  // 1: per-wave timing and lane-occupancy records into TraceArgs::prof
#endif
#if ARX_TRACE_WAVES == 5
#define ARX_TRACE_VGPR_FENCE "v87"
#elif ARX_TRACE_WAVES == 4
#define ARX_TRACE_VGPR_FENCE "v103"
#elif ARX_TRACE_WAVES == 6
#define ARX_TRACE_VGPR_FENCE "v79"
#else
#error "ARX_TRACE_WAVES must be 4, 5 or 6"
#endif

// The persistent trace kernel.  Each wave owns the static ray range [w_next, w_end) of its
// launch.  Outer loop: shade the lanes whose query finished, refill retired lanes with new rays
// (directions from the pre-pass), set up the next query of every lane that needs one.  Inner
// loop: NSTEPS guarded node steps per iteration; leaves are postponed and intersected wave-wide
// once LEAF_THRESH lanes hold one (or no lane can step); the loop is left when THRESH lanes wait
// for shading.
// LEAN (the small-launch instance): no per-lane "traversing" flag -- a lane's query is done when its
// node is -1 -- so the inner loop counts the lanes waiting for shading from wave masks on the SALU
// (C2 0.366 -> 0.350 ms; the pool instance measured +1 % with it, profiles/r05/ab_loop.txt).
// MEASURE (the measuring instance of the pool kernel, 16-bit nodes and LDS stack only): each lane counts
// the node steps and leaf steps of its current ray and, when it retires the ray, stores the count
// (ray_cost16; the largest count for a ray that ended on the receiver) into a.cost[slot], slot being
// the direction-buffer index the lane took at refill.  The
// launcher orders the pool's slots by that cost for the following launches (launch_order_pool).  Same
// rays, same arithmetic, same counters as the product instance, whose code this parameter leaves alone.
// RECORD (the path cache's recording instance, 16-bit nodes and LDS stack, pool or small): every query
// runs over the scene alone -- it starts at the top node's child 0, so the receiver is never a candidate
// and no ray ends on it -- and its final closest hit is stored at a.rec_*[depth * n + slot] before
// shade(), a miss too (unit -1).  The launcher points a.counters and a.cursor at a scratch block and
// passes no histogram: a scene may hold receiver-marked triangles of its own (absorption -1 / -2 is
// valid scene input), which end a ray here as they do in a traced frame, so this instance shades with
// shade<false>, which adds nothing to the histogram; the replay adds such a hit's energy from the
// record, with the frame's histogram.  replay_kernel answers the following launches of the same key.
template <int BLOCK, int THRESH, int LEAF_THRESH, int MINW, int NSTEPS, int FMT, bool GSTACK, bool LEAN = false,
          bool MEASURE = false, bool RECORD = false>
__global__ __launch_bounds__(BLOCK, MINW) void trace_kernel(TraceArgs a) {
    constexpr bool Q16 = FMT == kFmtQ16;
    constexpr bool W4 = FMT == kFmtW4;
    __shared__ int stk_lds[GSTACK ? 1 : (kLdsStack + 1) * BLOCK];  // + LdsStack's dummy row
    __shared__ uint4 ncache[(Q16 && kNodeCache > 0) ? 2 * kNodeCache : 1];
    if constexpr (Q16 && kNodeCache > 0) {
        const uint4* q = reinterpret_cast<const uint4*>(a.qnodes);
        for (int i = threadIdx.x; i < 2 * kNodeCache; i += BLOCK) ncache[i] = q[i];
        __syncthreads();
    }
    // Hold the VGPR allocation at the count that fits exactly MINW waves per SIMD (see
    // ARX_TRACE_VGPR_FENCE): the kernel needs ~74, which would let the dispatcher put 6 waves on
    // some SIMDs and 4 on others.
    asm volatile("" ::: ARX_TRACE_VGPR_FENCE);
    const int lane = threadIdx.x;
    const uint32_t gid = blockIdx.x * BLOCK + threadIdx.x;
    using Stack = typename std::conditional<
        W4, W4Stack<BLOCK, kLdsStack>,
        typename std::conditional<GSTACK, GlobalStack, LdsStack<BLOCK, kLdsStack>>::type>::type;
    Stack stk;
    if constexpr (W4) {  // LDS rows, then the global overflow column
        stk.lds = stk_lds + lane;
        stk.glob = a.gstack + gid;
        stk.stride = a.gstack_lanes;
    } else if constexpr (GSTACK) {
        stk.base = a.gstack + gid;
        stk.stride = a.gstack_lanes;
        stk.nrows = a.bvh_depth + 1;
    } else {
        stk.base = stk_lds + lane;
        stk_lds[lane] = -1;  // the dummy row under the stack (LdsStack::kSentinel)
    }
    const __amdgpu_buffer_rsrc_t nrs = W4 ? buffer_rsrc(a.wbuf)
                                          : (Q16 ? buffer_rsrc(a.qnodes, ARX_TRACE_IDXEN ? (short)sizeof(QNode2) : (short)0)
                                                 : buffer_rsrc(a.cnodes));
    const arx_i32x4 qrs = qnodes_rsrc4(a.qnodes);
    const float4* tbase = W4 ? reinterpret_cast<const float4*>(a.wbuf) : reinterpret_cast<const float4*>(a.tris);
    const __amdgpu_buffer_rsrc_t trs = buffer_rsrc(tbase);
    const uint64_t n = a.ray_end - a.ray_begin;
    const uint32_t wave_id = __builtin_amdgcn_readfirstlane(gid >> 6);
    const uint32_t n_waves = gridDim.x * (BLOCK / 64);
    // Rays [0, n_static) are dealt out statically (one contiguous range per wave); the rest form a
    // pool handed out in chunks of kDynChunk rays, one atomic per chunk, to waves whose static range
    // has run out -- equal work per wave still leaves waves finishing at different times (their
    // SIMD, CU and XCD neighbours differ), and the pool lets the fast ones finish the launch.
    const uint32_t dyn_chunk = a.dyn_chunk;
    const uint64_t n_static = pool_static_rays(n, a.dyn_share);
    const uint64_t n_dyn = n - n_static;
    uint64_t w_next = n_static * wave_id / n_waves;
    uint64_t w_end = n_static * (wave_id + 1) / n_waves;
    uint32_t n_q = 0, n_rx = 0, n_miss = 0;
#if ARX_TRACE_COUNT  // measurement builds only (build.py --exp ... -D ARX_TRACE_COUNT=1)
    uint32_t n_steps = 0, n_tris = 0;
    // the scalar-fetch probe: node lane-steps whose node is the wave leader's (the first lane with a
    // node to step), and node-step slots the wave ran -- a scalar load of the leader's node could
    // serve the former without vector-memory (TD) work
    uint32_t n_leader = 0, n_slots = 0;
#endif
#if ARX_TRACE_PROF  // measurement builds only: wave-uniform tallies (popcounts of ballots)
    // [0] start [1] end [2] rays [3] queries [4] node-step slots run [5] node lane-steps [6] leaf
    // phases [7] leaf lanes [8] shade phases [9] shade lanes [10] outer iterations [11] inner
    // iterations [12] time the wave's ray range ran out [13] wave id [14] refill phases [15] -
    uint64_t pf[kProfWords] = {};
    pf[0] = __builtin_readcyclecounter();
    pf[13] = wave_id;
    // HW_REG_HW_ID (wave / SIMD / CU / SE of this wave) | HW_REG_XCC_ID << 32: s_memtime counts per
    // XCD, so start skews compare waves of one XCD only
    pf[15] = (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
             ((uint64_t)__builtin_amdgcn_s_getreg((15 << 11) | 20) << 32);
#endif
    bool active = false, trav = false, exhausted = w_next >= w_end && n_dyn == 0;
    RayState s;
    s.depth = -1;
    Ray r;
    Trav t;
    t.best.t = __builtin_huge_valf();
    t.best.id = 0x7fffffff;
    t.best.unit = -1;
    t.node = -1;
    t.sp = 0;
    float oix = 0.f, oiy = 0.f, oiz = 0.f;
    uint32_t m_slot = 0u, m_cost = 0u;  // MEASURE: the current ray's buffer slot and its steps so far
    int rec_root = 0;  // RECORD: where a query starts, the scene root's code (a leaf code in a tiny scene)
    // RECORD: the filter's planes (null: records alone) and the current ray's flags so far
    float4* f_seg = nullptr;
    float4* f_state = nullptr;
    unsigned short* f_meta = nullptr;
    unsigned short f_flags = 0;
    if constexpr (RECORD) {
        rec_root = a.qnodes[0].c[0].code;
        if (a.gstack) {
            f_seg = reinterpret_cast<float4*>(a.gstack);
            f_state = f_seg + path_filter_seg_rows(a.max_bounces) * n;
            f_meta = reinterpret_cast<unsigned short*>(f_state + (uint64_t)a.max_bounces * n);
        }
    }
    while (true) {
#if ARX_TRACE_PROF
        ++pf[10];
        {
            const unsigned long long sh = __ballot(active && (LEAN ? t.node == -1 : !trav));
            if (sh) {
                ++pf[8];
                pf[9] += __popcll(sh);
            }
        }
#endif
        if (active && (LEAN ? t.node == -1 : !trav)) {  // the query is done: shade it
            const uint32_t rx_before = n_rx;
            int f_depth = 0;                            // RECORD with the filter's planes: the query's bounce ...
            float3 f_q = make_float3(0.f, 0.f, 0.f);  // ... and the ray's own hit point, pos + t * dir
            if constexpr (RECORD) {
                const uint64_t at = (uint64_t)s.depth * n + m_slot;
                float4* rec_hit = reinterpret_cast<float4*>(a.rec);
                float2* rec_bary = reinterpret_cast<float2*>(rec_hit + (uint64_t)a.max_bounces * n);
                rec_hit[at] = make_float4(t.best.t, __int_as_float(t.best.id), __int_as_float(t.best.unit), t.best.v);
                rec_bary[at] = make_float2(t.best.w, t.best.det);
                if (f_seg) {  // what the query started from (arx_layout.hpp, the path filter)
                    f_seg[at] = make_float4(s.pos.x, s.pos.y, s.pos.z, s.dist);
                    f_state[at] = make_float4(s.dir.x, s.dir.y, s.dir.z, s.e);
                    f_depth = s.depth;
                    f_q = add3(s.pos, scale3(t.best.t, s.dir));
                }
            }
            shade<!RECORD>(a, tbase, s, r, t.best, n_rx, n_miss);
            if constexpr (RECORD) {
                if (f_seg) {
                    // filter_kernel's margin rests on this: every point of [pos, pos + t * dir] lies within
                    // kFilterEndSlack per axis of the stored segment [pos, the pos shade() left].  A ray
                    // that breaks it once (a grazing hit's t, a degenerate triangle's reflection, a NaN)
                    // is replayed whole.
                    if (t.best.unit >= 0) {
                        const float3 dq = sub3(f_q, s.pos);
                        const float dev = fmaxf(fmaxf(fabsf(dq.x), fabsf(dq.y)), fabsf(dq.z));
                        if (!(dev <= kFilterEndSlack)) f_flags |= kFilterWild;
                    }
                    if (!wants_query(a, s)) {  // the ray's last query: the last segment's end and the per-ray record
                        const uint32_t cnt = (uint32_t)f_depth + 1u;
                        if (cnt <= a.max_bounces) f_seg[(uint64_t)cnt * n + m_slot] = make_float4(s.pos.x, s.pos.y, s.pos.z, s.dist);
                        f_meta[m_slot] = (unsigned short)((cnt & kFilterCount) | f_flags | (t.best.unit < 0 ? kFilterMiss : 0) |
                                                          (n_rx != rx_before ? kFilterMarked : 0));
                    }
                }
            }
            if (!wants_query(a, s)) {
                active = false;
                // the ray retires.  One the receiver ended says nothing about its length once the
                // listener has moved (the order outlives listener moves): it counts as the longest,
                // so it starts first -- ranked by its short count it would start last and, running its
                // full length from the listener's next position, be the launch's tail again
                if constexpr (MEASURE) a.cost[m_slot] = n_rx != rx_before ? (unsigned short)65535u : ray_cost16(m_cost);
            }
        }
        const unsigned long long need = __ballot(!active);
#if ARX_TRACE_PROF
        if (need != 0ull && !exhausted) {
            ++pf[14];
            pf[2] += std::min<uint64_t>(__popcll(need), w_end - w_next);
            if (w_next + __popcll(need) >= w_end) pf[12] = __builtin_readcyclecounter();
        }
#endif
        if (need != 0ull && !exhausted && w_next >= w_end) {  // the static range ran out: a pool chunk
            unsigned long long c = 0ull;
            if ((lane & 63) == 0) c = atomicAdd(a.cursor, (unsigned long long)dyn_chunk);
            const uint64_t start = n_static + __builtin_amdgcn_readfirstlane((uint32_t)c) +
                                   ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(c >> 32)) << 32);
            w_next = start;
            w_end = start + dyn_chunk < n ? start + dyn_chunk : n;
            if (start >= n) exhausted = true;
        }
        if (need != 0ull && !exhausted) {
            const int cnt = __popcll(need);
            const uint64_t base = w_next;
            w_next += (uint64_t)cnt;
            if (!active) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
                const uint64_t i = base + rank;
                if (i < w_end) {
                    ray_init(a, s, a.ray_begin + i);
                    active = wants_query(a, s);
                    if constexpr (RECORD) {
                        m_slot = (uint32_t)i;
                        f_flags = 0;
                        if (f_seg && !active) f_meta[i] = 0;  // a ray that never queries
                    }
                    if constexpr (MEASURE) {
                        m_slot = (uint32_t)i;  // i < n <= 2^31 - 1 rays
                        m_cost = 0u;
                        if (!active) a.cost[i] = 0;  // a ray that never queries
                    }
                }
            }
            if (w_next >= w_end && n_dyn == 0) exhausted = true;
        }
        if (active && (LEAN ? t.node == -1 : !trav)) {
            ++n_q;
            setup_ray(r, s.pos, s.dir);
            if constexpr (Q16 || W4) {  // grid form of the slab planes (node_step, node_step_w4)
                oix = (r.o[0] - a.qgrid.origin[0]) * r.inv[0];
                oiy = (r.o[1] - a.qgrid.origin[1]) * r.inv[1];
                oiz = (r.o[2] - a.qgrid.origin[2]) * r.inv[2];
                r.inv[0] *= a.qgrid.scale[0];
                r.inv[1] *= a.qgrid.scale[1];
                r.inv[2] *= a.qgrid.scale[2];
#if ARX_TRACE_SIGNSEL && ARX_TRACE_BITFLOAT
                if constexpr (Q16) {  // node_step's C = 2^23 * ix + (o - origin) * inv, one rounding
                    oix = __builtin_fmaf(8388608.0f, r.inv[0], oix);
                    oiy = __builtin_fmaf(8388608.0f, r.inv[1], oiy);
                    oiz = __builtin_fmaf(8388608.0f, r.inv[2], oiz);
                }
#endif
            } else {
                oix = r.o[0] * r.inv[0];
                oiy = r.o[1] * r.inv[1];
                oiz = r.o[2] * r.inv[2];
            }
            t.best.t = __builtin_huge_valf();
            t.best.id = 0x7fffffff;
            t.best.unit = -1;
            t.node = RECORD ? rec_root : 0;  // the top node (node 0; unit 0 of the CW4 buffer)
            t.sp = 0;
            trav = true;
        }
        if (__ballot(active) == 0ull) {
            if (exhausted) break;
            continue;
        }
        const unsigned long long m_active = LEAN ? __ballot(active) : 0ull;  // fixed inside the traversal loop
        while (true) {
            if (!LEAN && trav && t.node == -1) trav = false;  // query done (its stack is empty)
            const unsigned long long m_node = __ballot(t.node >= 0);
            const unsigned long long m_leaf = __ballot(t.node <= -2);
            if ((m_node | m_leaf) == 0ull) break;
            if constexpr (LEAN) {  // active lanes whose query is done (node -1) wait to be shaded
                if (lanes32(m_active & ~(m_node | m_leaf)) >= (uint32_t)THRESH) break;
            } else {
                if (__popcll(__ballot(active && !trav)) >= THRESH) break;
            }
#if ARX_TRACE_PROF
            ++pf[11];
#endif
            if (m_node != 0ull && (LEAN ? lanes32(m_leaf) < (uint32_t)LEAF_THRESH : __popcll(m_leaf) < LEAF_THRESH)) {
#pragma unroll
                for (int k = 0; k < NSTEPS; ++k) {
#if ARX_TRACE_PROF
                    const unsigned long long mk = __ballot(t.node >= 0);
                    if (mk) {
                        ++pf[4];
                        pf[5] += __popcll(mk);
                    }
#endif
#if ARX_TRACE_COUNT
                    {
                        const unsigned long long ml = __ballot(t.node >= 0);
                        if (ml) {
                            const int lead = __shfl(t.node, (int)__builtin_ctzll(ml), 64);
                            n_leader += (t.node >= 0 && t.node == lead) ? 1u : 0u;
                            n_slots += (lane & 63) == 0 ? 1u : 0u;
                        }
                    }
#endif
                    if (t.node >= 0) {
#if ARX_TRACE_COUNT
                        ++n_steps;
#endif
                        if constexpr (MEASURE) ++m_cost;
                        if constexpr (W4) node_step_w4(r, oix, oiy, oiz, t, stk, nrs);
                        else node_step<FMT, Stack, !LEAN>(r, oix, oiy, oiz, t, stk, nrs, ncache, qrs);
                    }
                }
            } else {
#if ARX_TRACE_PROF
                ++pf[6];
                pf[7] += __popcll(m_leaf);
#endif
#if ARX_TRACE_COUNT
                if (t.node <= -2) n_tris += (uint32_t)((~t.node) & (W4 ? 3 : 15));
#endif
                if constexpr (MEASURE) m_cost += t.node <= -2 ? 1u : 0u;
                leaf_step<FMT>(trs, r, t, stk);
            }
        }
    }
#if ARX_TRACE_PROF
    {
        unsigned int vq = n_q;
        for (int off = 32; off > 0; off >>= 1) vq += __shfl_xor(vq, off, 64);
        pf[3] = vq;
        pf[1] = __builtin_readcyclecounter();
        // one word per lane (a vector store with per-lane addresses)
        const int l = lane & 63;
        uint64_t v = 0;
#pragma unroll
        for (int k = 0; k < kProfWords; ++k) v = (l == k) ? pf[k] : v;
        if (a.prof && l < kProfWords) a.prof[(uint64_t)wave_id * kProfWords + l] = v;
    }
#endif
    flush_counters(a, n_q, n_rx, n_miss, lane);
#if ARX_TRACE_COUNT  // [4] node steps, [5] leaf triangle tests (lane level), [6] leader-node lane-steps, [7] step slots
    atomicAdd(a.counters + 4, (unsigned long long)n_steps);
    atomicAdd(a.counters + 5, (unsigned long long)n_tris);
    atomicAdd(a.counters + 6, (unsigned long long)n_leader);
    atomicAdd(a.counters + 7, (unsigned long long)n_slots);
#endif
}

__global__ void finalize_ir_kernel(const long long* __restrict__ hist, float* __restrict__ L, float* __restrict__ R,
                                   int32_t ir_len, double unit, int32_t mono) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ir_len) return;
    float l = (float)((double)hist[k] * unit);
    float r = (float)((double)hist[ir_len + k] * unit);
    if (mono) {  // addIRs (kernels.cu:519-527)
        const float s = l + r;
        l = s;
        r = s;
    }
    L[k] = l;
    R[k] = r;
}

// dst += src over n int64 bins (a group's shards summed on one device, arx_group.cpp).
__global__ void hist_add_kernel(long long* __restrict__ dst, const long long* __restrict__ src, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

// Histogram and counters zeroed in one launch (arx_clear_histogram; two memsets were two
// launches of a few microseconds each, one of them for a few dozen bytes).
__global__ void clear_kernel(unsigned long long* __restrict__ hist, uint64_t n, unsigned long long* __restrict__ counters,
                             int n_counters) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hist[i] = 0ull;
    if (i < (uint64_t)n_counters) counters[i] = 0ull;
}

// Direction pre-pass: float4(dir, 0) for rays [first, first + count); with clear_bins > 0 it also
// zeroes the histogram and the counters the trace accumulates into (render(): one launch fewer per
// frame, and the kernel boundary it cost).
__global__ void dirs_kernel(uint64_t seed, uint64_t first, uint64_t count, float4* out, unsigned long long* cursor,
                            unsigned long long* __restrict__ hist, uint64_t clear_bins,
                            unsigned long long* __restrict__ counters, int clear_counters) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *cursor = 0ull;  // the trace launch's chunk pool (trace_kernel) starts empty-handed
    if (i < clear_bins) hist[i] = 0ull;
    if (i < (uint64_t)clear_counters) counters[i] = 0ull;
    if (i >= count) return;
    const float3 d = ray_direction(seed, first + i);
    out[i] = make_float4(d.x, d.y, d.z, 0.0f);
}

// ------------------------------------------------- longest-first ray pool ---
// The pool hands out direction-buffer slots [n_static, n) in order, so the order of those slots is
// the order rays start in; the rays that start last set the launch's tail.  After a measuring launch
// (trace_kernel<MEASURE>) a counting sort by descending cost rewrites the pool's slots into the frame
// set's second buffer: a histogram over cost >> kOrderShift (LDS per block, then global), a one-block
// scan, and a scatter that gives each slot a place in its bin (the order inside a bin is free: the
// histogram and the counters do not depend on the order rays run in).  Slots below n_static are
// copied as they are.
constexpr int kOrderShift = 3;
constexpr int kOrderBins = 65536 >> kOrderShift;  // 8192 bins of 8 steps (a C3 ray takes 566 +- 94)
constexpr int kOrderTile = 8192;                  // slots per block of the histogram pass
constexpr int kOrderScanBlock = 1024;
static_assert(kOrderBins % kOrderScanBlock == 0, "the scan gives each lane a whole number of bins");
__device__ __forceinline__ uint32_t order_bin(unsigned short cost) {  // the costliest rays in bin 0
    return (uint32_t)(kOrderBins - 1) - ((uint32_t)cost >> kOrderShift);
}

__global__ __launch_bounds__(256) void order_hist_kernel(const unsigned short* __restrict__ cost, uint64_t n_static,
                                                         uint64_t n, uint32_t* __restrict__ bins) {
    __shared__ uint32_t h[kOrderBins];
    for (int b = threadIdx.x; b < kOrderBins; b += 256) h[b] = 0u;
    __syncthreads();
    const uint64_t base = n_static + (uint64_t)blockIdx.x * kOrderTile;
    const uint64_t end = base + kOrderTile < n ? base + kOrderTile : n;
    for (uint64_t i = base + threadIdx.x; i < end; i += 256) atomicAdd(&h[order_bin(cost[i])], 1u);
    __syncthreads();
    for (int b = threadIdx.x; b < kOrderBins; b += 256)
        if (h[b]) atomicAdd(&bins[b], h[b]);
}

// bins[b] = the number of pool slots in bins [0, b): one block, kOrderBins / kOrderScanBlock bins per lane
__global__ __launch_bounds__(kOrderScanBlock) void order_scan_kernel(uint32_t* __restrict__ bins) {
    constexpr int per = kOrderBins / kOrderScanBlock;
    __shared__ uint32_t part[kOrderScanBlock];
    const int t = threadIdx.x;
    uint32_t v[per], sum = 0u;
#pragma unroll
    for (int k = 0; k < per; ++k) {
        v[k] = bins[t * per + k];
        sum += v[k];
    }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < kOrderScanBlock; off <<= 1) {
        const uint32_t x = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
#pragma unroll
    for (int k = 0; k < per; ++k) {
        bins[t * per + k] = run;
        run += v[k];
    }
}

// One tile of kOrderTile pool slots per block, the histogram pass's tiles.  A slot's rank among its
// tile's slots of the same bin comes from an LDS atomic; one global atomic per (tile, occupied bin)
// then reserves the tile's run in that bin, instead of one per slot on a few dozen hot words (which
// took 0.73 ms at C3; the three passes now take 12 + 5 + 20 us).  The bins hold exactly the n - n_static
// pool slots the histogram pass counted from the same cost buffer, so every destination is in
// [n_static, n).
__global__ __launch_bounds__(256) void order_scatter_kernel(const float4* __restrict__ in,
                                                            const unsigned short* __restrict__ cost, uint64_t n_static,
                                                            uint64_t n, uint32_t* __restrict__ bins,
                                                            float4* __restrict__ out) {
    constexpr int per = kOrderTile / 256;
    __shared__ uint32_t h[kOrderBins];
    for (int b = threadIdx.x; b < kOrderBins; b += 256) h[b] = 0u;
    __syncthreads();
    const uint64_t base = n_static + (uint64_t)blockIdx.x * kOrderTile;
    uint32_t rank[per];
#pragma unroll
    for (int k = 0; k < per; ++k) {
        const uint64_t i = base + (uint64_t)k * 256 + threadIdx.x;
        rank[k] = i < n ? atomicAdd(&h[order_bin(cost[i])], 1u) : 0u;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kOrderBins; b += 256)
        if (h[b]) h[b] = atomicAdd(&bins[b], h[b]);  // the tile's first place in bin b
    __syncthreads();
#pragma unroll
    for (int k = 0; k < per; ++k) {
        const uint64_t i = base + (uint64_t)k * 256 + threadIdx.x;
        if (i < n) out[n_static + h[order_bin(cost[i])] + rank[k]] = in[i];
    }
}


__global__ void ray_dir_kernel(uint64_t seed, uint64_t first, uint64_t count, float* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float3 d = ray_direction(seed, first + i);
    out[3 * i + 0] = d.x;
    out[3 * i + 1] = d.y;
    out[3 * i + 2] = d.z;
}

// Production tuning: 128-lane blocks, exactly kWaves waves per SIMD, shade at
// 12 idle lanes, leaves at 12 pending, 12 node steps per inner iteration.  The ARX_TRACE_* macros
// exist only for design experiments (build.py --exp builds a separate library under
// tools/experiments/); the product build never defines them.
#ifndef ARX_TRACE_THRESH
#define ARX_TRACE_THRESH 12
#endif
#ifndef ARX_TRACE_STEPS
#define ARX_TRACE_STEPS 12
#endif
#ifndef ARX_TRACE_LEAF_THRESH
#define ARX_TRACE_LEAF_THRESH 12
#endif
#ifndef ARX_TRACE_SMALL_BLOCK
#define ARX_TRACE_SMALL_BLOCK 256  // block size of launches without the ray pool (0: kBlock)
#endif
constexpr int kSmallBlock = ARX_TRACE_SMALL_BLOCK;
// ... and their node steps per inner iteration / pending leaves before a leaf batch: shorter
// iterations suit a launch whose time is its longest lane chain (C2 0.419 -> 0.403 ms with 10
// steps, 0.408 with 8 leaves; C3 unchanged within noise, profiles/r03/ab_tune.txt)
#ifndef ARX_TRACE_SMALL_STEPS
#define ARX_TRACE_SMALL_STEPS 10
#endif
#ifndef ARX_TRACE_SMALL_LEAF
#define ARX_TRACE_SMALL_LEAF 8
#endif
constexpr int kSmallSteps = ARX_TRACE_SMALL_STEPS, kSmallLeaf = ARX_TRACE_SMALL_LEAF;
// waves per SIMD the small-launch instance is compiled for
constexpr int kSmallWaves = ARX_TRACE_WAVES;
constexpr int kThresh = ARX_TRACE_THRESH, kLeafThresh = ARX_TRACE_LEAF_THRESH, kWaves = ARX_TRACE_WAVES, kSteps = ARX_TRACE_STEPS;
constexpr int kSimdsPerCu = 4;

// Persistent grid of BLOCK-lane blocks: exactly kWaves waves per SIMD on every CU, fewer blocks
// for small launches (one ray per lane).
template <int BLOCK, bool GSTACK, int FMT>
int trace_grid(const TraceArgs& args, int cus, uint64_t n_rays) {
    constexpr int per_cu = kSimdsPerCu * kWaves * 64 / BLOCK;
    static_assert(per_cu * BLOCK == kSimdsPerCu * kWaves * 64, "blocks must fill the CU's wave slots exactly");
    const uint64_t want = (n_rays + BLOCK - 1) / BLOCK;
    uint64_t cap = (uint64_t)per_cu * (uint64_t)(cus > 0 ? cus : 256);
    if (GSTACK || FMT == kFmtW4) cap = std::min<uint64_t>(cap, args.gstack_lanes / BLOCK);  // one stack column per lane
    return (int)std::max<uint64_t>(1, std::min(want, cap));
}

// The ray pool (and the kBlock instance) for launches with at least kDynMinRaysPerWave rays per wave
// of the full grid; smaller launches take the kSmallBlock instance with static ranges.
template <int FMT, bool GSTACK>
bool uses_pool(const TraceArgs& args, int cus) {
    const uint64_t n_rays = args.ray_end - args.ray_begin;
    const int grid = trace_grid<kBlock, GSTACK, FMT>(args, cus, n_rays);
    return n_rays >= (uint64_t)kDynMinRaysPerWave * (uint64_t)grid * (kBlock / 64);
}

template <int FMT, bool GSTACK>
hipError_t launch(const TraceArgs& args, int cus, hipStream_t s, bool fill_dirs) {
    const uint64_t n_rays = args.ray_end - args.ray_begin;
#ifdef ARX_TRACE_DYN_LDS
    static const size_t dyn_lds = ARX_TRACE_DYN_LDS;  // design experiments only
#else
    static const size_t dyn_lds = 0;
#endif
    const int grid = trace_grid<kBlock, GSTACK, FMT>(args, cus, n_rays);
    TraceArgs a2 = args;
    const bool dyn = uses_pool<FMT, GSTACK>(args, cus);
    a2.dyn_share = dyn ? (uint32_t)kDynShare : 0u;
    a2.dyn_chunk = (uint32_t)kDynChunk;
    // the pre-pass: with the buffer's directions kept from an earlier launch (fill_dirs false) only the
    // fused clear and the pool-cursor reset, which lives in its lane 0 -- so at least one block
    const uint64_t n_fill = fill_dirs ? n_rays : 0;
    const uint64_t pre = std::max<uint64_t>(std::max<uint64_t>(n_fill, args.clear_bins), 1);
    hipLaunchKernelGGL(dirs_kernel, dim3((unsigned)((pre + 255) / 256)), dim3(256), 0, s, args.seed, args.ray_begin,
                       n_fill, reinterpret_cast<float4*>(const_cast<void*>(args.dirs)), args.cursor, args.hist,
                       args.clear_bins, args.counters, args.clear_counters);
    if constexpr (FMT == kFmtQ16 && !GSTACK) {
        if (dyn && args.cost) {  // the measuring instance of the pool kernel
            hipLaunchKernelGGL((trace_kernel<kBlock, kThresh, kLeafThresh, kWaves, kSteps, FMT, GSTACK, false, true>),
                               dim3(grid), dim3(kBlock), dyn_lds, s, a2);
            return hipGetLastError();
        }
    }
    a2.cost = nullptr;
    if (kSmallBlock > 0 && !dyn) {
        // Small launches (about a ray per lane: C2, one 8-GPU rank's C5 shard) in 4-wave blocks,
        // one wave per SIMD each: 0.465 -> 0.44 ms at C2
        constexpr int SB = kSmallBlock > 0 ? kSmallBlock : kBlock;
        const int g2 = trace_grid<SB, GSTACK, FMT>(args, cus, n_rays);
        hipLaunchKernelGGL((trace_kernel<SB, kThresh, kSmallLeaf, kSmallWaves, kSmallSteps, FMT, GSTACK, true>), dim3(g2), dim3(SB),
                           dyn_lds, s, a2);
    } else {
        hipLaunchKernelGGL((trace_kernel<kBlock, kThresh, kLeafThresh, kWaves, kSteps, FMT, GSTACK>), dim3(grid),
                           dim3(kBlock), dyn_lds, s, a2);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_trace(const TraceArgs& a, int cus, hipStream_t s, bool force_global_stack, bool fill_dirs) {
    if (a.ray_end <= a.ray_begin) return hipSuccess;
    (void)hipGetLastError();  // report this launch's error, not a stale one of an earlier runtime call
    if (!a.dirs || !a.cnodes || !a.tris || !a.hist || !a.counters || !a.cursor) return hipErrorInvalidValue;
    if (a.wbuf) {  // CW4: LDS rows + a global overflow column per lane (W4Stack)
        if (!a.gstack || a.gstack_lanes < (uint64_t)kBlock) return hipErrorInvalidValue;
        return launch<kFmtW4, false>(a, cus, s, fill_dirs);
    }
    const bool gstack = force_global_stack || a.bvh_depth + 1 > kLdsStack;
    if (gstack && (!a.gstack || a.gstack_lanes < (uint64_t)kBlock)) return hipErrorInvalidValue;
    if (a.qnodes) return gstack ? launch<kFmtQ16, true>(a, cus, s, fill_dirs) : launch<kFmtQ16, false>(a, cus, s, fill_dirs);
    return gstack ? launch<kFmtF32, true>(a, cus, s, fill_dirs) : launch<kFmtF32, false>(a, cus, s, fill_dirs);
}

#ifndef ARX_TRACE_SRC_ID
#define ARX_TRACE_SRC_ID 0ull  // set by build.py: hash of this kernel's sources and experiment macros
#endif
uint64_t trace_kernel_source_id() { return ARX_TRACE_SRC_ID; }

bool trace_uses_small_block(const TraceArgs& a, int cus, bool force_global_stack) {
    if (kSmallBlock <= 0 || a.ray_end <= a.ray_begin) return false;
    if (a.wbuf) return !uses_pool<kFmtW4, false>(a, cus);
    const bool gstack = force_global_stack || a.bvh_depth + 1 > kLdsStack;
    if (a.qnodes) return gstack ? !uses_pool<kFmtQ16, true>(a, cus) : !uses_pool<kFmtQ16, false>(a, cus);
    return gstack ? !uses_pool<kFmtF32, true>(a, cus) : !uses_pool<kFmtF32, false>(a, cus);
}

bool trace_can_measure(const TraceArgs& a, int cus, bool force_global_stack) {
    if (a.ray_end <= a.ray_begin || a.wbuf || !a.qnodes) return false;
    if (force_global_stack || a.bvh_depth + 1 > kLdsStack) return false;
    return uses_pool<kFmtQ16, false>(a, cus);
}

uint32_t trace_pool_share() { return (uint32_t)kDynShare; }

bool trace_can_cache(const TraceArgs& a, bool force_global_stack) {
    if (a.ray_end <= a.ray_begin || a.wbuf || !a.qnodes) return false;
    return !(force_global_stack || a.bvh_depth + 1 > kLdsStack);
}

hipError_t launch_path_record(const TraceArgs& a, int cus, hipStream_t s) {
    (void)hipGetLastError();
    if (!trace_can_cache(a, false) || !a.dirs || !a.tris || !a.counters || !a.cursor || !a.rec)
        return hipErrorInvalidValue;
    const uint64_t n_rays = a.ray_end - a.ray_begin;
    TraceArgs a2 = a;
    const bool dyn = uses_pool<kFmtQ16, false>(a, cus);
    a2.dyn_share = dyn ? (uint32_t)kDynShare : 0u;
    a2.dyn_chunk = (uint32_t)kDynChunk;
    // the pre-pass without directions or histogram: the scratch counters and the pool cursor zeroed
    hipLaunchKernelGGL(dirs_kernel, dim3(1), dim3(256), 0, s, a.seed, a.ray_begin, (uint64_t)0,
                       reinterpret_cast<float4*>(const_cast<void*>(a.dirs)), a.cursor, (unsigned long long*)nullptr,
                       (uint64_t)0, a.counters, a.clear_counters);
    if (kSmallBlock > 0 && !dyn) {
        constexpr int SB = kSmallBlock > 0 ? kSmallBlock : kBlock;
        const int g2 = trace_grid<SB, false, kFmtQ16>(a, cus, n_rays);
        hipLaunchKernelGGL((trace_kernel<SB, kThresh, kSmallLeaf, kSmallWaves, kSmallSteps, kFmtQ16, false, true, false, true>),
                           dim3(g2), dim3(SB), 0, s, a2);
    } else {
        const int grid = trace_grid<kBlock, false, kFmtQ16>(a, cus, n_rays);
        hipLaunchKernelGGL((trace_kernel<kBlock, kThresh, kLeafThresh, kWaves, kSteps, kFmtQ16, false, false, false, true>),
                           dim3(grid), dim3(kBlock), 0, s, a2);
    }
    return hipGetLastError();
}

int32_t trace_node_cache() { return kNodeCache; }

hipError_t launch_order_pool(const void* dirs_in, void* dirs_out, const unsigned short* cost, uint32_t* bins, uint64_t n,
                             hipStream_t s) {
    (void)hipGetLastError();
    if (!dirs_in || !dirs_out || !cost || !bins) return hipErrorInvalidValue;
    const uint64_t n_static = pool_static_rays(n, (uint32_t)kDynShare);
    if (n_static >= n) return hipSuccess;
    const hipError_t e = hipMemsetAsync(bins, 0, kOrderBins * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const uint64_t tiles = (n - n_static + kOrderTile - 1) / kOrderTile;
    hipLaunchKernelGGL(order_hist_kernel, dim3((unsigned)tiles), dim3(256), 0, s, cost, n_static, n, bins);
    hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(kOrderScanBlock), 0, s, bins);
    hipLaunchKernelGGL(order_scatter_kernel, dim3((unsigned)tiles), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(dirs_in), cost, n_static, n, bins,
                       reinterpret_cast<float4*>(dirs_out));
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess || n_static == 0) return e2;
    return hipMemcpyAsync(dirs_out, dirs_in, n_static * 16, hipMemcpyDeviceToDevice, s);  // the static ranges as they are
}
size_t order_bins_bytes() { return kOrderBins * sizeof(uint32_t); }

namespace {
template <int B, int L, int S, bool LEAN>
const void* lds_stack_instance(int fmt) {
    constexpr int W = LEAN ? kSmallWaves : kWaves;
    return fmt == kFmtW4    ? reinterpret_cast<const void*>(trace_kernel<B, kThresh, L, W, S, kFmtW4, false, LEAN>)
           : fmt == kFmtQ16 ? reinterpret_cast<const void*>(trace_kernel<B, kThresh, L, W, S, kFmtQ16, false, LEAN>)
                            : reinterpret_cast<const void*>(trace_kernel<B, kThresh, L, W, S, kFmtF32, false, LEAN>);
}
}  // namespace

hipError_t trace_kernel_occupancy(int fmt, int instance, int* vgprs, int* waves_admitted, int* waves_target) {
    hipFuncAttributes fa;
    constexpr int SB = kSmallBlock > 0 ? kSmallBlock : kBlock;
    const bool small = instance == kInstSmall;
    const void* k = small ? lds_stack_instance<SB, kSmallLeaf, kSmallSteps, true>(fmt)
                          : lds_stack_instance<kBlock, kLeafThresh, kSteps, false>(fmt);
    if (instance == kInstMeasure && fmt == kFmtQ16)  // the other formats have no measuring instance: their pool one
        k = reinterpret_cast<const void*>(
            trace_kernel<kBlock, kThresh, kLeafThresh, kWaves, kSteps, kFmtQ16, false, false, true>);
    const hipError_t e = hipFuncGetAttributes(&fa, k);
    if (e != hipSuccess) return e;
    // gfx950: 512 VGPRs per SIMD lane slot, allocated in granules of 8
    const int alloc = (fa.numRegs + 7) / 8 * 8;
    *vgprs = fa.numRegs;
    *waves_admitted = alloc > 0 ? std::min(8, 512 / alloc) : 8;
    *waves_target = small ? kSmallWaves : kWaves;
    return hipSuccess;
}

hipError_t launch_finalize_ir(const long long* hist, float* ir_left, float* ir_right, int32_t ir_len, double unit,
                              int32_t is_mono, hipStream_t s) {
    (void)hipGetLastError();
    const int b = 256;
    const int g = (ir_len + b - 1) / b;
    if (g > 0) hipLaunchKernelGGL(finalize_ir_kernel, dim3(g), dim3(b), 0, s, hist, ir_left, ir_right, ir_len, unit, is_mono);
    return hipGetLastError();
}

hipError_t launch_hist_add(long long* dst, const long long* src, uint64_t n, hipStream_t s) {
    (void)hipGetLastError();
    const uint64_t g = (n + 255) / 256;
    if (g > 0) hipLaunchKernelGGL(hist_add_kernel, dim3((unsigned)g), dim3(256), 0, s, dst, src, n);
    return hipGetLastError();
}

hipError_t launch_clear(unsigned long long* hist, uint64_t n, unsigned long long* counters, int n_counters,
                        hipStream_t s) {
    (void)hipGetLastError();
    const uint64_t m = n > (uint64_t)n_counters ? n : (uint64_t)n_counters;
    const uint64_t g = (m + 255) / 256;
    if (g > 0) hipLaunchKernelGGL(clear_kernel, dim3((unsigned)g), dim3(256), 0, s, hist, n, counters, n_counters);
    return hipGetLastError();
}

hipError_t launch_ray_directions(uint64_t seed, uint64_t first, uint64_t count, float* d_out, hipStream_t s) {
    (void)hipGetLastError();
    const int b = 256;
    const uint64_t g = (count + b - 1) / b;
    if (g > 0) hipLaunchKernelGGL(ray_dir_kernel, dim3((unsigned)g), dim3(b), 0, s, seed, first, count, d_out);
    return hipGetLastError();
}

}  // namespace arx
