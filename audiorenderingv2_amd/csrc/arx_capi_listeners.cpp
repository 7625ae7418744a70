// arx_capi_listeners.cpp -- a batch of listeners behind the C ABI (arx_render_listeners, include/arx.h):
// every pose's frame from one walk over the path cache's records (listeners_replay_kernel,
// arx_replay.hip), in chunks of receiver slots behind the renderer's own tree; the poses the batch cannot
// take go through arx_render one by one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

namespace {

constexpr uint64_t kListenerCounterWords = 16;  // a listener's block: kCounters counters, its candidate tally, padding

// arx_debug_listener_bytes' per-listener terms (include/arx.h)
uint64_t listener_bytes_each(uint64_t n, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris) {
    return listener_slot_bytes(recv_nodes, recv_tris) + sizeof(ListenerEntry) + 16ull * (uint64_t)ir_len +
           kListenerCounterWords * 8 + 3 * sizeof(arx_acoustics) + 8ull * (uint64_t)ir_len + path_filter_list_bytes(n) +
           4 * listener_work_words(n);
}

// One chunk's scratch (ListenerBatch::d_scratch): byte offsets, every region 16-B aligned.
struct ListenerScratch {
    uint64_t lists, list_stride, work, work_stride, table, hist, counters, res, ir, edc, acou, total;
};
ListenerScratch listener_scratch(uint64_t n, int32_t ir_len, int32_t chunk) {
    ListenerScratch s;
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 15) & ~15ull;
        return o;
    };
    const uint64_t J = (uint64_t)chunk;
    s.list_stride = path_filter_list_bytes(n);
    s.lists = take(J * s.list_stride);
    s.work_stride = 4 * listener_work_words(n);
    s.work = take(J * s.work_stride);
    s.table = take(J * sizeof(ListenerEntry));
    s.hist = take(J * 16 * (uint64_t)ir_len);
    s.counters = take(J * kListenerCounterWords * 8);
    s.res = take(J * 3 * sizeof(arx_acoustics));
    s.ir = take(J * 8 * (uint64_t)ir_len);  // the chunk's left IRs, then its right IRs
    s.edc = take(24 * (uint64_t)ir_len);
    s.acou = take(acoustics_scratch_bytes());
    s.total = at;
    return s;
}

// The pinned block of a call of n listeners: table entries by batched order; counter blocks and results by
// batched order in [0, n) and by pose index in [n, 2n) for the poses that went the one-listener route; the
// tree's off-grid flag as the chunks left it.
struct ListenerPinned {
    ListenerEntry* entries;
    unsigned long long* counters;
    arx_acoustics* res;
    unsigned int* flag;
};
size_t listener_pinned_bytes(size_t n) {
    return n * sizeof(ListenerEntry) + 2 * n * kListenerCounterWords * 8 + 2 * n * 3 * sizeof(arx_acoustics) + 16;
}
ListenerPinned listener_pinned(void* base, size_t n) {
    ListenerPinned p;
    char* c = static_cast<char*>(base);
    p.entries = reinterpret_cast<ListenerEntry*>(c);
    c += n * sizeof(ListenerEntry);
    p.counters = reinterpret_cast<unsigned long long*>(c);
    c += 2 * n * kListenerCounterWords * 8;
    p.res = reinterpret_cast<arx_acoustics*>(c);
    c += 2 * n * 3 * sizeof(arx_acoustics);
    p.flag = reinterpret_cast<unsigned int*>(c);
    return p;
}

// The chunk scratch for `chunk` listeners of n rays; false: no room (that size is not tried again).
bool listener_scratch_reserve(arx_renderer* r, uint64_t n, int32_t chunk) {
    ListenerBatch& lb = r->listeners;
    if (lb.d_scratch && lb.rays == n && lb.ir_len == r->ir_len && lb.chunk >= chunk) return true;
    const uint64_t need = listener_scratch(n, r->ir_len, chunk).total;
    if (known_no_room(lb.no_room, need) || sync_renderer(r) != ARX_OK) return false;
    lb.chunk = 0;
    if (!grow_device_optional(&lb.d_scratch, &lb.scratch_bytes, need, need, &lb.no_room)) return false;
    lb.chunk = chunk;
    lb.rays = n;
    lb.ir_len = r->ir_len;
    return true;
}

// One arx_render_listeners call: its arguments, and what its steps hand each other.
struct ListenerCall {
    arx_renderer* r;
    const arx_listener_pose* poses;
    size_t n;
    float* ir_left;
    float* ir_right;
    arx_acoustics* acoustics;
    arx_listener_result* results;
    ListenerPinned pin;
    uint64_t N;      // rays of a frame
    size_t ir_len;
    bool analyse;
    std::vector<int32_t> route;   // per pose: ARX_LISTENER_SINGLE or ARX_LISTENER_BATCHED
    std::vector<size_t> where;    // per pose: its block in pin.counters / pin.res
    std::vector<size_t> batched;  // the batched poses, in batched order
    size_t first = 0;             // poses before it went through the warm-up
    ReplayProbe probe;
    int32_t chunk = 0;            // listeners per chunk
    ListenerSlots sl;             // the receiver slots behind the renderer's own tree; sl.chunk == chunk
    ListenerScratch sc{};
    char* d_base = nullptr;       // the chunk scratch, and in it the slots' histograms, counter blocks and IRs
    unsigned long long* d_hist = nullptr;
    unsigned long long* d_cnt = nullptr;
    float* d_irl = nullptr;
    float* d_irr = nullptr;
    float fgrow = 0.0f;           // the filter's margin on the grid the batch runs on
};

// The one-listener route: the loop's own step, then its outputs queued on the stream.
arx_status render_single(ListenerCall& c, size_t j) {
    arx_renderer* r = c.r;
    const arx_listener_pose& p = c.poses[j];
    arx_status s1 = arx_set_listener(r, p.x, p.y, p.z, p.yaw_deg);
    if (s1 == ARX_OK) s1 = arx_render(r, nullptr);
    if (s1 == ARX_OK && c.analyse && !r->cur().acou.queued) s1 = arx_analyze_ir(r);
    if (s1 != ARX_OK) return s1;
    const arx_renderer::FrameSet& f = r->cur();
    const size_t ir_len = c.ir_len;
    c.where[j] = c.n + j;
    if (c.ir_left) {
        ARX_HIP(hipMemcpyAsync(c.ir_left + j * ir_len, f.d_ir, ir_len * sizeof(float), hipMemcpyDefault, r->stream));
        ARX_HIP(hipMemcpyAsync(c.ir_right + j * ir_len, f.d_ir + ir_len, ir_len * sizeof(float), hipMemcpyDefault,
                               r->stream));
    }
    unsigned long long* hc = c.pin.counters + c.where[j] * kListenerCounterWords;
    hc[kCounters] = 0;
    ARX_HIP(hipMemcpyAsync(hc, f.d_counters, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->stream));
    if (c.analyse)
        ARX_HIP(hipMemcpyAsync(c.pin.res + 3 * c.where[j], f.acou.d_res, 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost,
                               r->stream));
    c.route[j] = ARX_LISTENER_SINGLE;
    return ARX_OK;
}

// 1. the warm-up: the next pose through arx_render proper until the key is recorded with its filter state
arx_status warm_up(ListenerCall& c) {
    arx_renderer* r = c.r;
    arx_status st;
    for (; c.first < c.n; ++c.first) {
        if ((st = trace_rays(r, 0, c.N, false, false, &c.probe)) != ARX_OK) return st;
        const bool can = c.probe.ready && r->recv_refit && !r->recv.tris.empty() && !r->use_w4 && c.N > 0 &&
                         r->cfg.max_bounces <= kFilterMaxBounces;
        if (can) break;
        if ((st = render_single(c, c.first)) != ARX_OK) return st;
    }
    return ARX_OK;
}

// 2. the batched poses: grid, slots and scratch before the first launch; any "no" sends the rest through
// the loop.  *batch: the poses from c.first on may be batched, c.chunk at a time.
arx_status prepare_batch(ListenerCall& c, bool* batch) {
    arx_renderer* r = c.r;
    ListenerBatch& lb = r->listeners;
    arx_status st;
    *batch = c.first < c.n;
    if (*batch) {
        if ((st = listener_grid_for(r, c.poses, c.first, c.n)) != ARX_OK) return st;
    }
    c.sl = listener_slots(r);
    if (*batch) {
        const uint64_t each = listener_bytes_each(c.N, r->ir_len, c.sl.recv_nodes, c.sl.recv_tris);
        c.chunk = lb.forced_chunk > 0 ? lb.forced_chunk : (int32_t)std::min<uint64_t>(kListenerChunkMax, kListenerBudget / each);
        c.chunk = (int32_t)std::min<size_t>((size_t)c.chunk, c.n - c.first);
        *batch = c.chunk >= 1;
    }
    c.sl.chunk = c.chunk;
    if (*batch) {
        const ListenerLayout last = c.sl.layout(c.chunk - 1);
        *batch = listener_slots_valid(r, c.sl) && widen_tree_arrays(r, (size_t)last.total_nodes, (size_t)last.total_tris) &&
                 listener_scratch_reserve(r, c.N, c.chunk);
        c.chunk = std::min(c.chunk, std::max(lb.chunk, 0));
    }
    if (c.chunk != c.sl.chunk) *batch = false;  // the slots were checked for the chunk asked for
    if (*batch) {
        // the arrays may have moved and the grid grown: the replay's arguments as they stand now
        if ((st = trace_rays(r, 0, c.N, false, false, &c.probe)) != ARX_OK) return st;
        *batch = c.probe.ready && c.chunk >= 1;
    }
    c.sc = listener_scratch(lb.rays, lb.ir_len, std::max(lb.chunk, 1));
    c.d_base = static_cast<char*>(lb.d_scratch);
    c.d_hist = reinterpret_cast<unsigned long long*>(c.d_base + c.sc.hist);
    c.d_cnt = reinterpret_cast<unsigned long long*>(c.d_base + c.sc.counters);
    c.d_irl = reinterpret_cast<float*>(c.d_base + c.sc.ir);
    c.d_irr = c.d_irl + (size_t)lb.chunk * c.ir_len;
    c.fgrow = *batch ? path_filter_grow(c.probe.args.qgrid) : 0.0f;
    return ARX_OK;
}

// Which poses are batched: not those whose box holds the emitter (every ray a candidate), nor one off the
// grid.  Each gets its table entry, in batched order, with the slot of its chunk it runs in.
void select_batched(ListenerCall& c) {
    const arx_renderer* r = c.r;
    const ListenerScratch& sc = c.sc;
    for (size_t j = c.first; j < c.n; ++j) {
        if (!listener_pose_batchable(r, c.poses[j], c.fgrow)) continue;
        const size_t b = c.batched.size();
        const int32_t slot = (int32_t)(b % (size_t)c.chunk);
        ListenerEntry& e = c.pin.entries[b];
        listener_entry_place(r, c.sl, slot, c.poses[j], &e);
        e.hist = c.d_hist + (size_t)slot * 2 * c.ir_len;
        e.counters = c.d_cnt + (size_t)slot * kListenerCounterWords;
        e.cand = e.counters + kCounters;
        e.list = reinterpret_cast<FilterCand*>(c.d_base + sc.lists + (uint64_t)slot * sc.list_stride);
        e.heads = e.list + c.N;
        e.work = reinterpret_cast<unsigned int*>(c.d_base + sc.work + (uint64_t)slot * sc.work_stride);
        c.where[j] = b;
        c.route[j] = ARX_LISTENER_BATCHED;
        c.batched.push_back(j);
    }
}

// The call's last pose is the renderer's last frame: slot i of the chunk becomes the next frame set's
// histogram, counters, IR, candidate list and analysis, and the listener the renderer holds.
arx_status adopt_last_frame(ListenerCall& c, int32_t i) {
    arx_renderer* r = c.r;
    const ListenerScratch& sc = c.sc;
    const size_t ir_len = c.ir_len;
    const uint64_t N = c.N;
    arx_status st;
    if ((st = begin_frame(r)) != ARX_OK) return st;
    arx_renderer::FrameSet& f = r->cur();
    ARX_HIP(hipMemcpyAsync(f.d_hist, c.d_hist + (size_t)i * 2 * ir_len, 2 * ir_len * sizeof(unsigned long long),
                           hipMemcpyDeviceToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(f.d_counters, c.d_cnt + (size_t)i * kListenerCounterWords, kCounters * sizeof(unsigned long long),
                           hipMemcpyDeviceToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(f.d_ir, c.d_irl + (size_t)i * ir_len, ir_len * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(f.d_ir + ir_len, c.d_irr + (size_t)i * ir_len, ir_len * sizeof(float), hipMemcpyDeviceToDevice,
                           r->stream));
    PathCache& pc = r->path_cache;
    pc.state = kPathReplayed;
    pc.last_key = pc.key;
    pc.last_valid = true;
    pc.last_filtered = false;
    if (path_filter_list_reserve(r, N)) {
        ARX_HIP(hipMemcpyAsync(f.d_filter_list, c.d_base + sc.lists + (uint64_t)i * sc.list_stride, N * sizeof(FilterCand),
                               hipMemcpyDeviceToDevice, r->stream));
        ARX_HIP(hipMemcpyAsync(static_cast<FilterCand*>(f.d_filter_list) + f.filter_list_cap,
                               c.d_base + sc.lists + (uint64_t)i * sc.list_stride + N * sizeof(FilterCand),
                               16 * path_filter_heads(N), hipMemcpyDeviceToDevice, r->stream));
        pc.last_filtered = true;
        pc.filter_slot = r->slot;
        pc.filter_rays = N;
    }
    r->conv_ir_dirty = true;
    r->conv_live_ir_dirty = true;
    const arx_listener_pose& p = c.poses[c.n - 1];
    r->center[0] = p.x; r->center[1] = p.y; r->center[2] = p.z;
    r->yaw = p.yaw_deg;
    if ((c.analyse || r->auto_analyze) && (st = arx_analyze_ir(r)) != ARX_OK) return st;
    return ARX_OK;
}

// One chunk, on the one stream: the batched poses [c0, c0 + J) refit into their slots, replayed, finalized
// and analysed, and their outputs queued.
arx_status issue_chunk(ListenerCall& c, size_t c0, int32_t J) {
    arx_renderer* r = c.r;
    const ListenerScratch& sc = c.sc;
    const size_t ir_len = c.ir_len;
    const double unit = ir_unit(r->cfg);
    ListenerEntry* d_table = reinterpret_cast<ListenerEntry*>(c.d_base + sc.table);
    arx_acoustics* d_res = reinterpret_cast<arx_acoustics*>(c.d_base + sc.res);
    ARX_HIP(hipMemcpyAsync(d_table, c.pin.entries + c0, (size_t)J * sizeof(ListenerEntry), hipMemcpyHostToDevice, r->stream));
    ARX_HIP(launch_clear(c.d_hist, (uint64_t)J * 2 * ir_len, c.d_cnt, (int)(J * kListenerCounterWords), r->stream));
    ARX_HIP(launch_receiver_refit_multi(refit_args(r), d_table, J, r->stream));
    FilterArgs fa;
    fa.planes = c.probe.planes;
    fa.list = nullptr;  // per listener, from the table
    fa.heads = nullptr;
    fa.grow = c.fgrow;
    ARX_HIP(launch_listeners_replay(c.probe.args, fa, d_table, J, r->stream));
    for (int32_t i = 0; i < J; ++i) {
        const size_t j = c.batched[c0 + (size_t)i];
        const long long* h = reinterpret_cast<const long long*>(c.d_hist + (size_t)i * 2 * ir_len);
        float* il = c.d_irl + (size_t)i * ir_len;
        float* irr = c.d_irr + (size_t)i * ir_len;
        ARX_HIP(launch_finalize_ir(h, il, irr, r->ir_len, unit, r->cfg.is_mono, r->stream));
        ++r->ir_generation;
        if (c.analyse)
            ARX_HIP(launch_acoustics(acoustics_args(r, h, reinterpret_cast<long long*>(c.d_base + sc.edc), d_res + 3 * i,
                                                    c.d_base + sc.acou),
                                     r->stream));
        if (c.ir_left) {
            ARX_HIP(hipMemcpyAsync(c.ir_left + j * ir_len, il, ir_len * sizeof(float), hipMemcpyDefault, r->stream));
            ARX_HIP(hipMemcpyAsync(c.ir_right + j * ir_len, irr, ir_len * sizeof(float), hipMemcpyDefault, r->stream));
        }
    }
    ARX_HIP(hipMemcpyAsync(c.pin.counters + c0 * kListenerCounterWords, c.d_cnt, (size_t)J * kListenerCounterWords * 8,
                           hipMemcpyDeviceToHost, r->stream));
    if (c.analyse)
        ARX_HIP(hipMemcpyAsync(c.pin.res + 3 * c0, d_res, (size_t)J * 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipMemcpyAsync(c.pin.flag, r->d_tree_flag, sizeof(unsigned int), hipMemcpyDeviceToHost, r->stream));
    c.pin.flag[1] = r->tree_gen;
    if (c.batched.back() == c.n - 1 && c0 + (size_t)J == c.batched.size()) return adopt_last_frame(c, J - 1);
    return ARX_OK;
}

// 5. the host-side outputs, after the call's one synchronisation
void write_outputs(const ListenerCall& c) {
    for (size_t j = 0; j < c.n; ++j) {
        const unsigned long long* hc = c.pin.counters + c.where[j] * kListenerCounterWords;
        if (c.results) {
            arx_listener_result& o = c.results[j];
            std::memset(&o, 0, sizeof(o));
            o.queries = hc[0];
            o.receiver_hits = hc[1];
            o.misses = hc[2];
            o.candidate_rays = c.route[j] == ARX_LISTENER_BATCHED ? hc[kCounters] : 0;
            o.route = c.route[j];
        }
        if (c.analyse) std::memcpy(c.acoustics + 3 * j, c.pin.res + 3 * c.where[j], 3 * sizeof(arx_acoustics));
    }
}

arx_status render_listeners(ListenerCall& c) {
    arx_renderer* r = c.r;
    const size_t n = c.n;
    arx_status st;
    if ((st = warm_up(c)) != ARX_OK) return st;
    bool batch = false;
    if ((st = prepare_batch(c, &batch)) != ARX_OK) return st;
    if (batch) select_batched(c);
    // 3. the poses that take the one-listener route in place; the call's last pose waits, so that its frame is the last
    for (size_t j = c.first; j + 1 < n; ++j)
        if (c.route[j] == ARX_LISTENER_SINGLE && (st = render_single(c, j)) != ARX_OK) return st;
    // 4. the chunks
    for (size_t c0 = 0; c0 < c.batched.size(); c0 += (size_t)c.chunk) {
        const int32_t J = (int32_t)std::min<size_t>((size_t)c.chunk, c.batched.size() - c0);
        if ((st = issue_chunk(c, c0, J)) != ARX_OK) return st;
    }
    if (n >= 1 && c.first < n && c.route[n - 1] == ARX_LISTENER_SINGLE && (st = render_single(c, n - 1)) != ARX_OK) return st;
    // 5. the one synchronisation, then the host-side outputs
    ARX_HIP(hipStreamSynchronize(r->stream));
    if (!c.batched.empty() && c.pin.flag[1] != 0 && c.pin.flag[0] == c.pin.flag[1])
        return fail(ARX_ERR_INTERNAL, "receiver refit / re-quantization: a box left the quantization grid");
    write_outputs(c);
    return ARX_OK;
}

}  // namespace

// ---- what arx_render_listener_bands (arx_capi_listener_bands.cpp) shares with the call above ----

uint64_t arx::listener_slot_bytes(int64_t recv_nodes, int64_t recv_tris) {
    return (uint64_t)recv_nodes * (sizeof(BvhNode) + sizeof(QNode2)) + (uint64_t)recv_tris * sizeof(TriRec) +
           (sizeof(BvhNode) + sizeof(QNode2));
}

ListenerLayout arx::ListenerSlots::layout(int32_t slot) const {
    return listener_layout(own_nodes, own_tris, recv_nodes, recv_tris, chunk, slot, trace_node_cache());
}

ListenerSlots arx::listener_slots(const arx_renderer* r) {
    ListenerSlots s;
    s.recv_nodes = (int64_t)r->recv.nodes.size();
    s.recv_tris = (int64_t)r->recv.tris.size();
    s.own_nodes = r->scene_img ? 1 + (int64_t)r->scene_img->bvh.nodes.size() + s.recv_nodes : 0;
    s.own_tris = r->scene_img ? (int64_t)r->scene_img->bvh.tris.size() + s.recv_tris : 0;
    return s;
}

// the union of the poses' receiver bounds on the grid (grown once if need be)
arx_status arx::listener_grid_for(arx_renderer* r, const arx_listener_pose* poses, size_t first, size_t n) {
    float ulo[3] = {1e30f, 1e30f, 1e30f}, uhi[3] = {-1e30f, -1e30f, -1e30f};
    for (size_t j = first; j < n; ++j) {
        const float centre[3] = {poses[j].x, poses[j].y, poses[j].z};
        float lo[3], hi[3];
        bool empty = false;
        receiver_bound(r, centre, lo, hi, &empty);
        for (int k = 0; k < 3; ++k) {
            ulo[k] = std::min(ulo[k], lo[k]);
            uhi[k] = std::max(uhi[k], hi[k]);
        }
    }
    if (!qgrid_contains(r->qgrid, ulo, uhi)) return grow_grid_for(r, ulo, uhi);
    return ARX_OK;
}

// The extended tree must pass the kernels' offset limits and the structural check, slot by slot.
bool arx::listener_slots_valid(const arx_renderer* r, const ListenerSlots& c) {
    const ListenerLayout last = c.layout(c.chunk - 1);
    if (check_buffer_offsets((size_t)last.total_nodes, (size_t)last.total_tris) != ARX_OK) return false;
    std::vector<BvhNode> moved(r->recv.nodes);
    for (int32_t s = 0; s < c.chunk; s += std::max(1, c.chunk - 1)) {  // the first and the last slot
        const ListenerLayout l = c.layout(s);
        const int32_t ns = (int32_t)(l.node_begin - (c.own_nodes - c.recv_nodes)), ts = (int32_t)(l.tri_begin - (c.own_tris - c.recv_tris));
        for (size_t i = 0; i < moved.size(); ++i)
            for (int k = 0; k < 2; ++k) {
                const int32_t cnt = r->recv.nodes[i].d[2 + k];
                moved[i].d[k] = r->recv.nodes[i].d[k] + (cnt == 0 ? ns : cnt > 0 ? ts : 0);
            }
        const char* why = "";
        if (!validate_bvh_range(moved.data(), (size_t)l.node_begin, moved.size(), (size_t)last.total_nodes,
                                (size_t)last.total_tris, &why))
            return false;
    }
    return true;
}

// Not batched: a pose whose box holds the emitter (every ray a candidate), or one off the grid.
bool arx::listener_pose_batchable(const arx_renderer* r, const arx_listener_pose& p, float fgrow) {
    const float centre[3] = {p.x, p.y, p.z};
    float lo[3], hi[3];
    bool empty = false;
    receiver_bound(r, centre, lo, hi, &empty);
    return !emitter_in_receiver_box(r, centre, 2.0f * fgrow) && qgrid_contains(r->qgrid, lo, hi);
}

// A table entry's pose and slot: centre, top node, the refit's rotation, padding and shifts; its pointers zero.
void arx::listener_entry_place(const arx_renderer* r, const ListenerSlots& s, int32_t slot, const arx_listener_pose& p,
                               ListenerEntry* e) {
    const float centre[3] = {p.x, p.y, p.z};
    const ListenerLayout l = s.layout(slot);
    std::memset(e, 0, sizeof(*e));
    for (int k = 0; k < 3; ++k) e->center[k] = centre[k];
    e->top = (int32_t)l.top;
    receiver_rotation(p.yaw_deg, e->m);
    e->pad = refit_pad(r, centre);
    e->node_shift = (int32_t)(l.node_begin - (s.own_nodes - s.recv_nodes));
    e->tri_shift = (int32_t)(l.tri_begin - (s.own_tris - s.recv_tris));
}

void arx::free_listener_batch(ListenerBatch& b) {
    hipFree(b.d_scratch);
    if (b.h_pinned) hipHostFree(b.h_pinned);
    if (b.ev0) hipEventDestroy(b.ev0);
    if (b.ev1) hipEventDestroy(b.ev1);
    const int32_t forced = b.forced_chunk;
    b = ListenerBatch{};
    b.forced_chunk = forced;
}

extern "C" {

arx_status arx_render_listeners(arx_renderer* r, const arx_listener_pose* poses, size_t n, float* ir_left, float* ir_right,
                                arx_acoustics* acoustics, arx_listener_result* results, double* ms) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n == 0) return ARX_OK;
    if (!poses) return fail(ARX_ERR_INVALID_ARGUMENT, "poses is NULL");
    if ((ir_left == nullptr) != (ir_right == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ir_left and ir_right: both or neither");
    for (size_t j = 0; j < n; ++j)
        if (!std::isfinite(poses[j].x) || !std::isfinite(poses[j].y) || !std::isfinite(poses[j].z) ||
            !std::isfinite(poses[j].yaw_deg))
            return fail(ARX_ERR_INVALID_ARGUMENT, "pose %zu is not finite", j);
    if (r->fif != 1) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs one frame in flight");
    if (r->stream != r->cur().stream) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own stream");
    if (r->d_hist_ext) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own histogram");
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    ARX_HIP(hipSetDevice(r->cfg.device));
    ListenerBatch& lb = r->listeners;
    if (n > lb.h_listeners) {  // nothing of an earlier call is in flight: every call ends synchronised
        if (lb.h_pinned) hipHostFree(lb.h_pinned);
        lb.h_pinned = nullptr;
        lb.h_listeners = 0;
        ARX_HIP(hipHostMalloc(&lb.h_pinned, listener_pinned_bytes(n), hipHostMallocDefault));
        lb.h_listeners = n;
    }
    ListenerCall c{r, poses, n, ir_left, ir_right, acoustics, results, listener_pinned(lb.h_pinned, n)};
    c.N = n_rays(r->cfg);
    c.ir_len = (size_t)r->ir_len;
    c.analyse = acoustics != nullptr;
    c.route.assign(n, ARX_LISTENER_SINGLE);
    c.where.assign(n, 0);
    c.pin.flag[0] = c.pin.flag[1] = 0u;
    const bool timed = r->timing || ms != nullptr;
    if (timed) {
        if (!lb.ev0) ARX_HIP(hipEventCreate(&lb.ev0));
        if (!lb.ev1) ARX_HIP(hipEventCreate(&lb.ev1));
        ARX_HIP(hipEventRecord(lb.ev0, r->stream));
    }
    const float saved[4] = {r->center[0], r->center[1], r->center[2], r->yaw};
    arx_status st = render_listeners(c);
    arx_set_listener(r, saved[0], saved[1], saved[2], saved[3]);  // the listener set before the call, refit by the next frame
    if (st != ARX_OK) return st;
    if (timed) {
        ARX_HIP(hipEventRecord(lb.ev1, r->stream));
        ARX_HIP(hipEventSynchronize(lb.ev1));
        float t = 0.0f;
        ARX_HIP(hipEventElapsedTime(&t, lb.ev0, lb.ev1));
        if (ms) *ms = (double)t;
    }
    return ARX_OK;
}

arx_status arx_debug_set_listener_chunk(arx_renderer* r, int32_t listeners) {
    if (!r || listeners < 0 || listeners > kListenerChunkMax)
        return fail(ARX_ERR_INVALID_ARGUMENT, "listener chunk: 0 (automatic) or 1..%d", kListenerChunkMax);
    r->listeners.forced_chunk = listeners;
    return ARX_OK;
}

uint64_t arx_debug_listener_bytes(uint64_t n_rays, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t listeners) {
    if (ir_len < 0 || recv_nodes < 0 || recv_tris < 0 || listeners < 0) return 0;
    return (uint64_t)listeners * listener_bytes_each(n_rays, ir_len, recv_nodes, recv_tris);
}

arx_status arx_debug_listener_layout(int64_t n_scene_nodes, int64_t n_scene_tris, int64_t recv_nodes, int64_t recv_tris,
                                     int32_t listeners, int32_t slot, int64_t out5[5]) {
    if (!out5 || n_scene_nodes < 0 || n_scene_tris < 0 || recv_nodes < 0 || recv_tris < 0 || listeners < 1 ||
        listeners > kListenerChunkMax || slot < 0 || slot >= listeners)
        return fail(ARX_ERR_INVALID_ARGUMENT, "bad listener layout arguments");
    const ListenerLayout l = listener_layout(1 + n_scene_nodes + recv_nodes, n_scene_tris + recv_tris, recv_nodes, recv_tris,
                                             listeners, slot, trace_node_cache());
    const arx_status fit = check_buffer_offsets((size_t)l.total_nodes, (size_t)l.total_tris);
    if (fit != ARX_OK) return fit;
    out5[0] = l.node_begin;
    out5[1] = l.node_begin + recv_nodes;
    out5[2] = l.tri_begin;
    out5[3] = l.tri_begin + recv_tris;
    out5[4] = l.top;
    return ARX_OK;
}

}  // extern "C"
