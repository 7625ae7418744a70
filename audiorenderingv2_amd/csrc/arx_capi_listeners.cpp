// arx_capi_listeners.cpp -- a batch of listeners behind the C ABI (arx_render_listeners, include/arx.h):
// every pose's frame from one walk over the path cache's records (filter_multi_kernel + cand_work_kernel +
// replay_cand_multi_kernel, arx_replay.hip), in chunks of receiver slots behind the renderer's own tree; the
// poses the batch cannot take go through arx_render one by one.  The driver of a batched call
// (run_listener_call) is here too: arx_render_listener_bands (arx_capi_listener_bands.cpp) runs on it with
// its own steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arx_internal.hpp"

using namespace arx;

namespace {

// ---- the driver's steps, the same for both calls ----

ListenerSlots listener_slots(const arx_renderer* r) {  // chunk left 0
    ListenerSlots s;
    s.recv_nodes = (int64_t)r->recv.nodes.size();
    s.recv_tris = (int64_t)r->recv.tris.size();
    s.own_nodes = r->scene_img ? 1 + (int64_t)r->scene_img->bvh.nodes.size() + s.recv_nodes : 0;
    s.own_tris = r->scene_img ? (int64_t)r->scene_img->bvh.tris.size() + s.recv_tris : 0;
    return s;
}

// The quantization grid grown once, if need be, to hold the receivers of poses [first, n).
arx_status listener_grid_for(arx_renderer* r, const arx_listener_pose* poses, size_t first, size_t n) {
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
bool listener_slots_valid(const arx_renderer* r, const ListenerSlots& c) {
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
bool listener_pose_batchable(const arx_renderer* r, const arx_listener_pose& p, float fgrow) {
    const float centre[3] = {p.x, p.y, p.z};
    float lo[3], hi[3];
    bool empty = false;
    receiver_bound(r, centre, lo, hi, &empty);
    return !emitter_in_receiver_box(r, centre, 2.0f * fgrow) && qgrid_contains(r->qgrid, lo, hi);
}

// A table entry's pose and slot: centre, top node, the refit's rotation, padding and shifts; its pointers zero.
void listener_entry_place(const arx_renderer* r, const ListenerSlots& s, int32_t slot, const arx_listener_pose& p,
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

// The chunk scratch of `need` bytes; false: no room (that size is not tried again).
bool scratch_reserve(arx_renderer* r, ListenerScratch& lb, uint64_t need) {
    if (lb.d_scratch.p && need <= lb.d_scratch.cap) return true;
    if (known_no_room(lb.no_room, need) || sync_renderer(r) != ARX_OK) return false;
    return lb.d_scratch.try_reserve(need, &lb.no_room);
}

// The tree's flag as the chunks left it: a box of the chunks' last tree write left the quantization grid.
bool off_grid(const ListenerCall& c) { return !c.batched.empty() && c.h_flag[1] != 0 && c.h_flag[0] == c.h_flag[1]; }

// What the batched kernels need: the key recorded with its filter state, the refit's receiver, 16-bit nodes.
bool can_batch(const ListenerCall& c) {
    const arx_renderer* r = c.r;
    return c.probe.ready && r->recv_refit && !r->recv.tris.empty() && !r->use_w4 && c.N > 0 &&
           r->cfg.max_bounces <= kFilterMaxBounces;
}

// 2. the batched poses: grid, slots and scratch before the first launch; any "no" sends the poses from
// c.first on through the one-listener route.  *batch: they may be batched, c.chunk at a time.
arx_status prepare_batch(ListenerCall& c, bool* batch) {
    arx_renderer* r = c.r;
    arx_status st;
    *batch = c.first < c.n && can_batch(c);
    if (!*batch) return ARX_OK;
    if ((st = listener_grid_for(r, c.poses, c.first, c.n)) != ARX_OK) return st;
    c.sl = listener_slots(r);
    c.chunk = batch_chunk(r->listeners.forced_chunk, kListenerBudget, batch_bytes_fixed(c.N, c.bands),
                          batch_bytes_each(c.N, r->ir_len, c.sl.recv_nodes, c.sl.recv_tris, c.bands), c.n - c.first);
    c.sl.chunk = c.chunk;
    if (c.chunk < 1) {
        *batch = false;
        return ARX_OK;
    }
    const ListenerLayout last = c.sl.layout(c.chunk - 1);
    c.sc = batch_scratch(c.N, r->ir_len, c.bands, c.chunk, acoustics_scratch_bytes());
    *batch = listener_slots_valid(r, c.sl) && widen_tree_arrays(r, (size_t)last.total_nodes, (size_t)last.total_tris) &&
             scratch_reserve(r, *c.own, c.sc.total);
    if (!*batch) return ARX_OK;
    // the arrays may have moved and the grid grown: the replay's arguments as they stand now
    if ((st = trace_rays(r, 0, c.N, false, false, &c.probe)) != ARX_OK) return st;
    *batch = c.probe.ready;
    c.d_base = c.own->d_scratch.p;
    c.fgrow = path_filter_grow(c.probe.args.qgrid);
    return ARX_OK;
}

// Which poses are batched: not those whose box holds the emitter (every ray a candidate), nor one off the
// grid.  Each gets its table entry, in batched order, with the slot of its chunk it runs in.
void select_batched(ListenerCall& c) {
    const BatchScratch& sc = c.sc;
    const uint64_t cells = batch_cells(c.bands), words = batch_counter_words(c.bands);
    for (size_t j = c.first; j < c.n; ++j) {
        if (!listener_pose_batchable(c.r, c.poses[j], c.fgrow)) continue;
        const size_t b = c.batched.size();
        const uint64_t slot = b % (size_t)c.chunk;
        ListenerEntry& e = c.h_entries[b];
        listener_entry_place(c.r, c.sl, (int32_t)slot, c.poses[j], &e);
        e.hist = c.at<unsigned long long>(sc.hist) + slot * cells * 2 * c.ir_len;
        e.counters = c.at<unsigned long long>(sc.counters) + slot * words;
        e.cand = e.counters + cells * kBandCounterWords;
        e.list = c.at<FilterCand>(sc.lists + slot * sc.list_stride);
        e.heads = e.list + c.N;
        e.work = c.at<unsigned int>(sc.work + slot * sc.work_stride);
        c.where[j] = b;
        c.route[j] = ARX_LISTENER_BATCHED;
        c.batched.push_back(j);
    }
}

// The call's last pose is the renderer's last frame: slot i of the chunk becomes the next frame set's
// histogram, counters, IR, candidate list and analysis, and the listener the renderer holds.
arx_status adopt_last_frame(ListenerCall& c, int32_t i) {
    arx_renderer* r = c.r;
    const BatchScratch& sc = c.sc;
    const size_t ir_len = c.ir_len;
    const uint64_t N = c.N;
    arx_status st;
    if ((st = begin_frame(r)) != ARX_OK) return st;
    arx_renderer::FrameSet& f = r->cur();
    const float* d_irl = c.at<float>(sc.ir) + (size_t)i * ir_len;
    const char* d_list = c.d_base + sc.lists + (uint64_t)i * sc.list_stride;
    ARX_HIP(hipMemcpyAsync(f.d_hist.p, c.at<unsigned long long>(sc.hist) + (size_t)i * 2 * ir_len,
                           2 * ir_len * sizeof(unsigned long long), hipMemcpyDeviceToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(f.d_counters.p, c.at<unsigned long long>(sc.counters) + (size_t)i * batch_counter_words(0),
                           kCounters * sizeof(unsigned long long), hipMemcpyDeviceToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(f.d_ir.p, d_irl, ir_len * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
    ARX_HIP(hipMemcpyAsync(f.d_ir.p + ir_len, d_irl + (size_t)c.chunk * ir_len, ir_len * sizeof(float), hipMemcpyDeviceToDevice,
                           r->stream));
    PathCache& pc = r->path_cache;
    pc.state = kPathReplayed;
    pc.last_key = pc.key;
    pc.last_valid = true;
    pc.last_filtered = false;
    if (path_filter_list_reserve(r, N)) {
        ARX_HIP(hipMemcpyAsync(f.d_filter_list.p, d_list, N * sizeof(FilterCand), hipMemcpyDeviceToDevice, r->stream));
        ARX_HIP(hipMemcpyAsync(reinterpret_cast<FilterCand*>(f.d_filter_list.p) + f.filter_list_rays, d_list + N * sizeof(FilterCand),
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
    if ((c.acoustics || r->auto_analyze) && (st = arx_analyze_ir(r)) != ARX_OK) return st;
    return ARX_OK;
}

// A chunk's counter words and results into the pinned block's rows from c0 on, and the tree's flag.
arx_status queue_chunk_results(ListenerCall& c, size_t c0, int32_t J) {
    arx_renderer* r = c.r;
    const size_t cells = (size_t)batch_cells(c.bands), words = (size_t)batch_counter_words(c.bands);
    ARX_HIP(hipMemcpyAsync(c.h_counters + c0 * words, c.at<char>(c.sc.counters), (size_t)J * words * 8, hipMemcpyDeviceToHost,
                           r->stream));
    if (c.acoustics)
        ARX_HIP(hipMemcpyAsync(c.h_res + 3 * cells * c0, c.at<char>(c.sc.res), (size_t)J * cells * 3 * sizeof(arx_acoustics),
                               hipMemcpyDeviceToHost, r->stream));
    ARX_HIP(hipMemcpyAsync(c.h_flag, r->d_tree_flag.p, sizeof(unsigned int), hipMemcpyDeviceToHost, r->stream));
    c.h_flag[1] = r->tree_gen;
    return ARX_OK;
}

// One chunk, on the one stream: the batched poses [c0, c0 + J) refit into their slots, replayed, every cell
// finalized and analysed, and their outputs queued.
arx_status issue_chunk(ListenerCall& c, size_t c0, int32_t J) {
    arx_renderer* r = c.r;
    const BatchScratch& sc = c.sc;
    const size_t L = c.ir_len, cells = (size_t)batch_cells(c.bands), set = cells * L;
    ListenerEntry* d_table = c.at<ListenerEntry>(sc.table);
    unsigned long long* d_hist = c.at<unsigned long long>(sc.hist);
    arx_acoustics* d_res = c.at<arx_acoustics>(sc.res);
    float* d_irl = c.at<float>(sc.ir);
    float* d_irr = d_irl + (size_t)c.chunk * set;
    arx_status st;
    ARX_HIP(hipMemcpyAsync(d_table, c.h_entries + c0, (size_t)J * sizeof(ListenerEntry), hipMemcpyHostToDevice, r->stream));
    ARX_HIP(launch_clear(d_hist, (uint64_t)J * cells * 2 * L, c.at<unsigned long long>(sc.counters),
                         (int)((uint64_t)J * batch_counter_words(c.bands)), r->stream));
    ARX_HIP(launch_receiver_refit_multi(refit_args(r), d_table, J, r->stream));
    if ((st = c.replay(c, d_table, c0, J)) != ARX_OK) return st;
    for (int32_t i = 0; i < J; ++i) {
        const size_t j = c.batched[c0 + (size_t)i];
        for (size_t k = (size_t)i * cells; k < ((size_t)i + 1) * cells; ++k)
            if ((st = finalize_and_analyse(r, d_hist + k * 2 * L, d_irl + k * L, d_irr + k * L, d_res + 3 * k, c.at<char>(sc.edc),
                                           c.at<char>(sc.acou), c.want_ir, c.acoustics != nullptr)) != ARX_OK)
                return st;
        if (c.frames) ++r->ir_generation;
        if (c.ir_left) {
            ARX_HIP(hipMemcpyAsync(c.ir_left + j * set, d_irl + (size_t)i * set, set * sizeof(float), hipMemcpyDefault, r->stream));
            ARX_HIP(hipMemcpyAsync(c.ir_right + j * set, d_irr + (size_t)i * set, set * sizeof(float), hipMemcpyDefault, r->stream));
        }
        if (c.finish_listener && (st = c.finish_listener(c, i, j)) != ARX_OK) return st;
    }
    if ((st = queue_chunk_results(c, c0, J)) != ARX_OK) return st;
    if (c.frames && c.batched.back() == c.n - 1 && c0 + (size_t)J == c.batched.size()) return adopt_last_frame(c, J - 1);
    return ARX_OK;
}

arx_status run_batch(ListenerCall& c) {
    arx_status st;
    if ((st = c.warm_up(c)) != ARX_OK) return st;
    bool batch = false;
    if ((st = prepare_batch(c, &batch)) != ARX_OK) return st;
    if (batch) select_batched(c);
    // 3. the poses that take the one-listener route; where the batched listeners are the renderer's frames, the
    // call's last pose waits, so that its frame is the last
    const size_t wait = c.frames && c.first < c.n && c.route[c.n - 1] == ARX_LISTENER_SINGLE ? 1 : 0;
    for (size_t j = c.first; j + wait < c.n; ++j)
        if (c.route[j] == ARX_LISTENER_SINGLE && (st = c.render_single(c, j)) != ARX_OK) return st;
    // 4. the chunks
    if (!c.batched.empty() && c.begin_chunks && (st = c.begin_chunks(c)) != ARX_OK) return st;
    for (size_t c0 = 0; c0 < c.batched.size(); c0 += (size_t)c.chunk) {
        const int32_t J = (int32_t)std::min<size_t>((size_t)c.chunk, c.batched.size() - c0);
        if ((st = issue_chunk(c, c0, J)) != ARX_OK) return st;
    }
    if (wait && (st = c.render_single(c, c.n - 1)) != ARX_OK) return st;
    // 5. the one synchronisation, then the host-side outputs
    ARX_HIP(hipStreamSynchronize(c.r->stream));
    if (off_grid(c)) return fail(ARX_ERR_INTERNAL, "receiver refit / re-quantization: a box left the quantization grid");
    c.write_outputs(c);
    return ARX_OK;
}

// ---- arx_render_listeners' own steps ----

struct PlainCall : ListenerCall {
    arx_listener_result* results;
};

// The one-listener route: the loop's own step, then its outputs queued on the stream.
arx_status render_single(ListenerCall& c, size_t j) {
    arx_renderer* r = c.r;
    const arx_listener_pose& p = c.poses[j];
    arx_status s1 = arx_set_listener(r, p.x, p.y, p.z, p.yaw_deg);
    if (s1 == ARX_OK) s1 = arx_render(r, nullptr);
    if (s1 == ARX_OK && c.acoustics && !r->cur().acou.queued) s1 = arx_analyze_ir(r);
    if (s1 != ARX_OK) return s1;
    const arx_renderer::FrameSet& f = r->cur();
    const size_t ir_len = c.ir_len;
    c.where[j] = c.n + j;
    if (c.ir_left) {
        ARX_HIP(hipMemcpyAsync(c.ir_left + j * ir_len, f.d_ir.p, ir_len * sizeof(float), hipMemcpyDefault, r->stream));
        ARX_HIP(hipMemcpyAsync(c.ir_right + j * ir_len, f.d_ir.p + ir_len, ir_len * sizeof(float), hipMemcpyDefault,
                               r->stream));
    }
    unsigned long long* hc = c.h_counters + c.where[j] * batch_counter_words(0);
    hc[kCounters] = 0;
    ARX_HIP(hipMemcpyAsync(hc, f.d_counters.p, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->stream));
    if (c.acoustics)
        ARX_HIP(hipMemcpyAsync(c.h_res + 3 * c.where[j], f.acou.d_res.p, 3 * sizeof(arx_acoustics), hipMemcpyDeviceToHost,
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
        if (can_batch(c)) break;
        if ((st = render_single(c, c.first)) != ARX_OK) return st;
    }
    return ARX_OK;
}

arx_status replay(ListenerCall& c, const ListenerEntry* d_table, size_t, int32_t J) {
    ARX_HIP(launch_listeners_replay(c.probe.args, filter_args(c.probe, c.fgrow), d_table, J, c.r->stream));
    return ARX_OK;
}

void write_outputs(const ListenerCall& lc) {
    const PlainCall& c = static_cast<const PlainCall&>(lc);
    static_assert(kCounters == kBandCounterWords, "the plain batch's one cell is a frame's counters");
    for (size_t j = 0; j < c.n; ++j) {
        const unsigned long long* hc = c.h_counters + c.where[j] * batch_counter_words(0);
        if (c.results) {
            arx_listener_result& o = c.results[j];
            std::memset(&o, 0, sizeof(o));
            o.queries = hc[0];
            o.receiver_hits = hc[1];
            o.misses = hc[2];
            o.candidate_rays = c.route[j] == ARX_LISTENER_BATCHED ? hc[kCounters] : 0;
            o.route = c.route[j];
        }
        if (c.acoustics) std::memcpy(c.acoustics + 3 * j, c.h_res + 3 * c.where[j], 3 * sizeof(arx_acoustics));
    }
}

}  // namespace

ListenerLayout arx::ListenerSlots::layout(int32_t slot) const {
    return listener_layout(own_nodes, own_tris, recv_nodes, recv_tris, chunk, slot, trace_node_cache());
}

arx_status arx::check_batch_args(const arx_renderer* r, const arx_listener_pose* poses, size_t n, const float* ir_left,
                                 const float* ir_right, const double* filters, int32_t taps, const float* bb_left,
                                 const float* bb_right) {
    if (!r) return fail(ARX_ERR_INVALID_ARGUMENT, "renderer is NULL");
    if (n == 0) return ARX_OK;
    if (!poses) return fail(ARX_ERR_INVALID_ARGUMENT, "poses is NULL");
    if ((ir_left == nullptr) != (ir_right == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "ir_left and ir_right: both or neither");
    if ((bb_left == nullptr) != (bb_right == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "bb_left and bb_right: both or neither");
    if ((filters == nullptr) != (bb_left == nullptr))
        return fail(ARX_ERR_INVALID_ARGUMENT, "filters and bb_left / bb_right: all or none");
    if (filters && arx_debug_combine_bytes(1, 1, taps) == 0)
        return fail(ARX_ERR_INVALID_ARGUMENT, "taps %d: odd, 1..%d", taps, ARX_BAND_TAPS_MAX);
    for (size_t j = 0; j < n; ++j)
        if (!std::isfinite(poses[j].x) || !std::isfinite(poses[j].y) || !std::isfinite(poses[j].z) ||
            !std::isfinite(poses[j].yaw_deg))
            return fail(ARX_ERR_INVALID_ARGUMENT, "pose %zu is not finite", j);
    if (r->fif != 1) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs one frame in flight");
    if (r->stream != r->cur().stream) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own stream");
    if (r->d_hist_ext) return fail(ARX_ERR_INVALID_ARGUMENT, "a batch of listeners needs the renderer's own histogram");
    if (!r->scene_img) return fail(ARX_ERR_NOT_READY, "arx_set_scene has not been called");
    return ARX_OK;
}

arx_status arx::run_listener_call(ListenerCall& c, bool timed, double* ms) {
    arx_renderer* r = c.r;
    ListenerScratch& lb = *c.own;
    arx_status st;
    ARX_HIP(hipSetDevice(r->cfg.device));
    const BatchPinned pin = batch_pinned(c.n, c.bands);
    // nothing of an earlier call is in flight: every call ends synchronised
    if ((st = lb.h_pinned.reserve(pin.total)) != ARX_OK) return st;
    char* const h = lb.h_pinned.p;
    c.h_entries = reinterpret_cast<ListenerEntry*>(h + pin.entries);
    c.h_counters = reinterpret_cast<unsigned long long*>(h + pin.counters);
    c.h_res = reinterpret_cast<arx_acoustics*>(h + pin.res);
    c.h_flag = reinterpret_cast<unsigned int*>(h + pin.flag);
    c.h_flag[0] = c.h_flag[1] = 0u;
    c.ir_len = (size_t)r->ir_len;
    c.route.assign(c.n, ARX_LISTENER_SINGLE);
    c.where.assign(c.n, 0);
    if (timed && (st = lb.timer.begin(r->stream)) != ARX_OK) return st;
    const float saved[4] = {r->center[0], r->center[1], r->center[2], r->yaw};
    st = run_batch(c);
    arx_set_listener(r, saved[0], saved[1], saved[2], saved[3]);  // the listener set before the call, refit by the next frame
    if (st != ARX_OK || !timed) return st;
    if ((st = lb.timer.end(r->stream)) != ARX_OK) return st;
    return lb.timer.elapsed(ms);
}

extern "C" {

arx_status arx_render_listeners(arx_renderer* r, const arx_listener_pose* poses, size_t n, float* ir_left, float* ir_right,
                                arx_acoustics* acoustics, arx_listener_result* results, double* ms) {
    if (const arx_status st = check_batch_args(r, poses, n, ir_left, ir_right, nullptr, 0, nullptr, nullptr); st != ARX_OK || n == 0)
        return st;
    PlainCall c{{r, &r->listeners, poses, n, ir_left, ir_right, acoustics, 0, true, true, warm_up, render_single, nullptr, replay,
                 nullptr, write_outputs},
                results};
    c.N = n_rays(r->cfg);
    return run_listener_call(c, r->timing || ms != nullptr, ms);
}

arx_status arx_debug_set_listener_chunk(arx_renderer* r, int32_t listeners) {
    if (!r || listeners < 0 || listeners > kListenerChunkMax)
        return fail(ARX_ERR_INVALID_ARGUMENT, "listener chunk: 0 (automatic) or 1..%d", kListenerChunkMax);
    r->listeners.forced_chunk = listeners;
    return ARX_OK;
}

uint64_t arx_debug_listener_bytes(uint64_t n_rays, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t listeners) {
    if (ir_len < 0 || recv_nodes < 0 || recv_tris < 0 || listeners < 0) return 0;
    return (uint64_t)listeners * batch_bytes_each(n_rays, ir_len, recv_nodes, recv_tris, 0);
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
