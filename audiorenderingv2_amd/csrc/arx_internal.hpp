// arx_internal.hpp -- libarx.so internals shared by the C ABI translation units
// (arx_capi.cpp: one renderer's lifecycle, frame sets, timing rings and getters; arx_scene.cpp: the
// host-only scene image; arx_capi_device_scene.cpp: the tree on the device; arx_capi_trace.cpp: a frame --
// trace, finalize, analysis; arx_capi_path_cache.cpp: the path cache's buffers and launches;
// arx_capi_listeners.cpp: a batch of listeners and the driver of both batches; arx_capi_bands.cpp: frequency
// bands; arx_capi_listener_bands.cpp: the bands of a batch of listeners; arx_capi_directivity.cpp: the
// source's pattern, its orientation and the gain plane; arx_capi_air.cpp: air absorption's coefficients
// and attenuation table; arx_capi_conv.cpp: the
// file, live, streaming and walk-through convolution; arx_group.cpp: ray-sharded multi-GPU groups).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/arx.h"
#include "arx_bands.hpp"
#include "arx_batch_plan.hpp"
#include "arx_bvh.hpp"
#include "arx_kernels.hpp"
#include "arx_layout.hpp"
#include "arx_path_plan.hpp"
#include "arx_wide.hpp"

namespace arx {

// Records the message for arx_last_error() (thread-local) and returns s.
arx_status fail(arx_status s, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define ARX_HIP(call)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return ::arx::fail(e_ == hipErrorOutOfMemory ? ARX_ERR_OUT_OF_MEMORY : ARX_ERR_HIP,             \
                               "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);   \
    } while (0)

}  // namespace arx
#include "arx_device_mem.hpp"
namespace arx {

// device counters (per frame set, cleared by each frame): [0] queries [1] receiver hits [2] misses
// [3] error flag [4..7] counting builds (node steps, triangle tests, leader-node steps, step slots); the trace launch's ray-pool cursor lives after
// them (kCursor, reset by each launch itself).  The tree's off-grid flag is NOT among them: it is
// written by the tree updates that run before a frame's clear (arx_renderer::d_tree_flag).
constexpr int kCounters = 8;
constexpr int kCursor = 8;
// receivers up to this many triangles (and whose refit fits one workgroup's LDS: 9 floats per
// triangle, 11 words per node) are moved by the device refit; larger ones are rebuilt on the host
// per move
constexpr int64_t kRefitMaxTris = 3000;

inline uint64_t n_rays(const arx_config& c) {
    return (uint64_t)(int64_t)c.rays_x * (uint64_t)(int64_t)c.rays_y * (uint64_t)(int64_t)c.rays_z;
}

// The static scene as the host builds it once (buildAccel, AudioRenderer.cpp:95-218): the SBVH
// relocated into the device layout (scene nodes from index 1, node 0 being the top node; scene
// triangle records from 0) and its coded copy (code_nodes).  Immutable once built, shared by every
// renderer of a group (each uploads it to its own device).
struct SceneImage {
    BvhBuild bvh;
    std::vector<BvhNode> coded;
    int64_t n_input = 0;  // triangles given to arx_set_scene (global ids 0 .. n_input-1)
    uint64_t hash = 0;    // content hash of nodes and triangle records (profile guards)
    // The opt-in 4-wide compressed copy (CW4, arx_debug_set_trace_path bit 3; measured 1.9x slower
    // than the BVH2): made on first request only, never by the product path.
    struct Wide {
        W4Build w4;                    // scene root at unit 2, blocks from unit kW4SceneUnit
        std::vector<uint32_t> wimage;  // CW4 buffer units [0, w4.unit_end) x 4 words: leaf triangles
                                       // filled, node slots zero (quantized on the device)
    };
    const Wide& wide() const;
  private:
    mutable std::once_flag wide_once_;
    mutable Wide wide_;
};
// CW4 buffer: top node at unit 0, its block (scene root node, receiver root node) at units 2..5
constexpr uint32_t kW4SceneRoot = 2, kW4RecvRoot = 4, kW4SceneUnit = 6;
using SceneRef = std::shared_ptr<const SceneImage>;

// Input checks of arx_set_scene (finite vertices, absorption in [0, 1] or the receiver marks).
arx_status check_scene_input(const float* tri_v, const float* tri_abs, int64_t n);
// The trace kernel's 31-bit buffer offsets: a tree of n_nodes coded nodes and n_tris triangle records
// must fit them (ARX_ERR_INVALID_ARGUMENT otherwise).
arx_status check_buffer_offsets(size_t n_nodes, size_t n_tris);
// One host build (counted by arx_scene_build_count).
SceneRef build_scene_image(const float* tri_v, const float* tri_abs, int64_t n);
// Byte image of a build for the rank path's RCCL broadcast, and its inverse (NULL + why on a
// malformed image).
std::vector<uint8_t> serialize_scene(const SceneImage& s);
SceneRef deserialize_scene(const uint8_t* p, size_t n, const char** why);

}  // namespace arx

#ifndef ARX_RAY_ORDER_DEFAULT
#define ARX_RAY_ORDER_DEFAULT 1  // design experiments only (build.py --exp): arx_debug_set_ray_order's default
#endif
struct arx_renderer;
struct arx_stream;
namespace arx {
// The path cache (arx_debug_set_path_cache, include/arx.h): the scene-only closest hit of every query
// of every ray of one key, recorded by the second consecutive launch of that key and replayed against
// the receiver by the launches after it (plan_path_cache, arx_path_plan.hpp; issue_path_replay,
// arx_capi_path_cache.cpp).  The key is an OrderKey (arx_path_plan.hpp) without dyn_share and instance,
// valid for every 16-bit LDS-stack launch: the cache carries its own copy of the direction buffer it was
// recorded on, so neither the pool's share nor a frame set's own scatter order matters to it.  One per
// renderer, shared by its frame sets.
#ifndef ARX_PATH_CACHE_DEFAULT
#define ARX_PATH_CACHE_DEFAULT 1  // build.py --exp with 0: the cache-off library (A/B partner)
#endif
#ifndef ARX_PATH_FILTER_DEFAULT
#define ARX_PATH_FILTER_DEFAULT 1  // build.py --exp with 0: every replay unfiltered (A/B partner)
#endif
constexpr int kPathFrames = 3;    // arx_renderer::kMaxFrames
struct PathCache {
    int32_t mode = ARX_PATH_CACHE_DEFAULT;
    uint64_t max_bytes = 1ull << 30;
    int32_t state = ARX_PATH_CACHE_DEFAULT ? kPathTraced : kPathOff;  // of the last launch
    OrderKey key{};        // of the records (recorded) ...
    bool recorded = false;
    OrderKey last_key{};   // ... and of the previous launch (last_valid), whatever ran for it
    bool last_valid = false;
    DeviceBuf<float4> d_dirs;     // the direction buffer the records index, one per ray
    DeviceBuf<char> d_hits;       // [bounce][slot] 16-B records, then [bounce][slot] 8-B records
    uint64_t bytes = 0;           // of the records in use (recorded)
    uint64_t rec_rays = 0;        // rays of the records in use
    uint64_t rec_gen = 0;         // recordings made so far: what was derived from d_dirs is stale once it moves
    uint64_t no_room = 0;         // > 0: records of this size did not fit on the device (treated as over the cap)
    DeviceBuf<unsigned long long> d_scratch;  // the recording's counters and pool cursor (kCursor + 1 words)
    PinnedBuf<unsigned long long> h_scratch;  // kCounters words
    hipStream_t rec_stream = nullptr;         // the stream of the recording
    // frames in flight: a replay on another set's stream waits for `recorded`; a new recording waits
    // for every set's last replay
    hipEvent_t ev_recorded = nullptr, ev_replayed[kPathFrames] = {};
    bool replayed[kPathFrames] = {};
    // The path filter (arx_debug_set_path_filter, include/arx.h): the planes of what every recorded query
    // started from (path_filter_plane_bytes, arx_layout.hpp), outside the cap.  has_state: the records in
    // use came with them.  The candidate lists belong to the frame sets (FrameSet::d_filter_list).
    int32_t filter_on = ARX_PATH_FILTER_DEFAULT;
    DeviceBuf<char> d_filter;
    uint64_t filter_no_room = 0;      // > 0: planes of this size did not fit on the device: not tried again ...
    uint64_t filter_list_no_room = 0; // ... and a frame set's list of this size, a mark of its own (a list is far smaller)
    bool has_state = false;
    bool last_filtered = false;       // the last launch replayed filtered ...
    int32_t filter_slot = 0;          // ... on this frame set ...
    uint64_t filter_rays = 0;         // ... over this many rays
    // mode, max_bytes, filter_on and rec_gen stay (rec_gen never runs backwards: a plane made from freed
    // directions stays stale)
    void release() {
        d_dirs.release();
        d_hits.release();
        d_filter.release();
        d_scratch.release();
        h_scratch.release();
        if (ev_recorded) (void)hipEventDestroy(ev_recorded);
        ev_recorded = nullptr;
        for (hipEvent_t& e : ev_replayed) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        for (bool& b : replayed) b = false;
        recorded = last_valid = has_state = last_filtered = false;
        bytes = rec_rays = no_room = filter_no_room = filter_list_no_room = 0;
        state = mode == 1 ? kPathTraced : kPathOff;
    }
};
// The cache's buffers for a recording of n rays and `need` bytes of records: made at the first recording
// and kept across keys; a buffer that must grow is freed once every frame set's stream is idle (a replay
// of the key before may still read it).  *fits false: the device has no room for them (the cache is
// optional: the caller traces the launch instead); what was freed stays freed.
arx_status path_cache_reserve(arx_renderer* r, uint64_t n, uint64_t need, bool* fits);
// The current frame set's candidate list for n rays; false: no room on the device (the error cleared;
// that size is not tried again), and the frame replays unfiltered.
bool path_filter_list_reserve(arx_renderer* r, uint64_t n);
// The filter's margin (filter_kernel): kFilterMargin plus the slab test's own slack, 2^-18 of the
// largest coordinate magnitude the grid spans (scene, emitter and receiver lie on it).
float path_filter_grow(const QGrid& g);
// A launch the cache serves, on the current stream: with `record` the recording first, then the replay
// of n_launch rays with the launch's arguments a -- filtered where the filter's state allows it -- and
// PathCache::state set to what ran.
arx_status issue_path_replay(arx_renderer* r, const TraceArgs& a, bool record, uint64_t n_launch, int grid_cus);

// The device time of one call: an event pair made at first use.  begin and end record on s; elapsed waits
// for the end event.  Each call keeps its own rule for when it is timed and where its end lies.
struct CallTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    arx_status begin(hipStream_t s) {
        if (!ev0) ARX_HIP(hipEventCreate(&ev0));
        if (!ev1) ARX_HIP(hipEventCreate(&ev1));
        ARX_HIP(hipEventRecord(ev0, s));
        return ARX_OK;
    }
    arx_status end(hipStream_t s) {
        ARX_HIP(hipEventRecord(ev1, s));
        return ARX_OK;
    }
    arx_status elapsed(double* ms) {
        float t = 0.0f;
        ARX_HIP(hipEventSynchronize(ev1));
        ARX_HIP(hipEventElapsedTime(&t, ev0, ev1));
        if (ms) *ms = (double)t;
        return ARX_OK;
    }
    void destroy() {
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    }
};

// What a batch of listeners owns (arx_render_listeners: arx_renderer::listeners; arx_render_listener_bands:
// arx_renderer::listener_bands; include/arx.h): the scratch of one chunk (batch_scratch, arx_batch_plan.hpp)
// in one allocation made by the first batched call, reused while it is large enough, freed when it must grow
// and at arx_destroy, outside the path cache's cap; and the call's pinned block (batch_pinned).  The chunk's
// receiver slots live in the renderer's node and triangle arrays (listener_layout, arx_layout.hpp), which the
// first batched call widens.
struct ListenerScratch {
    int32_t forced_chunk = 0;     // arx_debug_set_listener_chunk: 0 automatic (`listeners` holds it for both calls)
    DeviceBuf<char> d_scratch;
    uint64_t no_room = 0;         // > 0: a scratch of this size did not fit on the device: not tried again
    PinnedBuf<char> h_pinned;     // per listener of a call: its table entry, counter words and results
    DeviceBuf<double> d_filters;  // the band call's filter bank (n_bands x taps)
    CallTimer timer;
    void release() {              // forced_chunk stays
        d_scratch.release();
        h_pinned.release();
        d_filters.release();
        timer.destroy();
        no_room = 0;
    }
};
// What a chunk of receiver slots is laid out from: the receiver's and the renderer's own tree sizes, and the chunk.
struct ListenerSlots {
    int64_t recv_nodes = 0, recv_tris = 0, own_nodes = 0, own_tris = 0;
    int32_t chunk = 0;
    ListenerLayout layout(int32_t slot) const;
};
// What a replayed frame of the current key would launch, as trace_rays decides it (probe below).
struct ReplayProbe {
    bool ready = false;     // the key is recorded with its filter state, and this launch would only replay
    bool recorded = false;  // the key is recorded (with or without filter state), and this launch would only replay
    int32_t state = 0;      // what the launch would leave in PathCache::state had it run traced (kPath*)
    TraceArgs args;         // the replay's arguments (dirs and rec the cache's)
    const void* planes = nullptr;
};
// A batched replay's filter arguments: the list and the heads come per listener, from the table.
inline FilterArgs filter_args(const ReplayProbe& probe, float fgrow) {
    FilterArgs fa;
    fa.planes = probe.planes;
    fa.list = nullptr;
    fa.heads = nullptr;
    fa.grow = fgrow;
    return fa;
}
// One call of either batch, for run_listener_call (arx_capi_listeners.cpp): its arguments, what its steps hand
// each other, and the steps that are the call's own.  bands 0 is arx_render_listeners: its batched listeners
// are frames of the renderer (`frames`: each counts in ir_generation, the call's last pose is adopted as the
// renderer's last frame, so that pose's one-listener route waits for the chunks).
struct ListenerCall {
    arx_renderer* r;
    ListenerScratch* own;
    const arx_listener_pose* poses;
    size_t n;
    float* ir_left;               // [pose][cell][ir_len], or null
    float* ir_right;
    arx_acoustics* acoustics;     // [pose][cell][3], or null
    int32_t bands;
    bool frames, want_ir;
    // 1. until the key is recorded (with its filter state, where the batch is to run): c.probe, c.first, c.warm
    arx_status (*warm_up)(ListenerCall& c);
    // a pose the batch cannot take, through the one-listener calls; sets c.route[j]
    arx_status (*render_single)(ListenerCall& c, size_t j);
    // once, in front of the first chunk, when a pose is batched; may be null
    arx_status (*begin_chunks)(ListenerCall& c);
    // the chunk's replay launch for the batched poses [c0, c0 + J), refit into d_table's slots
    arx_status (*replay)(ListenerCall& c, const ListenerEntry* d_table, size_t c0, int32_t J);
    // after the cells of chunk slot i (pose j) are finalized; may be null
    arx_status (*finish_listener)(ListenerCall& c, int32_t i, size_t j);
    // the host-side outputs, after the call's one synchronisation
    void (*write_outputs)(const ListenerCall& c);
    uint64_t N = 0;               // rays of a frame
    size_t ir_len = 0;
    size_t first = 0;             // poses before it went through the warm-up
    int32_t warm = 0;             // ordinary launches the recording took
    std::vector<int32_t> route;   // per pose: ARX_LISTENER_SINGLE or ARX_LISTENER_BATCHED
    std::vector<size_t> where;    // per pose: its row in the pinned counters / results
    std::vector<size_t> batched;  // the batched poses, in batched order
    ListenerEntry* h_entries = nullptr;         // the pinned block (batch_pinned)
    unsigned long long* h_counters = nullptr;
    arx_acoustics* h_res = nullptr;
    unsigned int* h_flag = nullptr;
    ReplayProbe probe;
    ListenerSlots sl;             // the receiver slots behind the renderer's own tree; sl.chunk == chunk
    int32_t chunk = 0;            // listeners per chunk
    BatchScratch sc{};
    char* d_base = nullptr;       // the chunk scratch
    float fgrow = 0.0f;           // the filter's margin on the grid the batch runs on
    template <class T>
    T* at(uint64_t offset) const { return reinterpret_cast<T*>(d_base + offset); }
};
// arx_render_listeners' and arx_render_listener_bands' common argument checks, in the order the ABI reports
// them (the plain call passes no filters); ARX_OK for n == 0, which the caller returns as it is.
arx_status check_batch_args(const arx_renderer* r, const arx_listener_pose* poses, size_t n, const float* ir_left,
                            const float* ir_right, const double* filters, int32_t taps, const float* bb_left,
                            const float* bb_right);
// The call: its pinned block, the driver (warm-up, prepare, select, the one-listener poses, the chunks, the one
// synchronisation, the off-grid check, the outputs) between the listener saved and restored, and its time.
arx_status run_listener_call(ListenerCall& c, bool timed, double* ms);
// The walk-through convolution (arx_convolute_walk, include/arx.h): one scratch allocation per renderer
// (walk_layout, arx_kernels.hpp), made by the first call, kept across calls and freed when it must grow and
// at arx_destroy; outside the path cache's cap.
struct WalkScratch {
    int32_t forced_tile = 0;      // arx_debug_set_walk_tile: 0 the product's tile
    DeviceBuf<char> d_scratch;
    int32_t tw_n = 0;             // the scratch holds the twiddles of this FFT size (0: none)
    std::vector<double> h_tw;     // their host copy (2 doubles each)
    std::vector<int32_t> h_tables, h_slot;  // a call's item tables and IR slots, reused
    std::vector<double> h_w;      // and its fade weights
    CallTimer timer;              // the call's device time
    uint64_t state[5] = {};       // arx_debug_walk_state
    void release() {              // forced_tile stays
        d_scratch.release();
        timer.destroy();
        tw_n = 0;
    }
};
constexpr int32_t kWalkTile = 8;      // items per MAC workgroup
constexpr int32_t kWalkTileMax = 64;  // arx_debug_set_walk_tile
// Frequency-band absorption (arx_set_band_absorption / arx_render_bands, include/arx.h): the device table
// ([triangle][band_width] f32, by global triangle id) and the call's scratch (band_scratch_layout,
// arx_bands.hpp) -- one allocation each, kept across calls, freed when they must grow and at arx_destroy;
// outside the path cache's cap.  arx_set_scene drops the table (n_bands 0) and keeps the memory.
struct BandState {
    int32_t n_bands = 0;          // 0: no table
    int64_t n_tris = 0;           // the table's rows
    DeviceBuf<float> d_table;
    DeviceBuf<char> d_scratch;
    PinnedBuf<char> h_pinned;     // kMaxBands counter blocks, then kMaxBands x 3 arx_acoustics
    CallTimer timer;              // the call's device time
    int32_t hist_bands = 0;       // the scratch holds the raw histograms of this many bands (the last call's) ...
    int32_t hist_ir_len = 0;      // ... of this length (arx_debug_band_histograms)
    void release() {
        d_table.release();
        d_scratch.release();
        h_pinned.release();
        timer.destroy();
        n_bands = hist_bands = 0;
    }
};
// Source directivity (arx_set_source_directivity / arx_set_source_orientation, include/arx.h): the pattern's
// cube map on the device, the orientation, and the gain plane the directed band replays read
// (arx_directivity.hpp) -- one allocation each, kept across calls, freed when they must grow and at
// arx_destroy; outside the path cache's cap.  The plane is remade only when a generation word it was made
// from has moved: the pattern's, the orientation's, the band count or the recording's (PathCache::rec_gen).
// The pattern survives arx_set_scene and arx_set_band_absorption.
struct DirectivityState {
    int32_t n_bands = 0;          // 0: no pattern (the band replays run undirected); 1 serves every band
    int32_t res = 0;
    float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    DeviceBuf<float> d_cube;
    DeviceBuf<float> d_plane;
    uint64_t pattern_gen = 0, orient_gen = 0;
    bool plane_valid = false;     // d_plane holds the plane of made_*
    uint64_t made_pattern = 0, made_orient = 0, made_rec = 0, made_rays = 0;
    int32_t made_bands = 0;
    uint64_t planes_made = 0;     // gain kernel launches so far
    void release() {
        d_cube.release();
        d_plane.release();
        n_bands = 0;
        plane_valid = false;
    }
};
// The rule of a band call with a pattern installed: a pattern of more than one band matches the table's bands.
arx_status directivity_check_bands(const arx_renderer* r, int32_t n_bands);
// The gain plane for a band call of n_bands bands over the recording whose direction copy is `dirs` (n rays),
// on the renderer's stream: *plane null without a pattern; else the plane, made now if what it was made from
// has changed.  Nothing of an earlier band call is in flight: each ends synchronised.
arx_status directivity_plane(arx_renderer* r, const void* dirs, uint64_t n, int32_t n_bands, const float** plane);
// Air absorption (arx_set_air_absorption, include/arx.h): the coefficients, and the attenuation table
// [bin][band_width] the band replays' AIR instantiations read at a deposit -- one allocation, kept across
// calls, freed when it must grow and at arx_destroy; outside the path cache's cap.  The table is made on the
// host and uploaded by the first band call that needs it, and remade only when the coefficients' generation
// or the call's band count has moved.  The coefficients survive arx_set_scene and arx_set_band_absorption.
struct AirState {
    int32_t n = 0;                // 0: none (the band replays run without the factor); 1 serves every band
    double alpha[kMaxBands] = {}; // dB per metre
    DeviceBuf<float> d_table;
    uint64_t gen = 0;             // changes of the coefficients so far
    bool table_valid = false;     // d_table holds the table of made_*
    uint64_t made_gen = 0;
    int32_t made_bands = 0;
    uint64_t tables_made = 0;     // uploads so far
    void release() {
        d_table.release();
        n = 0;
        table_valid = false;
    }
};
// The rule of a band call with coefficients installed: more than one coefficient matches the table's bands.
arx_status air_check_bands(const arx_renderer* r, int32_t n_bands);
// The attenuation table for a band call of n_bands bands: *table null without coefficients; else the device
// table, made now (a host loop and one blocking upload) if what it was made from has changed.  Nothing of an
// earlier band call is in flight: each ends synchronised.
arx_status air_table(arx_renderer* r, int32_t n_bands, const float** table);
// Band synthesis (arx_combine_bands, include/arx.h): one scratch allocation per renderer (the call's inputs,
// filters and outputs), made by the first call, kept across calls and freed when it must grow and at
// arx_destroy; outside the path cache's cap.
struct SynthScratch {
    DeviceBuf<char> d_scratch;
    CallTimer timer;              // the call's device time
    void release() {
        d_scratch.release();
        timer.destroy();
    }
};
// A band call's recording (arx_render_bands, arx_render_listener_bands): ordinary launches -- the first at
// *pose, when one is given -- until the cache holds the key's records (*probe says so); *warm counts them.
arx_status record_for_bands(arx_renderer* r, uint64_t N, const arx_listener_pose* pose, ReplayProbe* probe, int32_t* warm);
// One cell -- one histogram -- finalized into its f32 IR pair (want_ir) and analysed into d_res[0..3) (analyse).
arx_status finalize_and_analyse(arx_renderer* r, const unsigned long long* hist, float* irl, float* irr, arx_acoustics* d_res,
                                void* edc, void* acou, bool want_ir, bool analyse);
// Energy of a ray at the emitter (devicePrograms.cu:208).
float initial_energy(const arx_config& c);

// A ring of (start, end) event pairs around the last kTraceRing timed launches of one kind.  A launch
// that is not timed records nothing and does not advance the ring.
constexpr int kTraceRing = 256;
struct EventRing {
    hipEvent_t e0[kTraceRing] = {}, e1[kTraceRing] = {};
    uint64_t launches = 0;  // timed launches (the ring's index)
    arx_status create_all();  // every slot's events now (begin makes a slot's on first use otherwise)
    void destroy();
    arx_status begin(hipStream_t s);  // the start event of the next launch
    arx_status end(hipStream_t s);    // its end event; counts the launch
    // Device time (ms) of the last launch; wait = synchronise on it first.
    arx_status last_ms(bool wait, double* ms) const;
    // Device times of the last min(n, ring) launches, oldest first.
    arx_status times(double* ms, size_t n, size_t* n_out) const;
};

// arx_trace_rays with the per-launch events recorded or not (arx_set_timing, or a caller asking for the
// time); clear: the direction pre-pass zeroes the histogram and counters first (render() after
// begin_frame, instead of arx_clear_histogram's launch)
// probe: nothing is launched; the scene is brought up to date, the path cache's decision for this launch
// is made as usual (plan_path_cache) and *probe says whether it is "replay, with filter state".  Of the
// cache's history a probe writes one thing: records of another key are dropped, as a launch would drop them.
arx_status trace_rays(arx_renderer* r, uint64_t ray_begin, uint64_t ray_end, bool timed, bool clear = false,
                      ReplayProbe* probe = nullptr);
// Seconds-free scale of the fixed-point histogram: one unit of it in energy (finalize, analysis).
double ir_unit(const arx_config& c);
// The analysis of one histogram (3 decay curves into edc, 3 results into out) with the renderer's settings.
AcousticsArgs acoustics_args(const arx_renderer* r, const long long* hist, long long* edc, arx_acoustics* out, void* scratch);
// The tree on the device brought up to date with the scene, the receiver model and the listener's pose
// (arx_capi_device_scene.cpp): buffers, grid, uploads, re-quantization, the receiver's refit.
arx_status ensure_device_scene(arx_renderer* r);
// Rotation of a receiver at yaw_deg, row-major, exactly arx_place_receiver_vertices' floats.
void receiver_rotation(float yaw_deg, float m[9]);
// Box padding the refit kernel takes for a receiver at `centre` (arx_debug_set_refit_pad's when set).
float refit_pad(const arx_renderer* r, const float centre[3]);
// World-space bound of the receiver placed at `centre` (for the quantization grid): the refit path's ball
// widened by the refit kernel's box padding (the padded boxes it quantizes must stay on the grid), or the
// host-built sub-tree's root box (wherever `centre` is).
void receiver_bound(const arx_renderer* r, const float centre[3], float lo[3], float hi[3], bool* empty);
// Whether the emitter lies in that bound widened by `grow`: every ray would be a filter candidate at bounce 0.
bool emitter_in_receiver_box(const arx_renderer* r, const float centre[3], float grow);
// The refit kernels' arguments that do not depend on a pose: the receiver's local model, where it goes in
// the tree's arrays, the grid and the quantized nodes, the off-grid flag of the current tree write.
RefitArgs refit_args(const arx_renderer* r);
// The grid grown once for a batch, as ensure_device_scene grows it for a walking listener: the new grid
// spans the old one, the scene, the emitter and [ulo, uhi] with half the extent as margin, the top node and
// the scene are re-quantized on the device, and the renderer's own receiver is refit for it by the next
// ensure_device_scene.
arx_status grow_grid_for(arx_renderer* r, const float ulo[3], const float uhi[3]);
// The node and triangle arrays widened to hold a batch's slots: new buffers, what the old ones held copied
// on the device.  False: no room (the error cleared; the arrays as they were).
bool widen_tree_arrays(arx_renderer* r, size_t need_nodes, size_t need_tris);
// arx_clear_histogram without its launch: with frames in flight, the next frame takes the next set
arx_status begin_frame(arx_renderer* r);
// Install a built scene (arx_set_scene's second half): uploaded at the next trace.
arx_status set_scene_image(arx_renderer* r, SceneRef img);
// Frames in flight (arx_set_frames_in_flight; no-ops with one): the current set's stream waits for
// every other set's last trace / for the set that did the last scene write, convolution or all-reduce;
// `done_*` record the current set's.
arx_status fif_wait_traced(arx_renderer* r);
arx_status fif_done_traced(arx_renderer* r);
arx_status fif_wait_scene(arx_renderer* r);
arx_status fif_done_scene(arx_renderer* r);
arx_status fif_wait_conv(arx_renderer* r);
arx_status fif_done_conv(arx_renderer* r);
arx_status fif_wait_reduced(arx_renderer* r);
arx_status fif_done_reduced(arx_renderer* r);
// Every frame set's stream synchronised.
arx_status sync_renderer(arx_renderer* r);
// arx_convolute_device restricted to the file's one-second block pairs [pair_begin, pair_end)
// (conv_run_pairs; the group's time-block shards); timed: recorded in the file-convolution ring.
arx_status convolute_pairs(arx_renderer* r, const float* d_in, size_t n_frames, float* d_out_left, float* d_out_right,
                           int64_t pair_begin, int64_t pair_end, bool timed);
// The renderer's staging for a file convolution of n frames (arx_convolute_audio_file, the group's): n floats
// in, 2 * n out; both replaced when either is too small.  The caller has waited for the last convolution.
arx_status reserve_conv_staging(arx_renderer* r, size_t n);
// Whether the renderer's file convolution plan convolves a shard on its own (conv_plan_shards).
bool conv_shards(arx_renderer* r);
// Detach a streaming convolution from its renderer and release its device side (arx_destroy).
void release_stream(arx_stream* s);
}  // namespace arx

// One renderer = one device (AudioRenderer, AudioRenderer.h:16-152).
struct arx_renderer {
    arx_config cfg;
    int32_t ir_len = 0;
    int cus = 256;
    hipStream_t stream = nullptr;  // the stream work is issued on now: the current set's, or arx_set_stream's
    // timing events around the trace launches (arx_trace_times), file convolutions (arx_conv_times),
    // live / streaming convolutions (arx_live_times) and analyses (arx_analysis_times; made at first use)
    arx::EventRing trace_ring, conv_ring, live_ring, analysis_ring;
    bool timing = true;  // arx_set_timing: record the per-launch events

    float emitter[3] = {0.f, 0.f, 0.f};
    float center[3] = {0.f, 0.f, 0.f};
    float yaw = 0.f;

    // host scene (shared with the other members of a group)
    arx::SceneRef scene_img;
    std::vector<float> recv_local[2];
    arx::BvhBuild recv;
    bool scene_dirty = true;
    bool recv_model_dirty = true;  // receiver halves or scene changed: rebuild the local sub-tree
    bool recv_pose_dirty = true;   // listener moved: refit on the device
    bool scene_set = false;
    // receiver sub-tree in its local frame (refit path) and its device images
    bool recv_refit = true;
    float recv_radius = 0.0f;
    arx::DeviceBuf<arx::TriRec> d_recv_local;
    arx::DeviceBuf<arx::BvhNode> d_recv_nodes;
    arx::DeviceBuf<int32_t> d_recv_levels;  // level-ordered node indices, then level starts
    int32_t recv_levels = 0, recv_level_count = 0;

    // device
    arx::DeviceBuf<arx::BvhNode> d_cnodes;  // coded copy of the tree (code_nodes): the f32 fallback
    arx::DeviceBuf<arx::QNode2> d_qnodes;   // 16-bit quantized copy of d_cnodes (same indices and size): the default
    // CW4 copy: buffer, f32 node records (top node, scene, host-built receiver) for the device
    // re-quantization, the receiver's CW4 layout (refit path) and its device tables
    arx::DeviceBuf<uint4> d_wbuf;  // units
    arx::DeviceBuf<arx::W4NodeF> d_w4f;
    size_t n_w4f = 0;              // records in use
    arx::W4Build recv4;
    arx::DeviceBuf<int32_t> d_recv_w4;  // 11 ints per receiver CW4 node
    arx::DeviceBuf<int32_t> d_recv_w4_tris;
    bool use_w4 = false;           // arx_debug_set_trace_path bit 3: the CW4 tree
    int32_t depth4 = 0;            // CW4 levels (top node included): bounds the stack (3 per level)
    int32_t occ[3][3][3] = {};     // per node format and instance (kInstPool, kInstSmall, kInstMeasure): VGPRs, waves admitted, waves targeted
    int32_t ray_order = ARX_RAY_ORDER_DEFAULT;  // arx_debug_set_ray_order: 0 identity, directions kept; 1 longest-first pool; 2 directions re-made per launch
    uint64_t scene_gen = 0;        // scenes installed (set_scene_image): part of a frame set's OrderKey
    arx::PathCache path_cache;     // scene-only hits of the last repeated key (arx_debug_set_path_cache)
    arx::ListenerScratch listeners;  // arx_render_listeners' chunk scratch
    arx::WalkScratch walk;         // arx_convolute_walk's scratch
    arx::BandState bands;          // arx_render_bands' table and scratch
    arx::DirectivityState directivity;  // the source's pattern, orientation and gain plane
    arx::AirState air;             // air absorption's coefficients and attenuation table
    arx::SynthScratch synth;       // arx_combine_bands' scratch
    arx::ListenerScratch listener_bands;  // arx_render_listener_bands' scratch
    arx::QGrid qgrid{};
    bool qgrid_set = false;
    bool q_valid = false;         // d_qnodes matches the tree (re-quantized on the device, arx_receiver.hip)
    uint64_t requants = 0;        // device re-quantizations issued (new scene or grid)
    uint64_t nodes_cap() const { return std::min(d_cnodes.cap, d_qnodes.cap); }  // nodes both copies hold
    arx::DeviceBuf<arx::TriRec> d_tris;
    arx::DeviceBuf<int32_t> d_gstack;  // global traversal stack for trees deeper than the LDS stack
    bool force_global_stack = false;  // arx_debug_set_trace_path
    bool force_f32_nodes = false;
    unsigned long long* d_hist_ext = nullptr;  // caller-attached (arx_attach_histogram)
    unsigned long long* hist() const { return d_hist_ext ? d_hist_ext : cur().d_hist.p; }
    // The tree's off-grid flag (a receiver refit or re-quantization put a box outside the quantization
    // grid; its quantized copy then falls back to whole-axis boxes): one word per renderer, outside the
    // per-frame counters the direction pre-pass clears.  Each tree write (ensure_device_scene) runs with
    // a new generation tree_gen and raises the word to it (atomic max) on failure, so the flag reports
    // the tree as last written -- no clear launch, and a later clean write retires an old failure.
    arx::DeviceBuf<unsigned int> d_tree_flag;
    arx::PinnedBuf<unsigned int> h_tree_flag;
    uint32_t tree_gen = 0;
    float debug_refit_pad = 0.0f;  // arx_debug_set_refit_pad: the refit kernel's box padding (0 = automatic)

    uint64_t ir_generation = 0;  // bumped whenever the IR changes (finalize_ir, set_ir): streams re-transform
    arx::ConvPlan* conv_live = nullptr;  // mic path plan (block = live block length)
    bool conv_live_ir_dirty = true;
    arx::DeviceBuf<double> d_live_in;   // ir_len
    arx::DeviceBuf<double> d_live_out;  // 2 * ir_len

    arx::ConvPlan* conv = nullptr;
    bool conv_ir_dirty = true;
    arx::DeviceBuf<float> d_conv_in;   // the file convolution's staging: n frames in ...
    arx::DeviceBuf<float> d_conv_out;  // ... and 2 * n out (reserve_conv_staging)

    std::vector<arx_stream*> streams;  // live streaming convolutions of this renderer (arx_stream_create)

    // Frames in flight (arx_set_frames_in_flight, up to kMaxFrames): a frame's start
    // (arx_clear_histogram) takes the next of `sets` -- stream, histogram, IR, counters, direction
    // buffer and analysis -- so frame k + 1 traces on its own stream while frame k's trace finishes
    // and its IR is convolved.  The frames wait for each other only where they share state: writes to
    // the shared scene / receiver buffers (and traces on the one global stack) for every other set's
    // last trace (ev_traced); each trace for the last scene writes (ev_scene), each use of the shared
    // convolution plans and of the caller's output buffers for the last convolution (ev_conv), a
    // group's all-reduce for the last all-reduce on the same communicator (ev_reduced).  `slot` names
    // the current set (cur()); last_* the set that did the last such step (-1: none yet).
    static constexpr int kMaxFrames = 3;
    // A frame's room-acoustic analysis (arx_analyze_ir): decay curves (3*ir_len), results (3) and the
    // kernels' scratch, allocated by the frame set's first analysis; queued: the frame that now owns
    // the set was analysed (arx_get_acoustics).
    struct Acoustics {
        arx::DeviceBuf<long long> d_edc;
        arx::DeviceBuf<arx_acoustics> d_res;
        arx::DeviceBuf<char> d_scratch;
        bool queued = false;
        void release() {  // with the set, or after a failed first allocation
            d_edc.release();
            d_res.release();
            d_scratch.release();
            queued = false;
        }
    };
    bool auto_analyze = false;  // arx_set_auto_analyze
    int32_t scan_shape = 0;     // arx_debug_set_scan_shape (0: the product's)
    struct FrameSet {
        hipStream_t stream = nullptr;
        arx::DeviceBuf<unsigned long long> d_hist;      // 2*ir_len (own)
        arx::DeviceBuf<float> d_ir;                     // 2*ir_len: L then R
        arx::DeviceBuf<unsigned long long> d_counters;  // kCursor + 1 words
        arx::PinnedBuf<unsigned long long> h_counters;  // kCounters words
        arx::DeviceBuf<float4> d_dirs;                  // direction pre-pass (one per ray of the largest trace call)
        // What d_dirs holds, so a launch of the same seed and range skips the pre-pass's directions
        // (forgotten when the buffer is reallocated): the rays [dirs_begin, dirs_begin + dirs_count)
        // of dirs_seed, in ray order or (dirs_sorted) with the pool's slots ordered for order_key,
        // written on dirs_stream.
        bool dirs_valid = false, dirs_sorted = false;
        hipStream_t dirs_stream = nullptr;
        uint64_t dirs_seed = 0, dirs_begin = 0, dirs_count = 0;
        arx::OrderKey order_key{};
        // the longest-first pool (made by the set's first measuring launch): the buffer the sort
        // writes (swapped with d_dirs after it), per-slot costs, the sort's bins
        arx::DeviceBuf<float4> d_dirs_alt;
        arx::DeviceBuf<unsigned short> d_cost;
        arx::DeviceBuf<uint32_t> d_order_bins;          // order_bins_bytes()
        // the path filter's candidate list of this set's replays (two sets replay at once on two
        // streams): filter_list_rays entries, then the filter blocks' heads (path_filter_list_bytes)
        arx::DeviceBuf<char> d_filter_list;
        uint64_t filter_list_rays = 0;
        Acoustics acou;
        void release() {
            if (stream) (void)hipStreamDestroy(stream);
            stream = nullptr;
            d_hist.release();
            d_ir.release();
            d_counters.release();
            h_counters.release();
            d_dirs.release();
            d_dirs_alt.release();
            d_cost.release();
            d_order_bins.release();
            d_filter_list.release();
            acou.release();
            *this = FrameSet{};
        }
    };
    int32_t fif = 1;
    int32_t slot = 0;
    FrameSet sets[kMaxFrames];  // [0, fif) allocated
    FrameSet& cur() { return sets[slot]; }
    const FrameSet& cur() const { return sets[slot]; }
    hipEvent_t ev_traced[kMaxFrames] = {}, ev_conv[kMaxFrames] = {}, ev_reduced[kMaxFrames] = {},
               ev_scene[kMaxFrames] = {};
    int32_t last_conv = -1, last_reduced = -1, last_scene = -1;

    arx::DeviceBuf<unsigned long long> d_prof;  // per-wave records (profiling builds, ARX_TRACE_PROF)
    // The renderer's own buffers; its parts (the scratch structs above, the frame sets) have a release each.
    void release_buffers() {
        d_recv_local.release();
        d_recv_nodes.release();
        d_recv_levels.release();
        d_recv_w4.release();
        d_recv_w4_tris.release();
        d_cnodes.release();
        d_qnodes.release();
        d_tris.release();
        d_gstack.release();
        d_live_in.release();
        d_live_out.release();
        d_conv_in.release();
        d_conv_out.release();
        d_wbuf.release();
        d_w4f.release();
        d_prof.release();
        d_tree_flag.release();
        h_tree_flag.release();
    }
    int32_t last_format = 0;  // node format of the last trace launch (arx_stats::trace_format)
    arx_stats stats;
};
