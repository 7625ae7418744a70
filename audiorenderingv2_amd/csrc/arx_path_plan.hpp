// arx_path_plan.hpp -- what the path cache does with one launch, as arithmetic on keys and sizes.
//
// Host only and free of HIP, so that a host test can walk it through every case
// (tests/cpp/path_plan.cpp).  The state it reads and the buffers behind it live in PathCache
// (arx_internal.hpp); trace_rays (arx_capi_trace.cpp) calls it once per launch and commits the result,
// and once per probe and commits only a `recorded` that fell.
#pragma once
#include <cstdint>
#include <cstring>

namespace arx {

// Everything that changes a ray's path or length, so the per-ray costs one launch measured order the
// pool of the next: a frame set keeps its sorted direction buffer while this stays the same.  The
// listener's position and yaw are deliberately not in it (a few percent of the rays touch the receiver).
// Compared as bytes: a key is zeroed before its fields are set (make_order_key, arx_capi_trace.cpp).
struct OrderKey {
    uint64_t scene_gen, tree_hash, seed, ray_begin, ray_end;
    float emitter[3];
    float e0, energy_thres, hrtf, dist_limit;
    uint32_t max_bounces, dyn_share;
    int32_t is_mono, instance;
};
inline bool same_key(const OrderKey& a, const OrderKey& b) { return std::memcmp(&a, &b, sizeof(OrderKey)) == 0; }

constexpr int kPathOff = 0, kPathTraced = 1, kPathRecorded = 2, kPathReplayed = 3, kPathNotCacheable = 4,
              kPathOverCap = 5;  // arx_debug_path_cache_state

// The cache's side of the decision: what the launches before this one left (PathCache's fields of the
// same names).
struct PathHistory {
    bool recorded;      // `key` has records ...
    OrderKey key;
    bool last_valid;    // ... and `last_key` is the previous launch's key
    OrderKey last_key;
    uint64_t max_bytes;
    uint64_t no_room;   // > 0: records of this size did not fit on the device
};

struct PathPlan {
    int32_t state;      // PathCache::state as the launch leaves it when it is traced; a replay that was
                        // issued makes it kPathRecorded (record) or kPathReplayed
    bool replay;        // the launch replays the records ...
    bool record;        // ... after making them (then replay is set too)
    bool recorded;      // PathCache::recorded (until a recording that was issued sets it), last_valid and
    bool last_valid;    // last_key after the launch
    OrderKey last_key;
};

// mode: arx_debug_set_path_cache's; cacheable: the launch is one the cache can serve (trace_can_cache, on
// the frame set's own stream); key: the launch's, dyn_share and instance zeroed; final_dirs: the launch
// would neither fill nor measure its direction buffer; need: bytes of the launch's records.
// A launch whose key equals the previous launch's, on final directions, records and replays; the launches
// of that key after it only replay; a launch of another key drops the records.  Over the cap (or known
// not to fit) nothing is recorded or replayed.
inline PathPlan plan_path_cache(int32_t mode, bool cacheable, const OrderKey& key, bool final_dirs, uint64_t need,
                                const PathHistory& h) {
    PathPlan p{};
    p.last_key = h.last_key;
    if (mode != 1 || !cacheable) {
        p.state = mode != 1 ? kPathOff : kPathNotCacheable;
        return p;  // recorded and last_valid cleared
    }
    const bool repeated = h.last_valid && same_key(key, h.last_key);
    p.recorded = h.recorded && same_key(key, h.key);
    p.last_key = key;
    p.last_valid = true;
    p.state = kPathTraced;
    if (need > h.max_bytes || (h.no_room > 0 && need >= h.no_room)) {
        p.state = kPathOverCap;
        p.recorded = false;
    } else if (final_dirs && p.recorded) {
        p.replay = true;
    } else if (final_dirs && repeated) {
        p.record = p.replay = true;
    }
    return p;
}

}  // namespace arx
