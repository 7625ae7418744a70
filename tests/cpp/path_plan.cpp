// path_plan.cpp -- the path cache's decision (plan_path_cache, csrc/arx_path_plan.hpp) walked through a
// table of launches on the host.  One line per row: "<row> <state> <replay> <record> <recorded> <last_valid>",
// the plan's fields as the function returns them; tests/test_path_cache_host.py holds the expected lines.
//
//   g++ -std=c++17 -I audiorenderingv2_amd/csrc tests/cpp/path_plan.cpp -o path_plan && ./path_plan
#include <cstdio>
#include <cstring>

#include "arx_path_plan.hpp"

using namespace arx;

namespace {

const char* kStateName[] = {"Off", "Traced", "Recorded", "Replayed", "NotCacheable", "OverCap"};

OrderKey make_key(uint64_t seed) {
    OrderKey k;
    std::memset(&k, 0, sizeof(k));
    k.scene_gen = 3;
    k.tree_hash = 0x1234abcdull;
    k.seed = seed;
    k.ray_begin = 0;
    k.ray_end = 36000;
    k.emitter[0] = 0.5f; k.emitter[1] = 3.0f; k.emitter[2] = 1.0f;
    k.e0 = 1e-4f;
    k.energy_thres = 1e-7f;
    k.hrtf = 0.5f;
    k.dist_limit = 344.0f;
    k.max_bounces = 8;
    k.is_mono = 0;
    return k;  // dyn_share and instance stay 0, as the cache's key has them
}

// A cache as a renderer holds it: the history, and the two commits a launch makes -- the plan's fields, and
// behind a recording the key of the records.
struct Cache {
    PathHistory h;
    Cache() {
        std::memset(&h, 0, sizeof(h));
        h.max_bytes = 1ull << 30;
    }
    PathPlan launch(const char* row, const OrderKey& key, bool final_dirs = true, uint64_t need = 1000, int32_t mode = 1,
                    bool cacheable = true) {
        const PathPlan p = plan_path_cache(mode, cacheable, key, final_dirs, need, h);
        if (row)
            std::printf("%s %s %d %d %d %d\n", row, kStateName[p.state], (int)p.replay, (int)p.record, (int)p.recorded,
                        (int)p.last_valid);
        h.recorded = p.recorded;
        h.last_valid = p.last_valid;
        h.last_key = p.last_key;
        if (p.record) {
            h.key = key;
            h.recorded = true;
        }
        return p;
    }
    // two launches of `key`: the second records
    void record(const OrderKey& key) {
        launch(nullptr, key);
        launch(nullptr, key);
    }
};

template <class Set>
void field_row(const char* row, Set set) {
    const OrderKey A = make_key(1);
    OrderKey other = A;
    set(other);
    Cache c;
    c.record(A);
    c.launch(row, other);
}

}  // namespace

int main() {
    const OrderKey A = make_key(1), B = make_key(2);
    {  // rows 1, 2: the cache off, a launch it cannot serve -- over a recorded key
        Cache c;
        c.record(A);
        c.launch("1_mode_off", A, true, 1000, 0);
        Cache d;
        d.record(A);
        d.launch("2_not_cacheable", A, true, 1000, 1, false);
        d.launch("2_then_A", A);  // last_valid was cleared: a first launch again
    }
    {  // rows 3-5
        Cache c;
        c.launch("3_first_A", A);
        c.launch("4_second_A", A);
        c.launch("5_third_A", A);
    }
    {  // row 6: directions not final
        Cache c;
        c.launch(nullptr, A);
        c.launch("6_repeated_not_final", A, false);
        c.launch("6_then_final", A);  // still repeated: records now
        c.launch("6_recorded_not_final", A, false);
        c.launch("6_recorded_final_again", A);
    }
    {  // rows 7, 8
        Cache c;
        c.record(A);
        c.launch("7_recorded_A_then_B", B);
        c.launch("8_then_A", A);
        c.launch("8_A_after_it", A);
    }
    {  // row 9: the cap
        Cache c;
        c.record(A);
        c.h.max_bytes = 999;
        c.launch("9_over_cap", A);
        Cache d;
        d.record(A);
        d.h.max_bytes = 1000;
        d.launch("9_at_cap", A);
    }
    {  // rows 10, 11: a size known not to fit
        Cache c;
        c.record(A);
        c.h.no_room = 1000;
        c.launch("10_need_eq_no_room", A);
        Cache d;
        d.record(A);
        d.h.no_room = 900;
        d.launch("10_need_gt_no_room", A);
        Cache e;
        e.h.no_room = 1001;
        e.launch("11_first_A", A);
        e.launch("11_second_A", A);
        e.launch("11_third_A", A);
    }
    // row 12: one field differs, over a recorded A
    field_row("12_scene_gen", [](OrderKey& k) { k.scene_gen += 1; });
    field_row("12_tree_hash", [](OrderKey& k) { k.tree_hash ^= 1; });
    field_row("12_seed", [](OrderKey& k) { k.seed += 1; });
    field_row("12_ray_begin", [](OrderKey& k) { k.ray_begin += 1; });
    field_row("12_ray_end", [](OrderKey& k) { k.ray_end -= 1; });
    field_row("12_emitter_x", [](OrderKey& k) { k.emitter[0] = 0.25f; });
    field_row("12_emitter_y", [](OrderKey& k) { k.emitter[1] = 0.25f; });
    field_row("12_emitter_z", [](OrderKey& k) { k.emitter[2] = 0.25f; });
    field_row("12_e0", [](OrderKey& k) { k.e0 = 2e-4f; });
    field_row("12_energy_thres", [](OrderKey& k) { k.energy_thres = 2e-7f; });
    field_row("12_hrtf", [](OrderKey& k) { k.hrtf = 0.25f; });
    field_row("12_dist_limit", [](OrderKey& k) { k.dist_limit = 688.0f; });
    field_row("12_max_bounces", [](OrderKey& k) { k.max_bounces = 9; });
    field_row("12_is_mono", [](OrderKey& k) { k.is_mono = 1; });
    field_row("12_same_key", [](OrderKey&) {});  // the control: the same key replays
    return 0;
}
