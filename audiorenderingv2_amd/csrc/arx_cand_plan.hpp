// arx_cand_plan.hpp -- which part of a candidate list a block of replay_cand_kernel (arx_replay.hip) takes, as
// arithmetic on the heads' counts.
//
// A stretch is a filter block's kFilterBlock slots of the list; its head says how many candidates it holds, and
// a part is 64 of them, a lane each.  The parts that hold a candidate are numbered in stretch order, within a
// stretch by position.  A wave reads the heads in tiles, kCandHeadsPerLane consecutive heads a lane, and scans
// the lanes' part counts; the lane whose range holds part r of the tile finds the stretch and the position
// here.  Host and device, free of HIP, so that a host test can walk the numbering against the plain double
// loop over stretches and parts (tests/cpp/cand_plan.cpp).
#pragma once
#include <cstdint>

#include "arx_layout.hpp"

namespace arx {

constexpr uint32_t kCandPart = 64;         // entries of a part: a lane of one wave each
constexpr uint32_t kCandHeadsPerLane = 4;  // heads a lane reads per tile: independent loads
constexpr uint32_t kCandTile = 64 * kCandHeadsPerLane;

// The parts a stretch of n_cand candidates has: none without a candidate.
ARX_HOST_DEVICE inline uint32_t cand_parts(uint32_t n_cand) { return (n_cand + kCandPart - 1u) / kCandPart; }

// Part `at` of a lane's heads, counted over cand_parts of cand[0], cand[1], ...: the head it lies in
// (kCandHeadsPerLane if `at` is past the lane's parts), its position there, and that head's candidates.
struct CandItem { uint32_t head, part, n_cand; };
ARX_HOST_DEVICE inline CandItem cand_lane_item(const uint32_t (&cand)[kCandHeadsPerLane], uint32_t at) {
    CandItem it = {0u, at, 0u};
    for (uint32_t i = 0; i < kCandHeadsPerLane; ++i) {
        const uint32_t p = cand_parts(cand[i]);
        if (it.head == i) {  // not found yet
            if (it.part < p) {
                it.n_cand = cand[i];
            } else {
                it.part -= p;
                ++it.head;
            }
        }
    }
    return it;
}

}  // namespace arx
