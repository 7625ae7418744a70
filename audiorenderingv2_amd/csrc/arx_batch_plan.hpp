// arx_batch_plan.hpp -- what a batch of listeners costs and how it is laid out, as arithmetic on sizes:
// arx_render_listeners (bands = 0) and arx_render_listener_bands (bands = the table's) take the chunk's
// scratch, the call's pinned block, the byte terms of arx_debug_listener_bytes / arx_debug_listener_band_bytes
// and the chunk from here.
//
// Host only and free of HIP, so that a host test can walk it through every shape (tests/cpp/batch_plan.cpp).
// The buffers behind it live in ListenerScratch (arx_internal.hpp); the driver is run_listener_call
// (arx_capi_listeners.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/arx.h"
#include "arx_layout.hpp"

namespace arx {

constexpr int32_t kMaxBands = 8;          // ARX_MAX_BANDS
constexpr int32_t kBandCounterWords = 8;  // a counter block: [0] queries [1] receiver hits [2] misses, padding
constexpr uint64_t kListenerBudget = 512ull << 20;  // scratch of an automatic chunk

// Regions handed out one behind the other, each rounded up to `align` bytes.
struct Take {
    uint64_t align, at = 0;
    uint64_t operator()(uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + align - 1) & ~(align - 1);
        return o;
    }
};

// A listener's cells -- histograms, IR pairs and result triples: one per band, one for the plain batch --
// and its counter words: a kBandCounterWords block per cell, then one whose first word is its candidate tally.
inline uint64_t batch_cells(int32_t bands) { return bands > 0 ? (uint64_t)bands : 1; }
inline uint64_t batch_counter_words(int32_t bands) { return (batch_cells(bands) + 1) * kBandCounterWords; }

// bytes of one slot in the node and triangle arrays: its nodes (64-B and 32-B), triangle records and top node
inline uint64_t listener_slot_bytes(int64_t recv_nodes, int64_t recv_tris) {
    return (uint64_t)recv_nodes * (sizeof(BvhNode) + sizeof(QNode2)) + (uint64_t)recv_tris * sizeof(TriRec) +
           (sizeof(BvhNode) + sizeof(QNode2));
}

// The byte terms of include/arx.h: per listener of a chunk, and per call (the band call's per-ray counts and
// base counter block).
inline uint64_t batch_bytes_each(uint64_t n, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t bands) {
    const uint64_t L = (uint64_t)ir_len;
    return listener_slot_bytes(recv_nodes, recv_tris) + sizeof(ListenerEntry) + path_filter_list_bytes(n) +
           4 * listener_work_words(n) + batch_cells(bands) * (24 * L + kBandCounterWords * 8 + 3 * sizeof(arx_acoustics)) +
           kBandCounterWords * 8 + (bands > 0 ? 8 * L : 0);
}
inline uint64_t batch_bytes_fixed(uint64_t n, int32_t bands) {
    return bands > 0 ? 8 * n + (uint64_t)kMaxBands * kBandCounterWords * 8 : 0;
}

// Listeners per chunk: the forced chunk, or what the budget holds behind the fixed part (0: not even one),
// at most kListenerChunkMax and never more than the poses left.
inline int32_t batch_chunk(int32_t forced, uint64_t budget, uint64_t fixed, uint64_t each, size_t left) {
    uint64_t c = forced > 0 ? (uint64_t)forced : budget > fixed ? (budget - fixed) / each : 0;
    if (forced <= 0 && c > (uint64_t)kListenerChunkMax) c = (uint64_t)kListenerChunkMax;
    return (int32_t)(c < left ? c : left);
}

// The scratch of a chunk of `chunk` listeners of n rays, as byte offsets, every region 16-B aligned.  What does
// not depend on the chunk comes first: the band call's 8 B per ray of counts and its base counter block, the
// decay curves of one analysis and the analysis kernels' scratch.  Then per listener: a candidate list with its
// heads, the work items, a table entry, per cell a histogram, the counter words, per cell three results and an
// f32 IR pair (the chunk's lefts [listener][cell], then its rights); the band call's broadband pair last.
struct BatchScratch {
    uint64_t counts, base, edc, acou, lists, list_stride, work, work_stride, table, hist, counters, res, ir, bb, total;
};
inline BatchScratch batch_scratch(uint64_t n, int32_t ir_len, int32_t bands, int32_t chunk, uint64_t acou_bytes) {
    BatchScratch s;
    Take take{16};
    const uint64_t J = (uint64_t)chunk, L = (uint64_t)ir_len, C = batch_cells(bands);
    s.counts = take(bands > 0 ? 8 * n : 0);
    s.base = take(bands > 0 ? (uint64_t)kMaxBands * kBandCounterWords * 8 : 0);
    s.edc = take(24 * L);
    s.acou = take(acou_bytes);
    s.list_stride = path_filter_list_bytes(n);
    s.lists = take(J * s.list_stride);
    s.work_stride = 4 * listener_work_words(n);
    s.work = take(J * s.work_stride);
    s.table = take(J * sizeof(ListenerEntry));
    s.hist = take(J * C * 16 * L);
    s.counters = take(J * batch_counter_words(bands) * 8);
    s.res = take(J * C * 3 * sizeof(arx_acoustics));
    s.ir = take(J * C * 8 * L);
    s.bb = take(bands > 0 ? J * 8 * L : 0);
    s.total = take.at;
    return s;
}

// The pinned block of a call of n listeners, as byte offsets: the table entries by batched order; the counter
// words and the results by batched order in [0, n) and -- the plain call alone, whose one-listener route
// reports through the block -- by pose index in [n, 2n); the tree's off-grid flag as the chunks left it.
struct BatchPinned {
    size_t entries, counters, res, flag, total;
};
inline BatchPinned batch_pinned(size_t n, int32_t bands) {
    BatchPinned p;
    const size_t rows = bands > 0 ? n : 2 * n;
    p.entries = 0;
    p.counters = n * sizeof(ListenerEntry);
    p.res = p.counters + rows * (size_t)batch_counter_words(bands) * 8;
    p.flag = p.res + rows * (size_t)batch_cells(bands) * 3 * sizeof(arx_acoustics);
    p.total = p.flag + 16;
    return p;
}

}  // namespace arx
