// The listener batches' plan (csrc/arx_batch_plan.hpp) walked over bands x chunk x rays x ir_len: every
// region's offset and size of the chunk scratch and the pinned block, the byte terms, and the chunk choice.
// Stand-alone and host only; tests/test_batch_plan_host.py builds it, runs it and checks what it prints.
#include <cstdio>

#include "arx_batch_plan.hpp"

using namespace arx;

namespace {

constexpr uint64_t kAcou = 4100;  // an analysis scratch size that is no multiple of 16
constexpr int64_t kRecvNodes = 1019, kRecvTris = 1020;

void region(const char* name, uint64_t at, uint64_t bytes) {
    std::printf(" %s:%llu:%llu", name, (unsigned long long)at, (unsigned long long)bytes);
}

void scratch_row(int32_t B, int32_t J, uint64_t n, int32_t L) {
    const BatchScratch s = batch_scratch(n, L, B, J, kAcou);
    const uint64_t j = (uint64_t)J, l = (uint64_t)L, c = batch_cells(B);
    std::printf("scratch %d %d %llu %d %llu", B, J, (unsigned long long)n, L, (unsigned long long)s.total);
    region("counts", s.counts, B > 0 ? 8 * n : 0);
    region("base", s.base, B > 0 ? (uint64_t)kMaxBands * kBandCounterWords * 8 : 0);
    region("edc", s.edc, 24 * l);
    region("acou", s.acou, kAcou);
    region("lists", s.lists, j * s.list_stride);
    region("work", s.work, j * s.work_stride);
    region("table", s.table, j * sizeof(ListenerEntry));
    region("hist", s.hist, j * c * 16 * l);
    region("counters", s.counters, j * batch_counter_words(B) * 8);
    region("res", s.res, j * c * 3 * sizeof(arx_acoustics));
    region("ir", s.ir, j * c * 8 * l);
    region("bb", s.bb, B > 0 ? j * 8 * l : 0);
    std::printf(" strides:%llu:%llu\n", (unsigned long long)s.list_stride, (unsigned long long)s.work_stride);
}

void pinned_row(int32_t B, size_t n) {
    const BatchPinned p = batch_pinned(n, B);
    const size_t rows = B > 0 ? n : 2 * n;
    std::printf("pinned %d %zu %zu", B, n, p.total);
    region("entries", p.entries, n * sizeof(ListenerEntry));
    region("counters", p.counters, rows * batch_counter_words(B) * 8);
    region("res", p.res, rows * batch_cells(B) * 3 * sizeof(arx_acoustics));
    region("flag", p.flag, 16);
    std::printf("\n");
}

void chunk_row(const char* name, int32_t got) { std::printf("chunk %s %d\n", name, got); }

}  // namespace

int main() {
    const int32_t bands[] = {0, 1, 4, 5, 8}, chunks[] = {1, 2, 64}, lens[] = {1, 16000};
    const uint64_t rays[] = {1, 1024, 1025};
    for (const int32_t B : bands)
        for (const int32_t J : chunks) {
            pinned_row(B, (size_t)J);
            for (const uint64_t n : rays)
                for (const int32_t L : lens) {
                    scratch_row(B, J, n, L);
                    if (J == 1)
                        std::printf("bytes %d %llu %d %llu %llu\n", B, (unsigned long long)n, L,
                                    (unsigned long long)batch_bytes_each(n, L, kRecvNodes, kRecvTris, B),
                                    (unsigned long long)batch_bytes_fixed(n, B));
                }
        }
    // the chunk: a forced one, the figures of include/arx.h, a budget below the fixed part, the cap
    const uint64_t n = 1000000;
    const int32_t L = 96000;
    chunk_row("forced_5_left_3", batch_chunk(5, kListenerBudget, 0, 1, 3));
    chunk_row("forced_5_left_9", batch_chunk(5, kListenerBudget, 0, 1, 9));
    chunk_row("header_8_bands", batch_chunk(0, kListenerBudget, batch_bytes_fixed(n, 8),
                                            batch_bytes_each(n, L, kRecvNodes, kRecvTris, 8), 1000));
    chunk_row("header_4_bands", batch_chunk(0, kListenerBudget, batch_bytes_fixed(n, 4),
                                            batch_bytes_each(n, L, kRecvNodes, kRecvTris, 4), 1000));
    chunk_row("header_8_bands_left_9", batch_chunk(0, kListenerBudget, batch_bytes_fixed(n, 8),
                                                   batch_bytes_each(n, L, kRecvNodes, kRecvTris, 8), 9));
    chunk_row("budget_below_fixed", batch_chunk(0, batch_bytes_fixed(n, 8) - 1, batch_bytes_fixed(n, 8), 1, 1000));
    chunk_row("budget_at_fixed", batch_chunk(0, batch_bytes_fixed(n, 8), batch_bytes_fixed(n, 8), 1, 1000));
    chunk_row("cap", batch_chunk(0, kListenerBudget, 0, 1, 1000));
    chunk_row("cap_small_listeners", batch_chunk(0, kListenerBudget, batch_bytes_fixed(4096, 8),
                                                 batch_bytes_each(4096, 16000, kRecvNodes, kRecvTris, 8), 1000));
    return 0;
}
