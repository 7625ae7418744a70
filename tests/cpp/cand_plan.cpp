// cand_plan.cpp -- the candidate kernel's numbering of a list's parts (csrc/arx_cand_plan.hpp) walked on the host
// as replay_cand_kernel walks it: the heads in tiles of kCandTile, kCandHeadsPerLane consecutive heads a lane, a
// scan of the lanes' part counts, the first lane whose scan passes part r its owner, cand_lane_item in that lane.
// Input: a file of cases, one per line: a name, the blocks of the launch, the stretches, and every stretch's
// candidate count.  Output per case:
//   case <name> <blocks> <stretches> <parts in all>
//   block <j> <stretch>:<part>:<candidates> ...        the parts block j takes, in its order; every block
// tests/test_cand_plan_host.py writes the cases and holds the expectation (a plain double loop).
//
//   g++ -std=c++17 -I audiorenderingv2_amd/csrc tests/cpp/cand_plan.cpp -o cand_plan && ./cand_plan cases.txt
#include <cstdio>
#include <vector>

#include "arx_cand_plan.hpp"

using namespace arx;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* in = std::fopen(argv[1], "r");
    if (!in) return 2;
    char name[64];
    unsigned blocks, fblocks;
    while (std::fscanf(in, "%63s %u %u", name, &blocks, &fblocks) == 3) {
        std::vector<uint32_t> heads(fblocks);
        uint32_t items = 0;
        for (uint32_t& h : heads) {
            if (std::fscanf(in, "%u", &h) != 1) return 3;
            items += cand_parts(h);
        }
        std::printf("case %s %u %u %u\n", name, blocks, fblocks, items);
        for (uint32_t j = 0; j < blocks; ++j) {
            std::printf("block %u", j);
            uint32_t k = j, done = 0;
            for (uint32_t t0 = 0; t0 < fblocks && k < items; t0 += kCandTile) {
                uint32_t cand[64][kCandHeadsPerLane], parts[64], incl[64], sum = 0;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    parts[lane] = 0;
                    for (uint32_t i = 0; i < kCandHeadsPerLane; ++i) {
                        const uint32_t fb = t0 + lane * kCandHeadsPerLane + i;
                        cand[lane][i] = fb < fblocks ? heads[fb] : 0u;
                        parts[lane] += cand_parts(cand[lane][i]);
                    }
                    incl[lane] = sum += parts[lane];
                }
                while (k < done + incl[63]) {
                    const uint32_t r = k - done;
                    uint32_t owner = 0;
                    while (!(incl[owner] > r)) ++owner;
                    const CandItem it = cand_lane_item(cand[owner], r - (incl[owner] - parts[owner]));
                    std::printf(" %u:%u:%u", t0 + owner * kCandHeadsPerLane + it.head, it.part, it.n_cand);
                    k += blocks;
                }
                done += incl[63];
            }
            std::printf("\n");
        }
    }
    std::fclose(in);
    return 0;
}
