// tests/test_grid_plan.py asks rtk_grid_plan.h its questions through this program: one query per line on stdin, one line of
// integers per answer on stdout.  No device, no HIP: the header only.
//
//   plan CUS OCCUPANCY_WAVES MAX_WAVES_PER_BLOCK LDS_BLOCKS_PER_CU N_ITEMS CAP -> blocks threads
//   cap K                       -> cap_waves(K)
// Started with the argument "sweep" it reads nothing and writes the whole grid of the test as raw int32 pairs {blocks, threads}:
// CUs 1..304 x occupancy waves 1..40 x max_waves_per_block 4, 8, 16 x LDS limit 1..8 x the n_items below x cap 0..7, the
// last index fastest (21 million plans: text would take longer to parse than the test may run).
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rtk_grid_plan.h"

using namespace rtk::grid_plan;

static const int kItems[] = {1, 2, 63, 64, 65, 4095, 4096, 4097, 1000000};

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "sweep") {
        std::vector<int32_t> out;
        for (int cus = 1; cus <= 304; cus++) {
            out.clear();
            for (int waves = 1; waves <= 40; waves++)
                for (int max_wpb : {4, 8, 16})
                    for (int by_lds = 1; by_lds <= 8; by_lds++)
                        for (int n_items : kItems)
                            for (int cap = 0; cap <= 7; cap++) {
                                const Grid g = plan(cus, waves, max_wpb, by_lds, n_items, cap);
                                out.push_back(g.blocks);
                                out.push_back(g.threads);
                            }
            if (std::fwrite(out.data(), sizeof(int32_t), out.size(), stdout) != out.size()) return 3;
        }
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "plan") {
            int cus, waves, max_wpb, by_lds, n_items, cap;
            in >> cus >> waves >> max_wpb >> by_lds >> n_items >> cap;
            if (!in || cus < 1 || max_wpb < 1 || n_items < 1) return 2;
            const Grid g = plan(cus, waves, max_wpb, by_lds, n_items, cap);
            std::printf("%d %d\n", g.blocks, g.threads);
        } else if (what == "cap") {
            int k;
            in >> k;
            if (!in) return 2;
            std::printf("%d\n", cap_waves(k));
        } else {
            return 2;
        }
    }
    return 0;
}
