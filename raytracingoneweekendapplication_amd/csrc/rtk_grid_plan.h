// rtk_grid_plan.h -- the grid of a persistent render launch: how many workgroups of how many threads.  Host arithmetic
// only (no HIP): plan_launch (rtk_trace.hip) asks the occupancy API and rtk_lds_plan.h for the inputs and launches what this
// answers; tests/helpers/grid_plan_check.cpp asks the same questions without a device.  The kernels take work items from
// a counter, so any grid renders the same frame ("What the scheduler tests can see"): the grid decides how many
// items a wave takes, never what a pixel is.
#ifndef RTK_GRID_PLAN_H
#define RTK_GRID_PLAN_H

namespace rtk {
namespace grid_plan {

struct Grid {
    int blocks, threads;          // the launch
    int waves_per_cu;             // the register-limited count as used (4..32)
    int blocks_per_cu, waves_per_block;  // of the uncapped plan (the debug line prints them)
};

// Waves of a grid cap: variant bits 5..7 = k, 0 = no cap, k = 1..7 -> at most 2^(k-1) waves (1, 2, 4, ... 64).
inline constexpr int cap_waves(int cap) { return cap <= 0 ? 0 : 1 << ((cap > 7 ? 7 : cap) - 1); }

// cus: compute units; occupancy_waves: register-limited waves per CU as the occupancy API reports them (any value: used as
// 4..32); max_waves_per_block: the kernel's launch bound / 64; lds_blocks_per_cu: workgroups per CU whose LDS fits, 0 = the
// kernel stages nothing (no limit); n_items: work items of the launch (>= 1); cap: variant bits 5..7.
//
// Uncapped: enough workgroups per CU to reach the wave count (at most what LDS allows), the waves shared among them, one grid
// slot per CU and workgroup, and never more waves than work items.
// Capped (tests and tools only): a plan of more than cap_waves(cap) waves becomes exactly that many -- one workgroup of
// cap x 64 threads where the cap is below a workgroup's waves, otherwise workgroups of the largest power of two of waves
// that a workgroup of the uncapped plan holds (so that they divide the cap).  A plan within the cap is left as it is: the
// cap never adds a wave.
inline constexpr Grid plan(int cus, int occupancy_waves, int max_waves_per_block, int lds_blocks_per_cu, int n_items, int cap) {
    int waves_per_cu = occupancy_waves;
    if (waves_per_cu < 4) waves_per_cu = 4;
    if (waves_per_cu > 32) waves_per_cu = 32;
    int blocks_per_cu = (waves_per_cu + max_waves_per_block - 1) / max_waves_per_block;
    if (lds_blocks_per_cu > 0 && blocks_per_cu > lds_blocks_per_cu) blocks_per_cu = lds_blocks_per_cu;
    int waves_per_block = waves_per_cu / blocks_per_cu;
    if (waves_per_block > max_waves_per_block) waves_per_block = max_waves_per_block;
    if (waves_per_block < 1) waves_per_block = 1;
    int threads = waves_per_block * 64;
    int blocks = cus * blocks_per_cu;
    const int needed = (n_items + waves_per_block - 1) / waves_per_block;
    if (blocks > needed) blocks = needed;
    if (blocks < 1) blocks = 1;
    const int limit = cap_waves(cap);
    if (limit > 0 && (long long)blocks * waves_per_block > limit) {
        if (limit < waves_per_block) {
            blocks = 1;
            threads = limit * 64;
        } else {
            int pow2 = 1;
            while (pow2 * 2 <= waves_per_block) pow2 *= 2;
            threads = pow2 * 64;
            blocks = limit / pow2;
        }
    }
    return Grid{blocks, threads, waves_per_cu, blocks_per_cu, waves_per_block};
}

}  // namespace grid_plan
}  // namespace rtk

#endif
