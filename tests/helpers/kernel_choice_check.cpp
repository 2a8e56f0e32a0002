// tests/test_kernel_choice.py asks rtk_kernel_choice.h its questions through this program: one query per line on stdin, one
// line of integers per answer on stdout (`table`: one line per row; `name`: the string).  No device, no HIP: the header only.
//
//   choose REAL FEATURES COUNT ALLOW_LDS DIAG HAS_MIXED HAS_COMPACT HAS_HOT HAS_BOX_CACHE slots units units16 hot_units cached_boxes
//          kind_words rank_words materials perlins chains
//          -> feat count in_lds is_compiled has_view_kernel max_threads     (the last three: of the chosen instantiation)
//   table  -> real_bytes feat count in_lds, one line per compiled instantiation
//   name REAL FEAT COUNT IN_LDS VIEW -> rtk_render_kernel<...> (VIEW 0) or rtk_view_batch_kernel<...> (VIEW 1)
// REAL is 8 or 4.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "rtk_kernel_choice.h"

using namespace rtk::kernel_choice;

// the header's functions are constexpr: the counting MIXED kernel of a small sphere scene, decided by the compiler
static_assert(choose(Inputs{8, kFmaBox, true, true, 0, true, false, false, false, {25, 30, 0, 0, 0, 0, 0, 4, 0, 0}}).feat == 256 && is_compiled(8, 256, true, true) &&
                  !is_compiled(4, 256, true, true) && max_threads(8, 256, true) == 1024,
              "rtk_kernel_choice.h");

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "choose") {
            unsigned long long real, v[8], c[10];
            in >> real;
            for (auto& x : v) in >> x;
            for (auto& x : c) in >> x;
            if (!in || (real != 8 && real != 4)) return 2;
            Inputs q;
            q.real_bytes = size_t(real), q.features = uint32_t(v[0]), q.count = v[1] != 0, q.allow_lds = v[2] != 0, q.diag = uint32_t(v[3]);
            q.has_mixed = v[4] != 0, q.has_compact = v[5] != 0, q.has_hot = v[6] != 0, q.has_box_cache = v[7] != 0;
            q.n.slots = c[0], q.n.units = c[1], q.n.units16 = c[2], q.n.hot_units = c[3], q.n.cached_boxes = c[4], q.n.kind_words = c[5], q.n.rank_words = c[6];
            q.n.materials = c[7], q.n.perlins = c[8], q.n.chains = c[9];
            const Choice k = choose(q);
            std::printf("%u %d %d %d %d %d\n", k.feat, int(k.count), int(k.in_lds), int(is_compiled(q.real_bytes, k.feat, k.count, k.in_lds)),
                        int(has_view_kernel(k.feat, k.count, k.in_lds)), max_threads(q.real_bytes, k.feat, k.in_lds));
        } else if (what == "table") {
#define RTK_PRINT_ROW(F, C, L) std::printf("%d %d %d %d\n", real, F, int(C), int(L));
            for (int real : {8, 4}) {
                RTK_RENDER_KERNELS_BOTH(RTK_PRINT_ROW)
                if (real == 8) {
                    RTK_RENDER_KERNELS_F64(RTK_PRINT_ROW)
                }
            }
#undef RTK_PRINT_ROW
        } else if (what == "name") {
            unsigned long long real, feat, count, in_lds, view;
            in >> real >> feat >> count >> in_lds >> view;
            if (!in || (real != 8 && real != 4)) return 2;
            char name[96];
            const int n = format_name(name, sizeof name, size_t(real), Choice{uint32_t(feat), count != 0, in_lds != 0}, view != 0);
            if (n < 0 || size_t(n) >= sizeof name) return 3;
            std::printf("%s\n", name);
        } else {
            return 2;
        }
    }
    return 0;
}
