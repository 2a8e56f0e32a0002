// tests/test_lds_plan.py asks rtk_lds_plan.h its questions through this program: one query per line on stdin, one line of
// integers per answer on stdout.  No device, no HIP: the header and its record-size constants only.
//
//   plan REAL FEAT IN_LDS N_TILES HAS_ORDER slots units units16 hot_units cached_boxes kind_words rank_words materials perlins chains
//        -> total mats_lds_offset perlin_lds_offset chains_lds_offset order_in_lds order_lds_offset
//   whole PROGRAM_BYTES MATERIAL_BYTES        -> 0 | 1      (rows a, b)
//   hot HOT_BYTES MATERIAL_BYTES              -> 0 | 1      (row b)
//   boxes REAL SLOT_BYTES MATERIAL_BYTES N_BOXES N_KIND_WORDS N_RANK_WORDS -> wants_table table_bytes table_fits   (row c)
//   launch LDS_BYTES                          -> workgroups_per_cu needs_opt_in   (row h)
//   sizes REAL                                -> slot box material perlin chain mixed_unit unit16 capacity
// REAL is 8 or 4.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "rtk_lds_plan.h"

using namespace rtk::lds_plan;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "plan") {
            unsigned long long real, feat, in_lds, n_tiles, has_order, c[10];
            in >> real >> feat >> in_lds >> n_tiles >> has_order;
            for (auto& x : c) in >> x;
            if (!in || (real != 8 && real != 4)) return 2;
            Counts n;
            n.slots = c[0], n.units = c[1], n.units16 = c[2], n.hot_units = c[3], n.cached_boxes = c[4], n.kind_words = c[5], n.rank_words = c[6];
            n.materials = c[7], n.perlins = c[8], n.chains = c[9];
            const Plan p = plan(n, real == 8 ? kSizesF64 : kSizesF32, uint32_t(feat), in_lds != 0, size_t(n_tiles), has_order != 0);
            std::printf("%zu %d %d %d %d %d\n", p.total, p.mats_lds_offset, p.perlin_lds_offset, p.chains_lds_offset, p.order_in_lds, p.order_lds_offset);
        } else if (what == "whole" || what == "hot") {
            unsigned long long a, b;
            in >> a >> b;
            if (!in) return 2;
            std::printf("%d\n", int(what == "whole" ? whole_fits(size_t(a), size_t(b)) : hot_fits(size_t(a), size_t(b))));
        } else if (what == "boxes") {
            unsigned long long real, slot_bytes, mat_bytes, n_boxes, n_kind, n_rank;
            in >> real >> slot_bytes >> mat_bytes >> n_boxes >> n_kind >> n_rank;
            if (!in || (real != 8 && real != 4)) return 2;
            const size_t bytes = box_table_bytes(size_t(n_boxes), (real == 8 ? kSizesF64 : kSizesF32).box, size_t(n_kind), size_t(n_rank));
            std::printf("%d %zu %d\n", int(wants_box_table(size_t(slot_bytes), size_t(mat_bytes))), bytes, int(box_table_fits(bytes)));
        } else if (what == "launch") {
            unsigned long long lds;
            in >> lds;
            if (!in || lds == 0) return 2;
            std::printf("%d %d\n", workgroups_per_cu(size_t(lds)), int(needs_opt_in(size_t(lds))));
        } else if (what == "sizes") {
            unsigned long long real;
            in >> real;
            if (!in || (real != 8 && real != 4)) return 2;
            const RecordSizes s = real == 8 ? kSizesF64 : kSizesF32;
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", s.slot, s.box, s.material, s.perlin, s.chain, kMixedUnitBytes, kUnit16Bytes, kCapacity);
        } else {
            return 2;
        }
    }
    return 0;
}
