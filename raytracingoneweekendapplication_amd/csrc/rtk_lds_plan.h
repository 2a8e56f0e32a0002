// rtk_lds_plan.h -- what a workgroup of the render kernels stages in LDS, and at which byte offsets of its dynamic
// segment.  Host arithmetic only (no HIP, no SceneView): the upload (rtk_api.cpp) asks it which tables to build,
// kernel_choice::choose (rtk_kernel_choice.h) and launch_one (rtk_trace.hip) ask it which kernel form a scene takes and where its tables go, and
// tests/helpers/lds_plan_check.cpp asks it the same questions without a device.  The kernel body (rtk_render_body.inc)
// trusts the offsets of a Plan without checking them; DESIGN.md, "The LDS staging plan", states the rule in words.
// Every comparison with the LDS capacity of a CU is in this file.
#ifndef RTK_LDS_PLAN_H
#define RTK_LDS_PLAN_H

#include <stddef.h>
#include <stdint.h>

namespace rtk {
namespace lds_plan {

constexpr size_t kCapacity = 160 * 1024;          // LDS bytes of one gfx950 CU (rtk_device_layout.h: kLdsBytesPerCU)
constexpr size_t kReserve = 64;                   // kept free by every "is there room behind ..." test
constexpr size_t kMaxSplitMaterialBytes = 16 * 1024;  // a larger material table stays in memory behind a box table
constexpr size_t kMaxChainBytes = 8192;           // larger chain tables stay in memory
constexpr size_t kOptInAbove = 64 * 1024;         // dynamic LDS beyond this needs hipFuncAttributeMaxDynamicSharedMemorySize

// The bits of the FEAT word that the plan reads (rtk_device_layout.h: Feature; rtk_trace.hip asserts that they agree).
constexpr uint32_t kXform = 1u << 2, kTexture = 1u << 4, kF32Box = 1u << 8, kMatte = 1u << 9, kLdsBoxes = 1u << 10;
constexpr uint32_t kLeanFamily = 0;

// Record sizes in bytes (rtk_trace.hip asserts that they are the sizeof of rtk_device_layout.h's records).
struct RecordSizes {
    size_t slot, box, material, perlin, chain;
};
constexpr size_t kMixedUnitBytes = 32, kUnit16Bytes = 16;
constexpr RecordSizes kSizesF64{64, 56, 48, 9216, 120};
constexpr RecordSizes kSizesF32{32, 32, 32, 6144, 68};

// Record counts of an uploaded scene (SceneView's n_* members).
struct Counts {
    size_t slots = 0, units = 0, units16 = 0, hot_units = 0;      // slot, MIXED, COMPACT programs; hot part of the COMPACT one
    size_t cached_boxes = 0, kind_words = 0, rank_words = 0;      // the F_LDS_BOXES tables
    size_t materials = 0, perlins = 0, chains = 0;
};

inline constexpr size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

// F_F32_BOX on any family but the lean one: the COMPACT program (the lean family's is the MIXED program).
inline constexpr bool is_compact(uint32_t feat) { return (feat & kF32Box) != 0 && (feat & ~uint32_t(kF32Box | kMatte | kLdsBoxes)) != kLeanFamily; }

// (a), (b): a whole program -- slots, MIXED units or COMPACT units -- with the material table behind it.
inline constexpr bool whole_fits(size_t program_bytes, size_t material_bytes) { return program_bytes + material_bytes <= kCapacity; }
// (b): the hot part of a COMPACT program with the material table behind it (the COLD kernels' image).
inline constexpr bool hot_fits(size_t hot_bytes, size_t material_bytes) { return hot_bytes + material_bytes + kReserve <= kCapacity; }
// (c): the upload builds the box table of a slot program that cannot be staged whole ...
inline constexpr bool wants_box_table(size_t slot_bytes, size_t material_bytes) { return !whole_fits(slot_bytes, material_bytes); }
// ... when the table itself can: box records, kind nibbles (padded to 8 bytes), rank words.
inline constexpr size_t box_table_bytes(size_t n_boxes, size_t box_record_bytes, size_t n_kind_words, size_t n_rank_words) {
    return n_boxes * box_record_bytes + ((n_kind_words * 4 + 7) & ~size_t(7)) + n_rank_words * 8;
}
inline constexpr bool box_table_fits(size_t table_bytes) { return table_bytes + kReserve <= kCapacity; }

// The program a kernel stages whole (IN_LDS) with the material table behind it.
inline constexpr size_t image_bytes(const Counts& n, const RecordSizes& s, uint32_t feat) {
    const size_t program = is_compact(feat) ? n.units16 * kUnit16Bytes : ((feat & kF32Box) ? n.units * kMixedUnitBytes : n.slots * s.slot);
    return program + n.materials * s.material;
}
// What an F_LDS_BOXES kernel always stages: COLD, the hot program and the materials; SPLIT, the box table.
inline constexpr size_t split_bytes(const Counts& n, const RecordSizes& s, uint32_t feat) {
    if (is_compact(feat)) return n.hot_units * kUnit16Bytes + n.materials * s.material;
    return box_table_bytes(n.cached_boxes, s.box, n.kind_words, n.rank_words);
}

// Workgroups of `lds_bytes` dynamic LDS that one CU holds (0: the launch is impossible); lds_bytes > 0.
inline constexpr int workgroups_per_cu(size_t lds_bytes) { return int(kCapacity / lds_bytes); }
// (h)
inline constexpr bool needs_opt_in(size_t lds_bytes) { return lds_bytes > kOptInAbove; }

struct Plan {
    size_t total = 0;  // dynamic LDS bytes of the launch
    int32_t mats_lds_offset = 0, perlin_lds_offset = 0, chains_lds_offset = 0;  // 0 = that table stays in memory
    int32_t order_in_lds = 0, order_lds_offset = 0;
};

// (d)-(g): the tables behind what the kernel <FEAT, IN_LDS> always stages, in the kernel's order: materials (SPLIT
// only), Perlin tables, instance chains, tile order.  `has_order`: the launch was given a learned tile order.
inline constexpr Plan plan(const Counts& n, const RecordSizes& s, uint32_t feat, bool in_lds, size_t n_tiles_local, bool has_order) {
    Plan p;
    size_t lds = in_lds ? image_bytes(n, s, feat) : ((feat & kLdsBoxes) ? split_bytes(n, s, feat) : 0);
    if ((feat & kLdsBoxes) != 0) {  // boxes-in-LDS kernels: the material table too, if it is small and there is room
        const size_t mat_bytes = n.materials * s.material;
        const size_t at = align16(lds);
        if (!is_compact(feat) /* (COLD kernels always stage it, right behind the hot program) */ && mat_bytes <= kMaxSplitMaterialBytes &&
            at + mat_bytes + kReserve <= kCapacity) {
            p.mats_lds_offset = int32_t(at);
            lds = at + mat_bytes;
        }
        // ... and the Perlin tables (book-2's noise sphere: 7.8 % of the C5 frame went into perlin::turb's dependent gathers from memory)
        const size_t perlin_bytes = n.perlins * s.perlin;
        const size_t pat = align16(lds);
        if ((feat & kTexture) != 0 && perlin_bytes > 0 && pat + perlin_bytes + kReserve <= kCapacity) {
            p.perlin_lds_offset = int32_t(pat);
            lds = pat + perlin_bytes;
        }
    }
    if ((feat & kXform) != 0 && (in_lds || (feat & kLdsBoxes) != 0)) {
        const size_t chain_bytes = n.chains * s.chain;
        const size_t cat = align16(lds);
        if (n.chains > 1 && chain_bytes <= kMaxChainBytes && cat + chain_bytes + kReserve <= kCapacity) {
            p.chains_lds_offset = int32_t(cat);
            lds = cat + chain_bytes;
        }
    }
    // room for the tile order behind everything?  (never at the price of a second resident workgroup's LDS)
    p.order_lds_offset = int32_t(align16(lds));
    const size_t order_end = size_t(p.order_lds_offset) + n_tiles_local * sizeof(int32_t);
    if (has_order && order_end <= kCapacity && (lds == 0 || kCapacity / lds == kCapacity / order_end)) {
        p.order_in_lds = 1;
        lds = order_end;
    }
    p.total = lds;
    return p;
}

}  // namespace lds_plan
}  // namespace rtk

#endif  // RTK_LDS_PLAN_H
