// rtk_kernel_choice.h -- which rtk_render_kernel<real, FEAT, COUNT, IN_LDS> a launch runs, and the list of the ones that are
// compiled.  Host arithmetic only (no HIP, no SceneView): launch_chosen, render_kernel_name and view_kernel_name
// (rtk_trace.hip) fill Inputs from a SceneView and ask choose; launch_chosen then launches the row of the table that the answer
// names, and nothing else; the kernels' __launch_bounds__ ask max_threads.  tests/helpers/kernel_choice_check.cpp asks the
// same questions without a device.  DESIGN.md, "The instantiation table" and "Kernel choice", state the rule in words.
#ifndef RTK_KERNEL_CHOICE_H
#define RTK_KERNEL_CHOICE_H

#include <stdio.h>

#include "rtk_lds_plan.h"

namespace rtk {
namespace kernel_choice {

// The bits of the FEAT word that the choice reads and rtk_lds_plan.h does not already restate, and the four families
// (rtk_device_layout.h: Feature, kFeat*; rtk_trace.hip asserts that they agree).
using lds_plan::kF32Box, lds_plan::kLdsBoxes, lds_plan::kLeanFamily, lds_plan::kMatte;
constexpr uint32_t kFmaBox = 1u << 7, kSphereMediaOnly = 1u << 11;
constexpr uint32_t kMeshFamily = 66, kQuadBoxFamily = 69, kFullFamily = 127;
// The scene's family: FEAT without the bits that describe the hierarchy, the program or the staging.
inline constexpr uint32_t family(uint32_t feat) { return feat & ~uint32_t(kFmaBox | kF32Box | kMatte | kLdsBoxes | kSphereMediaOnly); }

// Variant bits (A/B, tests): the slot program although the upload built a MIXED / COMPACT one; no F_LDS_BOXES; the hot/cold
// form of the COMPACT program although the whole would fit.
constexpr uint32_t kVariantSlot = 1u << 20, kVariantNoLdsBoxes = 1u << 21, kVariantCold = 1u << 23;

struct Inputs {
    size_t real_bytes = 8;        // sizeof(real)
    uint32_t features = 0;        // the scene's mask with the upload's F_FMA_BOX / F_MATTE / F_SPHERE_MEDIA_ONLY
    bool count = false, allow_lds = true;
    uint32_t diag = 0;            // the variant word
    bool has_mixed = false, has_compact = false, has_hot = false, has_box_cache = false;  // what the upload built
    lds_plan::Counts n;
};

// Which instantiation a launch uses -- decided in ONE place, for the launcher and for rtk_kernel_name alike.
struct Choice {
    uint32_t feat;   // template FEAT word, F_LDS_BOXES included
    bool count, in_lds;
};

// Kernel instantiation for a scene: the leanest feature subset that covers it, with or without the fused slab test;
// `mixed` / `compact` = the scene has that program and the caller did not ask for the f64 boxes.
inline constexpr uint32_t kernel_features_base(uint32_t features, bool count, bool mixed, bool compact) {
    const uint32_t fma = features & kFmaBox, matte = features & kMatte, scene = features & ~uint32_t(kFmaBox | kMatte);
    // counting instantiations: the MIXED program has its own (the kernel bench.py times on sphere-only scenes, with
    // counters), the COMPACT program counts with the full-feature kernel on that program, everything else with the
    // full-feature kernel on the slot program (exact boxes: these counters equal the oracle's)
    if (count) return (mixed && scene == kLeanFamily) ? (kLeanFamily | kF32Box) : (compact ? (kFullFamily | kF32Box) : (kFullFamily | fma));
    if (scene == kLeanFamily) return mixed ? (kLeanFamily | kF32Box) : (kLeanFamily | fma);
    if ((scene & ~kQuadBoxFamily) == 0) return kQuadBoxFamily | matte | (compact ? kF32Box : 0u);  // slot program: no registers to spare for o*inv at 4 waves/SIMD (it spills): exact slab test, A/B on C3 40.7 vs 42.2 ms
    if ((scene & ~kMeshFamily) == 0) return kMeshFamily | matte | (compact ? kF32Box : fma);
    return kFullFamily | (compact ? kF32Box : fma);
}
inline constexpr uint32_t kernel_features(uint32_t features, bool count, bool mixed, bool compact) {
    const uint32_t sphere_media = count ? 0u : (features & kSphereMediaOnly);  // (the counting kernels serve every scene: no restriction)
    const uint32_t base = kernel_features_base(features & ~kSphereMediaOnly, count, mixed, compact);
    return base == (kFullFamily | kF32Box) ? (base | sphere_media) : base;  // the COMPACT full-feature kernels (what bench.py times on C5) have the restricted variant
}

inline constexpr Choice choose(const Inputs& in) {
    const bool f64 = in.real_bytes == 8;
    const lds_plan::RecordSizes& sizes = f64 ? lds_plan::kSizesF64 : lds_plan::kSizesF32;
    // The f32-culling-box programs are used whenever the upload built one (f64, fast order): the MIXED program of a sphere-only
    // scene, the COMPACT program of any other; kVariantSlot keeps the f64 boxes of the slot program instead.
    const bool mixed = f64 && in.has_mixed && (in.diag & kVariantSlot) == 0;
    bool compact = f64 && in.has_compact && (in.diag & kVariantSlot) == 0;
    bool cold = false;
    if (compact) {
        // Only when it fits one CU's LDS.  A COMPACT program split between LDS (box heads) and memory (primitives) is slower
        // than the slot program split the same way, measured: C4 with 4 494 ops 175 ms against 95 ms, C5 714 against 838
        // Msamples/s (there the coordinates run into the thousands -- a fog boundary of radius 5000 -- and the 2^-19 x extent
        // margin exceeds a quad's own box thickness: +55 % quad tests).
        const size_t mat_bytes = in.n.materials * sizes.material;
        if (!(in.allow_lds && lds_plan::whole_fits(in.n.units16 * lds_plan::kUnit16Bytes, mat_bytes)) || (in.diag & kVariantCold) != 0) {
            // ... unless its hot part does (COLD kernels: quads and triangles stay in memory, everything else in LDS) -- full-feature family, timed kernels
            const uint32_t scene = in.features & ~uint32_t(kFmaBox | kMatte | kSphereMediaOnly);
            cold = in.allow_lds && !in.count && in.has_hot && lds_plan::hot_fits(in.n.hot_units * lds_plan::kUnit16Bytes, mat_bytes) &&
                   (in.diag & kVariantNoLdsBoxes) == 0 && (scene & ~kQuadBoxFamily) != 0 && (scene & ~kMeshFamily) != 0;
            compact = cold;
        }
    }
    // the matte variants pay off in f64 only (C3: f64 34.8 -> 31.9 ms, f32 26.6 -> 36.5 ms at one more wave per SIMD)
    Choice k{kernel_features(f64 ? in.features : (in.features & ~kMatte), in.count, mixed, compact), in.count, false};
    const bool fits = in.allow_lds && lds_plan::whole_fits(lds_plan::image_bytes(in.n, sizes, k.feat), 0);
    if (in.count) {  // counting builds: only the MIXED one stages its program (it is the timed kernel with counters)
        k.in_lds = fits && (k.feat & kF32Box) != 0 && !lds_plan::is_compact(k.feat);
        return k;
    }
    k.in_lds = fits;
    if (!fits && !cold) k.feat &= ~kSphereMediaOnly;  // (the restricted variant exists for the LDS-resident forms only)
    if (cold) {
        k.in_lds = false;
        k.feat |= kLdsBoxes;
        return k;
    }
    // a program larger than LDS whose box records are not: the boxes-in-LDS kernel (mesh and full-feature families)
    if (!fits && !(k.feat & kF32Box) && in.has_box_cache && (family(k.feat) == kMeshFamily || family(k.feat) == kFullFamily) &&
        (in.diag & kVariantNoLdsBoxes) == 0)
        k.feat |= kLdsBoxes;
    return k;
}

// Workgroup-size bound = register budget: 1024 threads -> 4 waves per SIMD, 128 VGPRs; 768 -> 3 waves, 168 VGPRs;
// 512 -> 2 waves, 256 VGPRs.  Measured on C2 (lean f64 kernel): 2 waves 93.8 ms, 3 waves 73.5 ms, 4 waves 68.5 ms
// per frame (the 4-wave build spills a few values in the shade path).  Same-box A/B for the other f64 kernels
// (tools/ab/run_ab.sh): quad/box subset on C3 43.3 ms at 4 waves vs 48.7 at 3; mesh subset on C4 no difference;
// the full-feature kernel, which needs far more registers (~560 B/lane of spills at 168), is fastest at 2 waves.
constexpr int kThreadsAllF64 = 768;    // workgroup bound of the full-feature f64 kernels: 3 waves per SIMD, 168 VGPRs (measured against 512 = 2 waves and 1024 = 4)
constexpr int kThreadsMeshF64 = 1024;  // workgroup bound of the f64 mesh kernels: 4 waves per SIMD, 128 VGPRs (C4 60.1 -> 53.0 ms; 768 = 3 waves)
// (round 3) the f64 mesh kernels run at four waves per SIMD when the whole program is staged in LDS (C4 60.1 -> 53.0 ms, 44 B of
// scratch); with the program, or all but its boxes, in memory a fourth wave only adds pressure on L2 (C4, program in global
// memory: 23.2 ms at three waves, 33.6 at four), so those keep 768 threads.
inline constexpr int max_threads(size_t real_bytes, uint32_t feat, bool in_lds) {
    // ... and the full-feature f64 kernels run at three waves where the traversal data is in LDS -- the whole program, or the
    // hot part of a COMPACT program (F_LDS_BOXES | F_F32_BOX: C5 at 16 spp 21.1 -> 17.7 ms) -- and stay at two where records
    // come from memory (program in global memory 25.5 vs 29.1 ms at three; slot program with its boxes in LDS 25.6 vs 29.0).
    const bool hot_cold = (feat & kLdsBoxes) != 0 && (feat & kF32Box) != 0;
    if (real_bytes == 8)
        return family(feat) == kFullFamily ? ((in_lds || hot_cold) ? kThreadsAllF64 : 512)
                                           : ((family(feat) == kLeanFamily || family(feat) == kQuadBoxFamily) ? 1024 : (in_lds ? kThreadsMeshF64 : 768));
    return 768;
}
// Which instantiations have a view kernel: the non-counting ones that stage the program, its hot part or its boxes in LDS.
inline constexpr bool has_view_kernel(uint32_t feat, bool count, bool in_lds) { return !count && (in_lds || (feat & kLdsBoxes) != 0); }

// The compiled instantiations, X(FEAT, COUNT, IN_LDS): DESIGN.md's instantiation table, and the only list of them.  FEAT is
// family + 128 F_FMA_BOX + 256 F_F32_BOX + 512 F_MATTE + 1024 F_LDS_BOXES + 2048 F_SPHERE_MEDIA_ONLY.
#define RTK_RENDER_KERNELS_BOTH(X) /* double and float: the slot program, with and without F_FMA_BOX */ \
    X(0, false, false) X(0, false, true) X(128, false, false) X(128, false, true)                       \
    X(69, false, false) X(69, false, true)                                                              \
    X(66, false, false) X(66, false, true) X(194, false, false) X(194, false, true)                     \
    X(127, false, false) X(127, false, true) X(127, true, false)                                        \
    X(255, false, false) X(255, false, true) X(255, true, false)                                        \
    X(1090, false, false) X(1218, false, false) X(1151, false, false) X(1279, false, false)
#define RTK_RENDER_KERNELS_F64(X) /* double only: MIXED (256), COMPACT (F_F32_BOX on another family), F_MATTE */ \
    X(256, false, false) X(256, false, true) X(256, true, false) X(256, true, true)                     \
    X(325, false, true) X(837, false, true) X(322, false, true) X(834, false, true)                     \
    X(383, false, true) X(383, true, false) X(2431, false, true) X(1407, false, false) X(3455, false, false) \
    X(581, false, false) X(581, false, true)                                                            \
    X(578, false, false) X(578, false, true) X(706, false, false) X(706, false, true)                   \
    X(1602, false, false) X(1730, false, false)

inline constexpr bool is_compiled(size_t real_bytes, uint32_t feat, bool count, bool in_lds) {
#define RTK_ROW_IS(F, C, L) \
    if (feat == F && count == C && in_lds == L) return true;
    RTK_RENDER_KERNELS_BOTH(RTK_ROW_IS)
    if (real_bytes == 8) {
        RTK_RENDER_KERNELS_F64(RTK_ROW_IS)
    }
#undef RTK_ROW_IS
    return false;
}

// What rtk_kernel_name / rtk_view_kernel_name print and a kernel trace shows behind `rtk::`.
inline int format_name(char* out, size_t size, size_t real_bytes, const Choice& k, bool view) {
    const char* real = real_bytes == 8 ? "double" : "float";
    if (view) return snprintf(out, size, "rtk_view_batch_kernel<%s, %uu, %s>", real, k.feat, k.in_lds ? "true" : "false");
    return snprintf(out, size, "rtk_render_kernel<%s, %uu, %s, %s>", real, k.feat, k.count ? "true" : "false", k.in_lds ? "true" : "false");
}

}  // namespace kernel_choice
}  // namespace rtk

#endif  // RTK_KERNEL_CHOICE_H
