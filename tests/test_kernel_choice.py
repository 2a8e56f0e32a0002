"""CPU test of csrc/rtk_kernel_choice.h, the host arithmetic that decides which rtk_render_kernel<real, FEAT, COUNT, IN_LDS> a
launch runs and lists the instantiations that are compiled ("Kernel choice" and "The instantiation table").
tests/helpers/kernel_choice_check.cpp -- a stand-alone program over the header alone, built with the address and
undefined-behaviour sanitizers -- answers queries; the expected answers come from `ref_choose` below, a second statement of
DESIGN.md's rule written from its words.

The inputs are enumerated, not sampled: both real types, ten scene masks, every hierarchy flag, count, allow_lds, the eight
settings of the three variant bits, the sixteen settings of what the upload built, and four size classes.  On every input the
header must agree with the restated rule; on every input that an upload can produce the choice must be a compiled
instantiation, and the one that the removed launch ladder would have launched for it; and the choices over those inputs must
be the table, no more and no less."""
import itertools
import os
import subprocess

import pytest

from tests import kernel_matrix as km
from tests.conftest import ROOT
from tests.test_lds_plan import CAPACITY, COUNT_NAMES, MIXED_UNIT, PKG, UNIT16, counts, pad8, record_sizes

F_MEDIA, F_FMA_BOX, F_F32_BOX, F_MATTE, F_LDS_BOXES, F_SPHERE_MEDIA_ONLY = 8, 128, 256, 512, 1024, 2048
LEAN, MESH, QUADBOX, FULL = 0, 66, 69, 127
V_SLOT, V_NO_LDS_BOXES, V_COLD = km.V_SLOT, km.V_NO_LDS_BOXES, km.V_COLD

SCENE_MASKS = (0, 1, 2, 3, 4, 8, 64, 66, 69, 127)
SIZE_CLASSES = ("whole", "hot", "boxes", "nothing")
MATERIALS = 4


def class_counts(real, size_class):
    """Record counts of a size class: the byte totals on either side of the capacity, from the record sizes of `real`."""
    s = record_sizes(real)
    mats = MATERIALS * s["material"]
    over = lambda record: (CAPACITY - mats) // record + 1                    # the first count whose program + materials exceeds C
    small = counts(slots=100, units=100, units16=400, hot_units=300, cached_boxes=50, kind_words=13, rank_words=4, materials=MATERIALS)
    large = counts(slots=over(s["slot"]), units=over(MIXED_UNIT), units16=over(UNIT16), hot_units=over(UNIT16), cached_boxes=CAPACITY // s["box"] + 1,
                   kind_words=over(s["slot"]) // 8 + 1, rank_words=over(s["slot"]) // 32 + 1, materials=MATERIALS)
    n = dict(small if size_class == "whole" else large)
    if size_class == "hot":
        n["hot_units"] = (CAPACITY - 64 - mats) // UNIT16                      # the largest hot part that fits
    if size_class == "boxes":
        tables = pad8(4 * n["kind_words"]) + 8 * n["rank_words"]
        n["cached_boxes"] = (CAPACITY - 64 - tables) // s["box"]               # the largest box table that fits
    fits = dict(slots=n["slots"] * s["slot"] + mats <= CAPACITY, units=n["units"] * MIXED_UNIT + mats <= CAPACITY, units16=n["units16"] * UNIT16 + mats <= CAPACITY,
                hot=hot_fits(real, n), boxes=box_table_fits(real, n))
    want = {"whole": dict(slots=True, units=True, units16=True, hot=True, boxes=True), "hot": dict(slots=False, units=False, units16=False, hot=True, boxes=False),
            "boxes": dict(slots=False, units=False, units16=False, hot=False, boxes=True), "nothing": dict.fromkeys(("slots", "units", "units16", "hot", "boxes"), False)}
    assert fits == want[size_class], (real, size_class, fits)
    return n


def hot_fits(real, n):
    return n["hot_units"] * UNIT16 + n["materials"] * record_sizes(real)["material"] + 64 <= CAPACITY


def box_table_fits(real, n):
    return n["cached_boxes"] * record_sizes(real)["box"] + pad8(4 * n["kind_words"]) + 8 * n["rank_words"] + 64 <= CAPACITY


def family_of_scene(scene):
    """The leanest family that covers a scene mask (quad/box before mesh: a mask of F_EXOTIC_MAT alone is quad/box)."""
    if scene == 0:
        return LEAN
    if scene & ~QUADBOX == 0:
        return QUADBOX
    if scene & ~MESH == 0:
        return MESH
    return FULL


def ref_choose(real, features, count, allow_lds, diag, has_mixed, has_compact, has_hot, has_box_cache, n):
    """DESIGN.md, "Kernel choice": the program first, then the FEAT word, then what is staged."""
    s = record_sizes(real)
    mats = n["materials"] * s["material"]
    scene = features & ~(F_FMA_BOX | F_MATTE | F_SPHERE_MEDIA_ONLY)
    family = family_of_scene(scene)
    f32_boxes = real == 8 and not diag & V_SLOT
    # 1. the program
    program = "slot"
    if f32_boxes and has_compact:
        if allow_lds and n["units16"] * UNIT16 + mats <= CAPACITY and not diag & V_COLD:
            program = "compact"
        elif allow_lds and not count and has_hot and hot_fits(real, n) and not diag & V_NO_LDS_BOXES and family == FULL:
            program = "cold"
    if f32_boxes and has_mixed and family == LEAN:
        program = "mixed"
    # 2. the FEAT word
    fma = features & F_FMA_BOX
    matte = features & F_MATTE if real == 8 else 0
    if count:
        feat = {"mixed": LEAN | F_F32_BOX, "compact": FULL | F_F32_BOX}.get(program, FULL | fma)
    elif family == LEAN:
        feat = LEAN | F_F32_BOX if program == "mixed" else LEAN | fma
    elif family == QUADBOX:
        feat = QUADBOX | matte | (F_F32_BOX if program == "compact" else 0)
    elif family == MESH:
        feat = MESH | matte | (F_F32_BOX if program == "compact" else fma)
    else:
        feat = FULL | (F_F32_BOX if program in ("compact", "cold") else fma)
    # 3. staging
    on_compact = bool(feat & F_F32_BOX) and feat & ~(F_F32_BOX | F_MATTE) != LEAN
    program_bytes = n["units16"] * UNIT16 if on_compact else (n["units"] * MIXED_UNIT if feat & F_F32_BOX else n["slots"] * s["slot"])
    fits = allow_lds and program_bytes + mats <= CAPACITY
    if count:
        return feat, True, fits and feat == LEAN | F_F32_BOX
    if program == "cold":
        return feat | F_LDS_BOXES | (features & F_SPHERE_MEDIA_ONLY), False, False
    if fits:
        return feat | (features & F_SPHERE_MEDIA_ONLY if feat == FULL | F_F32_BOX else 0), False, True
    if not feat & F_F32_BOX and has_box_cache and family in (MESH, FULL) and not diag & V_NO_LDS_BOXES:
        feat |= F_LDS_BOXES
    return feat, False, False


# The chain of `if constexpr` blocks that launched a choice before the table did (launch_chosen's switch on the FEAT word without
# F_LDS_BOXES and F_SPHERE_MEDIA_ONLY, then launch_feat's rungs, each falling through to the next): the removed code, restated
# rung by rung and kept as the record that exact matching changed no launch.
LADDER_CASES = {4: {LEAN, QUADBOX, MESH, LEAN | 128, MESH | 128, FULL, FULL | 128}}
LADDER_CASES[8] = LADDER_CASES[4] | {QUADBOX | 512, MESH | 512, MESH | 128 | 512, LEAN | 256, QUADBOX | 256, QUADBOX | 512 | 256, MESH | 256, MESH | 512 | 256, FULL | 256}


def ref_ladder(real, choice):
    """-> the (FEAT, COUNT, IN_LDS) the removed chain launched for `choice`, None where it returned hipErrorInvalidValue."""
    feat, count, in_lds = choice
    F = feat & ~(F_LDS_BOXES | F_SPHERE_MEDIA_ONLY)
    smo = feat & F_SPHERE_MEDIA_ONLY
    if F not in LADDER_CASES[real]:
        return None
    if F & ~F_FMA_BOX == FULL and count:
        return F, True, False
    if F == LEAN | F_F32_BOX and count:
        return F, True, in_lds
    if F == FULL | F_F32_BOX:
        if count:
            return F, True, False
        if feat & F_LDS_BOXES:
            return F | F_LDS_BOXES | smo, False, False
        if in_lds and smo:
            return F | smo, False, True
    if not F & F_F32_BOX and F & ~(F_FMA_BOX | F_MATTE) in (MESH, FULL) and feat & F_LDS_BOXES:
        return F | F_LDS_BOXES, False, False
    if in_lds:
        return F, False, True
    if F & F_F32_BOX and F & ~(F_F32_BOX | F_MATTE) != LEAN:
        return None
    return F, False, False


def consistent(real, features, diag, has_mixed, has_compact, has_hot, has_box_cache, n):
    """Whether build_device_scene / upload_scene (rtk_api.cpp) can produce this view of a scene."""
    s = record_sizes(real)
    scene = features & ~(F_FMA_BOX | F_MATTE | F_SPHERE_MEDIA_ONLY)
    fast = bool(features & F_FMA_BOX)                       # `hierarchy_flags = fast_order ? uint32_t(F_FMA_BOX) : 0u`
    if (has_mixed or has_compact) and not (real == 8 and fast):
        return False                                        # `if constexpr (sizeof(real) == 8)` around `if (fast_order && want_mixed) ... else if (fast_order)`
    if real == 8 and fast and has_mixed == has_compact:
        return False                                        # ... one branch or the other: exactly one of the two programs
    if has_mixed and scene != LEAN:
        return False                                        # `want_mixed = fast_order && prog.features == kFeatLean && ...`
    if has_hot and not (has_compact and family_of_scene(scene) == FULL and hot_fits(real, n)):
        return False                                        # `if ((prog.features & ~kFeatQuadBox) != 0 && (prog.features & ~kFeatMesh) != 0)`, `if (lds_plan::hot_fits(...) && ...)`
    if has_box_cache and not (n["slots"] * s["slot"] + n["materials"] * s["material"] > CAPACITY and box_table_fits(real, n)):
        return False                                        # `if (lds_plan::wants_box_table(...))`, `if (!boxes.empty() && lds_plan::box_table_fits(bytes))`
    if features & F_SPHERE_MEDIA_ONLY and not scene & F_MEDIA:
        return False                                        # `if ((prog.features & F_MEDIA) != 0 && !prog.has_media_bracket) hierarchy_flags |= F_SPHERE_MEDIA_ONLY`
    return True


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kernel_choice") / "kernel_choice_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "helpers", "kernel_choice_check.cpp"), "-I" + os.path.join(PKG, "csrc"), "-o", exe])

    def run(lines):
        p = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        return p.stdout.splitlines()
    return run


def ints(lines):
    return [tuple(int(x) for x in line.split()) for line in lines]


@pytest.fixture(scope="module")
def table(ask):
    """The header's list of compiled instantiations as (real bytes, FEAT, COUNT, IN_LDS)."""
    rows = [(real, feat, bool(count), bool(in_lds)) for real, feat, count, in_lds in ints(ask(["table"]))]
    assert len(rows) == len(set(rows))
    return rows


@pytest.fixture(scope="module")
def enumeration(ask):
    """Every input with the header's answer: [(input, (feat, count, in_lds), is_compiled, has_view_kernel, max_threads)]."""
    sizes = {(real, c): class_counts(real, c) for real in (8, 4) for c in SIZE_CLASSES}
    variants = [a | b | c for a in (0, V_SLOT) for b in (0, V_NO_LDS_BOXES) for c in (0, V_COLD)]
    flags = [a | b | c for a in (0, F_FMA_BOX) for b in (0, F_MATTE) for c in (0, F_SPHERE_MEDIA_ONLY)]
    inputs = []
    for real, scene, flag, count, allow_lds, diag, has, size_class in itertools.product(
            (4, 8), SCENE_MASKS, flags, (False, True), (False, True), variants, itertools.product((False, True), repeat=4), SIZE_CLASSES):
        inputs.append((real, scene | flag, count, allow_lds, diag, *has, sizes[real, size_class]))
    lines = ["choose %d %d %d %d %d %d %d %d %d " % tuple(int(x) for x in q[:9]) + " ".join(str(q[9][k]) for k in COUNT_NAMES) for q in inputs]
    got = ints(ask(lines))
    assert len(got) == len(inputs) == 2 * 10 * 8 * 2 * 2 * 8 * 16 * 4
    return [(q, (g[0], bool(g[1]), bool(g[2])), bool(g[3]), bool(g[4]), g[5]) for q, g in zip(inputs, got)]


def is_consistent(q):
    real, features, _count, _allow_lds, diag, has_mixed, has_compact, has_hot, has_box_cache, n = q
    return consistent(real, features, diag, has_mixed, has_compact, has_hot, has_box_cache, n)


def test_the_header_is_the_rule_on_every_input(enumeration):
    for q, choice, _, _, _ in enumeration:
        assert choice == ref_choose(*q), (q, choice, ref_choose(*q))


def test_every_producible_choice_is_compiled_and_is_what_the_ladder_launched(enumeration, table):
    n_consistent = 0
    for q, choice, compiled, _, _ in enumeration:
        assert compiled == ((q[0], *choice) in table), (q, choice)
        if is_consistent(q):
            n_consistent += 1
            assert compiled, (q, choice)
            assert ref_ladder(q[0], choice) == choice, (q, choice, ref_ladder(q[0], choice))
    assert n_consistent   # (that they reach every row of the table is the next test)


def test_the_choices_are_the_table_and_the_matrix_rows(enumeration, table):
    """"Unreachable: none": every compiled instantiation is chosen for some input an upload can produce, and nothing else is."""
    chosen = {(q[0], *choice) for q, choice, _, _, _ in enumeration if is_consistent(q)}
    assert chosen == set(table), {"chosen, not compiled": sorted(chosen - set(table)), "compiled, never chosen": sorted(set(table) - chosen)}
    rows = {(8 if real == km.F64 else 4, feat, count, in_lds) for real, feat, count, in_lds in (r.expect for r in km.ROWS)}
    assert rows == set(table), {"rows, not in the table": sorted(rows - set(table)), "in the table, no row": sorted(set(table) - rows)}
    assert len(table) == 61 and sum(r[0] == 8 for r in table) == 41 and not km.UNREACHABLE


def test_properties_of_every_choice(enumeration):
    for q, (feat, count, in_lds), _, _, _ in enumeration:
        real = q[0]
        family = feat & ~(F_FMA_BOX | F_F32_BOX | F_MATTE | F_LDS_BOXES | F_SPHERE_MEDIA_ONLY)
        assert family in (LEAN, MESH, QUADBOX, FULL), (q, feat)
        assert count == q[2]
        assert real == 8 or not feat & F_MATTE, (q, feat)
        assert not (feat & F_LDS_BOXES and in_lds), (q, feat)
        assert not feat & F_SPHERE_MEDIA_ONLY or in_lds or feat & F_LDS_BOXES, (q, feat)
        assert not count or family == FULL or feat == LEAN | F_F32_BOX, (q, feat)
        assert q[3] or not (in_lds or feat & F_F32_BOX and feat & F_LDS_BOXES), (q, feat)   # LDS not allowed: no program staged, whole or hot part


def ref_max_threads(real, feat, in_lds):
    """The workgroup bound: f32 768; f64 by family and by where the traversal data is ("Kernel choice")."""
    if real == 4:
        return 768
    family = feat & ~(F_FMA_BOX | F_F32_BOX | F_MATTE | F_LDS_BOXES | F_SPHERE_MEDIA_ONLY)
    if family == FULL:
        cold = bool(feat & F_LDS_BOXES) and bool(feat & F_F32_BOX)
        return 768 if in_lds or cold else 512
    if family == MESH:
        return 1024 if in_lds else 768
    return 1024


def test_thread_bounds_and_view_kernels_of_the_table(enumeration, table):
    seen = {}
    for q, choice, _, view, threads in enumeration:
        seen[(q[0], *choice)] = (view, threads)
    for row in table:
        real, feat, count, in_lds = row
        view, threads = seen[row]                                   # (every row is chosen: the test above)
        assert threads in (512, 768, 1024) and threads == ref_max_threads(real, feat, in_lds), row
        assert view == (not count and bool(in_lds or feat & 1024)), row


def test_names_are_the_ones_tests_and_traces_match_on(ask, table):
    for real, feat, count, in_lds in table:
        expect = (km.F64 if real == 8 else km.F32, feat, count, in_lds)
        got = ask(["name %d %d %d %d 0" % (real, feat, count, in_lds), "name %d %d 0 %d 1" % (real, feat, in_lds)])
        assert got[0] == km.kernel_name(expect), row_text(expect)
        assert got[1] == f"rtk_view_batch_kernel<{'double' if real == 8 else 'float'}, {feat}u, {'true' if in_lds else 'false'}>"


def row_text(expect):
    return "/".join(str(x) for x in expect)
