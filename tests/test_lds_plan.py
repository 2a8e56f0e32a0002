"""CPU test of csrc/rtk_lds_plan.h, the host arithmetic that decides what a render-kernel workgroup stages in LDS and at which
offsets ("The LDS staging plan").  tests/helpers/lds_plan_check.cpp -- a stand-alone program over the header alone,
built with the address and undefined-behaviour sanitizers -- answers queries; the expected answers come from `ref_*` below, a
second statement of DESIGN.md's table written from the table, with the record sizes worked out from the members that
rtk_device_layout.h declares.

For every row a-g: the largest input that takes the staged branch (found by a search in the restated rule and checked to be
within one record of the limit), that input plus one record, and the exact-equality input where the record sizes allow one.
Every plan must keep its offsets multiples of 16, its regions in the kernel's order without overlap, its total within the
capacity, the COLD form without a second material table, and the tile order from costing a resident workgroup."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

PKG = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
CAPACITY = 160 * 1024
F_XFORM, F_TEXTURE, F_F32_BOX, F_MATTE, F_LDS_BOXES = 4, 16, 256, 512, 1024
LEAN, MESH, QUADBOX, FULL = 0, 66, 69, 127


def record_sizes(real):
    """sizeof of rtk_device_layout.h's records for `real`-byte reals, from their members."""
    def struct(members, align):
        return -(-sum(members) // align) * align
    return {
        "slot": struct([(7 if real == 8 else 6) * real, 4, 4], 16),        # Slot: v[kReals], kind_payload, aux; alignas(16)
        "box": struct([6 * real, 4, 4], 8),                                # BoxRec: v[6], aux, unused; alignas(8)
        "material": struct([4 * real, 4 * 4], 16),                         # MaterialRec: albedo[3], param, four int32; alignas(16)
        "perlin": struct([256 * 3 * real, 3 * 256 * 4], real),             # PerlinRec: randvec[256][3], three int32[256]
        "chain": struct([4 + 4 * 4 + (4 if real == 8 else 0), 3 * 4 * real], real),  # ChainRec: count, is_rotate[4], (padding), a, b, c[4]
    }


MIXED_UNIT, UNIT16 = 32, 16
COUNT_NAMES = ("slots", "units", "units16", "hot_units", "cached_boxes", "kind_words", "rank_words", "materials", "perlins", "chains")


def align16(n):
    return (n + 15) // 16 * 16


def pad8(n):
    return (n + 7) // 8 * 8


def is_compact(feat):
    return bool(feat & F_F32_BOX) and (feat & ~(F_F32_BOX | F_MATTE | F_LDS_BOXES)) != LEAN


def ref_base(real, feat, in_lds, n):
    """-> (bytes the kernel always stages, end of the program or box table inside them)"""
    s = record_sizes(real)
    mats = n["materials"] * s["material"]
    if in_lds:
        program = n["units16"] * UNIT16 if is_compact(feat) else (n["units"] * MIXED_UNIT if feat & F_F32_BOX else n["slots"] * s["slot"])
        return program + mats, program
    if feat & F_LDS_BOXES:
        if is_compact(feat):
            return n["hot_units"] * UNIT16 + mats, n["hot_units"] * UNIT16
        table = n["cached_boxes"] * s["box"] + pad8(4 * n["kind_words"]) + 8 * n["rank_words"]
        return table, table
    return 0, 0


def ref_plan(real, feat, in_lds, n_tiles, has_order, n):
    """DESIGN.md's rows d-g -> (total, mats, perlin, chains, order_in_lds, order offset)"""
    s = record_sizes(real)
    lds, _ = ref_base(real, feat, in_lds, n)
    mats = perlin = chains = 0
    if feat & F_LDS_BOXES:
        mat_bytes = n["materials"] * s["material"]
        if not is_compact(feat) and mat_bytes <= 16384 and align16(lds) + mat_bytes + 64 <= CAPACITY:
            mats = align16(lds)
            lds = mats + mat_bytes
        perlin_bytes = n["perlins"] * s["perlin"]
        if feat & F_TEXTURE and n["perlins"] >= 1 and align16(lds) + perlin_bytes + 64 <= CAPACITY:
            perlin = align16(lds)
            lds = perlin + perlin_bytes
    if feat & F_XFORM and (in_lds or feat & F_LDS_BOXES):
        chain_bytes = n["chains"] * s["chain"]
        if n["chains"] > 1 and chain_bytes <= 8192 and align16(lds) + chain_bytes + 64 <= CAPACITY:
            chains = align16(lds)
            lds = chains + chain_bytes
    order = align16(lds)
    end = order + 4 * n_tiles
    staged = bool(has_order) and end <= CAPACITY and (lds == 0 or CAPACITY // lds == CAPACITY // end)
    return (end if staged else lds, mats, perlin, chains, int(staged), order)


def counts(**kw):
    n = dict.fromkeys(COUNT_NAMES, 0)
    n.update(kw)
    return n


def last_true(pred, hi=1 << 20):
    """The largest k >= 0 with pred(k), for a pred that is true up to some k and false beyond it."""
    assert pred(0) and not pred(hi)
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_plan") / "lds_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "helpers", "lds_plan_check.cpp"), "-I" + os.path.join(PKG, "csrc"), "-o", exe])

    def run(lines):
        p = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
        out = [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def plan_line(real, feat, in_lds, n_tiles, has_order, n):
    return "plan %d %d %d %d %d " % (real, feat, int(in_lds), n_tiles, int(has_order)) + " ".join(str(n[k]) for k in COUNT_NAMES)


def check_plans(ask, cases):
    """Every case (real, feat, in_lds, n_tiles, has_order, counts): the header's plan == the restated rule's, and the invariants."""
    got = ask([plan_line(*c) for c in cases])
    for case, g in zip(cases, got):
        real, feat, in_lds, n_tiles, has_order, n = case
        assert g == ref_plan(*case), (case, g, ref_plan(*case))
        total, mats, perlin, chains, order_in_lds, order = g
        s = record_sizes(real)
        base, program_end = ref_base(real, feat, in_lds, n)
        assert all(x % 16 == 0 for x in (mats, perlin, chains, order)), case
        assert total <= CAPACITY, case
        # regions in the kernel's order, none overlapping: [start, end) of what is staged
        regions = [(0, program_end)]
        if in_lds or (feat & F_LDS_BOXES and is_compact(feat)):
            regions.append((program_end, base))                    # the material table the kernel puts right behind the program
            assert program_end % 16 == 0
        if mats:
            regions.append((mats, mats + n["materials"] * s["material"]))
        if perlin:
            regions.append((perlin, perlin + n["perlins"] * s["perlin"]))
        if chains:
            regions.append((chains, chains + n["chains"] * s["chain"]))
        if order_in_lds:
            regions.append((order, order + 4 * n_tiles))
        for (a0, a1), (b0, b1) in zip(regions, regions[1:]):
            assert a0 <= a1 <= b0 <= b1, (case, regions)
        assert regions[-1][1] == total, (case, regions)
        if feat & F_LDS_BOXES and is_compact(feat):
            assert mats == 0, case                                 # COLD: no second material table
        if order_in_lds:
            before = regions[-2][1]
            assert has_order and (before == 0 or CAPACITY // before == CAPACITY // total), case
        else:
            assert order >= regions[-1][1]                         # where the kernel would look is never inside a staged region
    return got


def test_record_sizes_are_the_headers(ask):
    for real in (8, 4):
        s = record_sizes(real)
        assert ask(["sizes %d" % real]) == [(s["slot"], s["box"], s["material"], s["perlin"], s["chain"], MIXED_UNIT, UNIT16, CAPACITY)]
    assert record_sizes(8) == {"slot": 64, "box": 56, "material": 48, "perlin": 9216, "chain": 120}
    assert record_sizes(4) == {"slot": 32, "box": 32, "material": 32, "perlin": 6144, "chain": 68}
    layout = open(os.path.join(PKG, "csrc", "rtk_device_layout.h")).read()
    assert "sizeof(Slot<double>) == 64 && sizeof(Slot<float>) == 32" in layout and "sizeof(BoxRec<double>) == 56 && sizeof(BoxRec<float>) == 32" in layout
    assert "sizeof(MixedHead) == 32" in layout and "kLdsBytesPerCU = 160 * 1024" in layout


# (real, FEAT, count name, record bytes, material counts; the last one allows program + materials == CAPACITY exactly)
ROW_A = [(8, LEAN, "slots", 64, (1, 3, 4)), (4, LEAN, "slots", 32, (1, 3, 4)), (8, LEAN | F_F32_BOX, "units", 32, (1, 3, 2)),
         (8, MESH | F_F32_BOX, "units16", 16, (1, 2, 3)), (8, FULL | F_F32_BOX, "units16", 16, (1, 2, 3)), (8, FULL | 128, "slots", 64, (5, 7, 8))]


@pytest.mark.parametrize("real,feat,name,rec,material_counts", ROW_A)
def test_row_a_whole_program_and_materials(ask, real, feat, name, rec, material_counts):
    mat = record_sizes(real)["material"]
    for m in material_counts:
        n_max = last_true(lambda k: k * rec + m * mat <= CAPACITY)
        assert CAPACITY - rec < n_max * rec + m * mat <= CAPACITY
        assert ask(["whole %d %d" % (n_max * rec, m * mat), "whole %d %d" % ((n_max + 1) * rec, m * mat)]) == [(1,), (0,)]
        # the whole_fits(image, 0) form kernel_choice::choose uses
        assert ask(["whole %d 0" % (n_max * rec + m * mat), "whole %d 0" % ((n_max + 1) * rec + m * mat)]) == [(1,), (0,)]
        got = check_plans(ask, [(real, feat, True, 15, order, counts(**{name: n_max, "materials": m})) for order in (False, True)])
        assert got[0][0] == n_max * rec + m * mat
    m = material_counts[-1]
    n_max = last_true(lambda k: k * rec + m * mat <= CAPACITY)
    assert n_max * rec + m * mat == CAPACITY                       # the exact fit: nothing else gets in, not even one tile of the order
    got = check_plans(ask, [(real, feat, True, 1, True, counts(**{name: n_max, "materials": m, "chains": 2}))])
    assert got == [(CAPACITY, 0, 0, 0, 0, CAPACITY)]
    assert ask(["launch %d" % CAPACITY, "launch %d" % (CAPACITY // 2), "launch %d" % (CAPACITY // 2 + 16), "launch 65536", "launch 65552"]) == \
        [(1, 1), (2, 1), (1, 1), (2, 0), (2, 1)]


def test_row_b_compact_program_and_its_hot_part(ask):
    mat = record_sizes(8)["material"]
    for m in (1, 4, 9):
        h_max = last_true(lambda k: k * UNIT16 + m * mat + 64 <= CAPACITY)
        assert h_max * UNIT16 + m * mat + 64 == CAPACITY           # 16-byte units: the largest hot part is always the exact fit
        assert ask(["hot %d %d" % (h_max * UNIT16, m * mat), "hot %d %d" % ((h_max + 1) * UNIT16, m * mat)]) == [(1,), (0,)]
        for feat in (FULL | F_F32_BOX | F_LDS_BOXES, FULL | F_F32_BOX | F_LDS_BOXES | 2048):
            got = check_plans(ask, [(8, feat, False, 15, order, counts(units16=40000, hot_units=h_max, materials=m, chains=3, perlins=1)) for order in (False, True)])
            # hot program + materials, nothing behind them: 64 bytes are left, no room for a Perlin table, chains or 15 tiles at no cost
            assert got[0] == (CAPACITY - 64, 0, 0, 0, 0, CAPACITY - 64)
        # ... and with room: chains, then the order
        got = check_plans(ask, [(8, FULL | F_F32_BOX | F_LDS_BOXES, False, 15, True, counts(hot_units=2000, materials=m, chains=3))])
        assert got[0][1] == 0 and got[0][3] == align16(2000 * UNIT16 + m * mat)


def test_row_c_box_table_at_upload(ask):
    for real in (8, 4):
        s = record_sizes(real)
        m = 4
        n_fit = last_true(lambda k: k * s["slot"] + m * s["material"] <= CAPACITY)
        kind_words, rank_words = 200, 72
        tables = pad8(4 * kind_words) + 8 * rank_words
        b_max = last_true(lambda k: k * s["box"] + tables + 64 <= CAPACITY)
        assert CAPACITY - s["box"] < b_max * s["box"] + tables + 64 <= CAPACITY
        lines = ["boxes %d %d %d %d %d %d" % (real, slots * s["slot"], m * s["material"], boxes, kind_words, rank_words)
                 for slots, boxes in ((n_fit, b_max), (n_fit + 1, b_max), (n_fit + 1, b_max + 1))]
        assert ask(lines) == [(0, b_max * s["box"] + tables, 1), (1, b_max * s["box"] + tables, 1), (1, (b_max + 1) * s["box"] + tables, 0)]
        got = check_plans(ask, [(real, MESH | F_LDS_BOXES, False, 15, False, counts(slots=9999, cached_boxes=b_max, kind_words=kind_words, rank_words=rank_words, materials=m))])
        assert got[0][0] == b_max * s["box"] + tables and got[0][1] == 0     # the table alone: no room for the materials behind it
    # exact equality in f64: 2 900 boxes x 56 + 800 + 576 + 64 == 163 840; an odd kind-word count is padded to 8 bytes
    assert ask(["boxes 8 163841 0 2900 200 72", "boxes 8 163841 0 2900 199 72", "boxes 8 163841 0 2900 201 72"]) == \
        [(1, CAPACITY - 64, 1), (1, CAPACITY - 64, 1), (1, CAPACITY - 56, 0)]


@pytest.mark.parametrize("real", (8, 4))
def test_row_d_materials_behind_the_box_table(ask, real):
    s = record_sizes(real)
    feat = MESH | F_LDS_BOXES
    small = counts(slots=9999, cached_boxes=1000, kind_words=1250, rank_words=313)
    m_max = last_true(lambda k: k * s["material"] <= 16384)
    assert 16384 - s["material"] < m_max * s["material"] <= 16384 and (real == 8 or m_max * s["material"] == 16384)   # f32: 512 x 32 is the exact case
    got = check_plans(ask, [(real, feat, False, 15, False, dict(small, materials=m)) for m in (m_max, m_max + 1)])
    table = ref_base(real, feat, False, small)[0]
    assert got[0][1] == align16(table) and got[0][0] == align16(table) + m_max * s["material"]
    assert got[1][1] == 0 and got[1][0] == table
    # a small table, but the boxes leave no room: the box count straddles, with kind and rank words that leave the table's end off 16
    for m in (3, 100):
        tables = pad8(4 * 1251) + 8 * 313
        b_max = last_true(lambda k: align16(k * s["box"] + tables) + m * s["material"] + 64 <= CAPACITY)
        cases = [(real, feat, False, 15, False, counts(slots=9999, cached_boxes=b, kind_words=1251, rank_words=313, materials=m)) for b in (b_max, b_max + 1)]
        got = check_plans(ask, cases)
        assert got[0][1] == align16(b_max * s["box"] + tables) and CAPACITY - s["box"] - 16 < got[0][0] + 64 <= CAPACITY
        assert got[1][1] == 0
    # exact equality: 56 b + 5008 + 2504 == 16 k and + 48 m + 64 == CAPACITY
    if real == 8:
        b, m = 2778, 12                                             # 155 568 + 7 512 = 163 080 (a multiple of 8, not of 16) -> 163 088 + 576 + 64 = 163 728
        k = (CAPACITY - 64 - align16(b * 56 + tables)) // 48
        got = check_plans(ask, [(8, feat, False, 15, False, counts(slots=9999, cached_boxes=b, kind_words=1251, rank_words=313, materials=k))])
        assert got[0][1] == align16(b * 56 + tables) and got[0][1] != b * 56 + tables and m <= k


@pytest.mark.parametrize("real,cold", ((8, False), (4, False), (8, True)))   # (the COLD form is the COMPACT program's: f64 kernels only)
def test_row_e_perlin_tables(ask, real, cold):
    s = record_sizes(real)
    feat = FULL | F_LDS_BOXES | (F_F32_BOX if cold else 128)
    for base_records in (2000, 2301):
        if cold:
            n0 = counts(hot_units=base_records * 3, materials=7, chains=1)
        else:
            n0 = counts(slots=99999, cached_boxes=base_records, kind_words=1251, rank_words=313, materials=7, chains=1)
        before = ref_plan(real, feat, False, 15, False, n0)[0]       # what lies in front of the Perlin tables (SPLIT: with the materials)
        p_max = last_true(lambda k: k == 0 or align16(before) + k * s["perlin"] + 64 <= CAPACITY, hi=64)
        assert p_max >= 1 and CAPACITY - s["perlin"] < align16(before) + p_max * s["perlin"] + 64 <= CAPACITY
        got = check_plans(ask, [(real, feat, False, 15, False, dict(n0, perlins=p)) for p in (0, p_max, p_max + 1)])
        assert got[0][2] == 0 and got[1][2] == align16(before) and got[2][2] == 0 and got[2][0] == before
        assert got[1][0] == align16(before) + p_max * s["perlin"]
        # without F_TEXTURE the kernel has no staging code: never
        assert check_plans(ask, [(real, feat & ~F_TEXTURE, False, 15, False, dict(n0, perlins=p_max))])[0][2] == 0
    # exact equality, COLD: hot part + 7 materials + 64 + P tables == CAPACITY
    if cold:
        hot = (CAPACITY - 64 - 2 * s["perlin"] - 7 * 48) // 16
        n = counts(hot_units=hot, materials=7, perlins=2)
        assert hot * 16 + 7 * 48 + 2 * s["perlin"] + 64 == CAPACITY
        got = check_plans(ask, [(8, feat, False, 17, True, n), (8, feat, False, 17, True, dict(n, hot_units=hot + 1)), (8, feat, False, 16, True, n)])
        assert got[0] == (CAPACITY - 64, 0, hot * 16 + 7 * 48, 0, 0, CAPACITY - 64) and got[1][2] == 0
        assert got[2] == (CAPACITY, 0, hot * 16 + 7 * 48, 0, 1, CAPACITY - 64)     # the order has no reserve: 16 tiles fill the 64 bytes exactly
    # IN_LDS kernels never stage them
    assert check_plans(ask, [(real, FULL, True, 15, False, counts(slots=100, materials=7, perlins=1))])[0][2] == 0


@pytest.mark.parametrize("real", (8, 4))
def test_row_f_instance_chains(ask, real):
    s = record_sizes(real)
    k_max = last_true(lambda k: k * s["chain"] <= 8192)
    assert 8192 - s["chain"] < k_max * s["chain"] < 8192            # (no chain count gives 8 192 B exactly in either real type)
    for feat, in_lds, n0 in ((QUADBOX, True, counts(slots=301, materials=5)), (FULL | F_LDS_BOXES | 128, False, counts(slots=9999, cached_boxes=1001, kind_words=1251, rank_words=313, materials=5)),
                             (FULL | F_F32_BOX | F_LDS_BOXES, False, counts(hot_units=3001, materials=5))):
        if real == 4 and feat & F_F32_BOX:
            continue
        before = ref_plan(real, feat, in_lds, 15, False, n0)[0]
        got = check_plans(ask, [(real, feat, in_lds, 15, False, dict(n0, chains=k)) for k in (0, 1, 2, k_max, k_max + 1)])
        assert [g[3] for g in got] == [0, 0, align16(before), align16(before), 0]
        assert got[3][0] == align16(before) + k_max * s["chain"] and got[4][0] == before
        # a kernel without F_XFORM has no staging code
        assert check_plans(ask, [(real, feat & ~F_XFORM, in_lds, 15, False, dict(n0, chains=2))])[0][3] == 0
    # behind a box table that ends 8 bytes off a multiple of 16, with a material table too large to be staged in between
    n0 = counts(slots=9999, cached_boxes=1001, kind_words=1250, rank_words=313, materials=600, chains=3)
    table = ref_base(real, FULL | F_LDS_BOXES, False, n0)[0]
    got = check_plans(ask, [(real, FULL | F_LDS_BOXES, False, 15, True, n0)])
    assert (real == 4 or table % 16 == 8) and got[0][1] == 0 and got[0][3] == align16(table) and got[0][5] == align16(got[0][3] + 3 * s["chain"])
    # program in memory: nothing is staged, chains included
    assert check_plans(ask, [(real, QUADBOX, False, 15, False, counts(slots=301, materials=5, chains=2))])[0][:4] == (0, 0, 0, 0)
    # the room clause: K chains behind a program that leaves room for them or not (slots straddle)
    chain_bytes = 60 * s["chain"]
    n_max = last_true(lambda k: align16(k * s["slot"] + 5 * s["material"]) + chain_bytes + 64 <= CAPACITY)
    got = check_plans(ask, [(real, QUADBOX, True, 15, False, counts(slots=n, materials=5, chains=60)) for n in (n_max, n_max + 1)])
    assert got[0][3] == n_max * s["slot"] + 5 * s["material"] and CAPACITY - s["slot"] < got[0][0] + 64 <= CAPACITY and got[1][3] == 0
    # exact equality: f64, 64 n + 48 m + 120 k + 64 == CAPACITY with m = 1, k = 2: 64 n == 163 488 -- not a multiple of 64; m = 4, k = 8: 64 n = 162 624 = 64 x 2541
    if real == 8:
        got = check_plans(ask, [(8, QUADBOX, True, 17, True, counts(slots=2541, materials=4, chains=8)), (8, QUADBOX, True, 17, True, counts(slots=2542, materials=4, chains=8))])
        assert got[0] == (CAPACITY - 64, 0, 0, 2541 * 64 + 192, 0, CAPACITY - 64) and got[1][3] == 0


def test_row_g_tile_order(ask):
    # nothing else staged: fitting alone decides, and 40 960 tiles are the capacity exactly
    got = check_plans(ask, [(8, LEAN, False, t, order, counts(slots=25, materials=4)) for t, order in ((40960, True), (40961, True), (40960, False), (15, True))])
    assert got == [(CAPACITY, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (60, 0, 0, 0, 1, 0)]
    # residency: a program of 1 600 B (22 slots + 4 materials) is held 102 times by a CU; with 15 tiles behind it, 98 times
    n = counts(slots=22, materials=4)
    assert ref_base(8, LEAN, True, n)[0] == 1600
    got = check_plans(ask, [(8, LEAN, True, t, True, n) for t in (1, 2, 15)])
    assert got == [(1604, 0, 0, 0, 1, 1600), (1600, 0, 0, 0, 0, 1600), (1600, 0, 0, 0, 0, 1600)]       # 163 840 / 1 604 = 102, / 1 608 = 101
    # 31 slots + 1 material = 2 032 B: 80 workgroups up to 2 048 B exactly (4 tiles), 79 beyond
    n = counts(slots=31, materials=1)
    got = check_plans(ask, [(8, LEAN, True, t, True, n) for t in (4, 5)])
    assert got == [(2048, 0, 0, 0, 1, 2032), (2032, 0, 0, 0, 0, 2032)]
    # a program that takes more than half the capacity holds one workgroup with or without the order: fitting decides again
    for real, rec in ((8, 64), (4, 32)):
        slots = 90000 // rec
        base = slots * rec + 2 * record_sizes(real)["material"]
        t_max = last_true(lambda k: align16(base) + 4 * k <= CAPACITY)
        got = check_plans(ask, [(real, LEAN, True, t, True, counts(slots=slots, materials=2)) for t in (t_max, t_max + 1)])
        assert got[0] == (CAPACITY, 0, 0, 0, 1, align16(base)) and got[1] == (base, 0, 0, 0, 0, align16(base))
    # behind chains whose end is not a multiple of 16 (f32: 68-byte records)
    got = check_plans(ask, [(4, QUADBOX, True, 15, True, counts(slots=2000, materials=5, chains=3))])
    assert got[0] == (align16(64160 + 204) + 60, 0, 0, 64160, 1, align16(64160 + 204))
