"""GPU tests (-m gpu) of the LDS staging plan (csrc/rtk_lds_plan.h; DESIGN.md, "The LDS staging plan") at its size limits:
for every row a-g of that table a pair of scenes that differ in one integer parameter -- the last one that takes the staged
branch and the first one that does not -- found by a bisection over that parameter on the device (uploads are cheap), never
from a count worked out here.  What a launch staged is read from the `[rtk] lds plan:` line that RTK_DEBUG makes launch_one
print, what an upload built from the upload's own RTK_DEBUG lines, the kernel from rtk_kernel_name.

Every side of every pair must
  * be the kernel and the plan the row expects, the two sides differing in the decision under test only, and the staged side
    lie within one record (the thing the parameter adds: a slot, a unit record, a MaterialRec, a PerlinRec, a ChainRec, a
    BoxRec with its share of the kind and rank words) of its limit;
  * equal, bit for bit in linear and rgb8, the same scene rendered by the all-in-memory twin of its kernel (variant bit 0 for a
    staged program, bit 21 for a box table or a hot part; the matrix relies on the same identities);
  * in f64, equal the CPU oracle on the same description: rgb8 equal, linear within test_gpu_parity's F64_RMSE_BOUND.

Fast-order scenes are uploaded with rtk_scene_upload_optimized as the hierarchy they already are -- flat lists, or a BVH whose
boxes were grown here -- because rtk_scene_optimize chooses its hierarchy BY the LDS budget and so never leaves a program within
a record of the limit; the oracle then executes the same description, whose visiting order is the kernels'.  The MIXED and
COMPACT programs and the hot/cold form exist in f64 only, so those pairs have no f32 side.

The frame is tests/kernel_matrix.py's: 37 x 21 (5 x 3 ragged tiles), 3 spp, depth 8."""
import collections
import random
import re

import numpy as np
import pytest

from tests import kernel_matrix as km
from tests.desc_builder import NODE_BVH, Aabb, DescBuilder, _union
from tests.scene_cases import RENDER_SEED
from tests.test_gpu_parity import F64_RMSE_BOUND, rmse
from tests.test_view_batch import assert_views_are_their_frames, five_views

pytestmark = pytest.mark.gpu

CAPACITY = 160 * 1024
REF, OPT = "reference", "optimized"
F64, F32 = km.F64, km.F32
BOX_REC = {F64: 56, F32: 32}
MATERIAL_REC = {F64: 48, F32: 32}
PERLIN_REC = {F64: 9216, F32: 6144}
CHAIN_REC = {F64: 120, F32: 68}
DEPTH = km.CUSTOM_DEPTH

Launch = collections.namedtuple("Launch", "real feat in_lds views total mats perlin chains order_in_lds order")
_PLAN = re.compile(r"\[rtk\] lds plan: real (\d) FEAT (\d+) IN_LDS (\d) views (\d): total (\d+) B, mats_lds_offset (\d+), perlin_lds_offset (\d+), "
                   r"chains_lds_offset (\d+), order_in_lds (\d), order_lds_offset (\d+)")
_BOX_TABLE = re.compile(r"\[rtk\] (\d)-byte reals: (\d+) slots, (\d+) box slots, boxes \+ tables (\d+) B")
_HOT = re.compile(r"\[rtk\] COMPACT program (\d+) B; hot part (\d+) B, cold part (\d+) B")


def launches(err):
    return [Launch(F64 if m.group(1) == "8" else F32, *(int(g) for g in m.groups()[1:])) for m in _PLAN.finditer(err)]


class Rig:
    """One Renderer, the matrix's camera, and the capture of what the library prints."""

    def __init__(self, rt, orc, renderer, capfd):
        self.rt, self.orc, self.renderer, self.capfd = rt, orc, renderer, capfd
        self.view = rt.Scene.build("three_spheres")              # its camera: at the origin, looking down -z
        self.cam = self.view.camera(km.WIDTH, km.HEIGHT, km.SPP, DEPTH)
        self.said = []

    def say(self, *what):
        """For the test's report: printed when the test ends (what is printed meanwhile, the next capture read would swallow)."""
        self.said.append(" ".join(str(w) for w in what))

    def mode(self, real):
        return self.rt.RTK_REAL_F64 if real == F64 else self.rt.RTK_REAL_F32

    def upload(self, scene, order):
        """-> what the upload printed"""
        self.capfd.readouterr()
        if order == REF:
            self.renderer.upload(scene)
        else:
            self.renderer.upload_optimized(scene, self.cam.center)
        return self.capfd.readouterr().err

    def name(self, real, variant=0):
        return self.renderer.kernel_name(self.mode(real), variant)

    def frame(self, real, variant=0, cam=None):
        """-> linear, rgb8, the launches' plans"""
        self.capfd.readouterr()
        img, img8, _ = self.renderer.render_host(cam or self.cam, seed=RENDER_SEED, real_mode=self.mode(real), variant=variant)
        got = launches(self.capfd.readouterr().err)
        assert got and all(g.real == real and g.views == 0 for g in got), got
        return img, img8, got

    def first_plan(self, scene, order, real):
        """The plan of the first frame after an upload: no tile order is known yet, so none is staged."""
        self.upload(scene, order)
        return self.frame(real)[2][0]

    def check_side(self, scene, order, real, feat, in_lds, twin):
        """Upload, name, first frame and its plan; the all-in-memory twin; the oracle in f64.  -> (upload's output, plan)"""
        up = self.upload(scene, order)
        assert self.name(real) == km.kernel_name((real, feat, False, in_lds))
        img, img8, got = self.frame(real)
        assert len(got) == 1 and (got[0].feat, got[0].in_lds, got[0].order_in_lds) == (feat, int(in_lds), 0), got
        assert np.isfinite(img).all()
        twin_img, twin_img8, twin_got = self.frame(real, twin)
        assert all(not g.in_lds and not g.feat & 1024 and g.mats == g.perlin == g.chains == 0 for g in twin_got), twin_got
        assert np.array_equal(img, twin_img) and np.array_equal(img8, twin_img8), float(np.abs(img - twin_img).max())
        if real == F64:
            ref, ref8, _ = self.orc.render(scene.desc_ptr, self.cam, RENDER_SEED, 8)
            self.say(f"{order} {real} FEAT {feat} IN_LDS {int(in_lds)}: rmse against the oracle {rmse(img, ref):.3e}, plan {got[0]}")
            assert np.array_equal(img8, ref8) and rmse(img, ref) < F64_RMSE_BOUND
        else:
            self.say(f"{order} {real} FEAT {feat} IN_LDS {int(in_lds)}: plan {got[0]}")
        return up, got[0]


@pytest.fixture(scope="module")
def module_renderer(rt):
    renderer = rt.Renderer(0)     # its own context: a learned tile order belongs to a context
    yield renderer
    renderer.close()


@pytest.fixture
def rig(rt, orc, module_renderer, capfd, monkeypatch):
    monkeypatch.setenv("RTK_DEBUG", "1")
    rig = Rig(rt, orc, module_renderer, capfd)
    yield rig
    print("\n".join(rig.said))


def last_staged(staged, lo, hi):
    """The largest k in [lo, hi) with staged(k), for a staged() that holds up to some k and fails beyond it; both ends are checked,
    so a pair that cannot be shown fails here."""
    assert staged(lo), f"not staged at {lo}"
    assert not staged(hi), f"still staged at {hi}"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if staged(mid) else (lo, mid)
    return lo


# ------------------------------------------------------------------------------------------------ scenes
def _colour(i):
    return (0.15 + 0.8 * ((i * 37) % 101) / 101.0, 0.15 + 0.8 * ((i * 11) % 53) / 53.0, 0.15 + 0.8 * ((i * 7) % 29) / 29.0)


def _materials(b, n, first=0):
    """n materials of distinct colours: lambertians, every fifth a metal (so no scene here is F_MATTE)."""
    return [b.metal(_colour(first + i), 0.1) if i % 5 == 1 else b.lambertian(_colour(first + i)) for i in range(n)]


def _sphere_field(b, n, mats, z=-6.0, radius=0.07, first=0):
    """n small spheres on a grid of 64 columns that faces the camera; sphere i wears mats[(first + i) % len(mats)]."""
    out = []
    for i in range(n):
        col, row = i % 64, i // 64
        centre = (-6.0 + 12.0 * col / 63.0, -3.0 + 0.085 * row, z - 0.16 * (row % 8))
        out.append(b.sphere(centre, radius, mats[(first + i) % len(mats)]))
    return out


def lean_scene(n_spheres, n_materials):
    """A flat list of n_spheres spheres (the ground among them) and n_materials materials, all of them in use: the lean family."""
    b = DescBuilder()
    mats = _materials(b, n_materials)
    members = [b.sphere((0.0, -100.5, -1.0), 97.0, mats[0])] + _sphere_field(b, n_spheres - 1, mats, first=1)
    return b.finish(b.list(members))


def _triangle_field(b, n, mats, rnd, size=0.3):
    out = []
    for i in range(n):
        c = (rnd.uniform(-3.5, 3.5), rnd.uniform(-0.9, 2.5), rnd.uniform(-8.0, -3.0))
        u = (rnd.uniform(0.4, 1.0) * size, rnd.uniform(-0.3, 0.3) * size, rnd.uniform(-0.4, 0.4) * size)
        v = (rnd.uniform(-0.3, 0.3) * size, rnd.uniform(0.4, 1.0) * size, rnd.uniform(-0.4, 0.4) * size)
        out.append(b.triangle(c, tuple(c[k] + u[k] for k in range(3)), tuple(c[k] + v[k] for k in range(3)), mats[i % len(mats)]))
    return out


def _bvh_pair(b, left, right):
    """One more bvh_node over two nodes with known boxes: exactly one box more."""
    box = _union([b.box_of[left], b.box_of[right]])
    b.boxes.append(Aabb(*box))
    node = b._node(NODE_BVH, left, right, len(b.boxes) - 1)
    b.box_of[node] = box
    return node


def mesh_scene(n_triangles, n_materials, extra=0):
    """kernel_matrix._mesh_metal with n_materials materials of distinct colours on its triangles (triangle i wears material
    i % n_materials, so every one is on geometry the camera sees while n_materials <= n_triangles), and `extra` more triangles,
    each under a bvh_node of its own on top of the tree: one box per extra triangle."""
    rnd = random.Random(20251017)
    b = DescBuilder()
    mats = _materials(b, n_materials)
    members = [b.sphere((0, -101, -5), 100.0, b.lambertian((0.5, 0.5, 0.5))), b.sphere((2.5, 4.0, -3.0), 1.5, b.light((10.0, 10.0, 9.0))),
               b.sphere((0.0, 0.0, -4.0), 0.7, b.metal((0.8, 0.7, 0.6), 0.1))]
    tris = _triangle_field(b, n_triangles + extra, mats, rnd)
    root = b.bvh(members + tris[:n_triangles], random.Random(7))
    for t in tris[n_triangles:]:
        root = _bvh_pair(b, t, root)
    return b.finish(b.list([root]))


def _grow_boxes(b, by=1e-3):
    """Boxes with a margin of their own, for descriptions handed to rtk_scene_upload_optimized (its kernels use the fused slab test
    and f32 culling boxes, which rtk_scene_optimize's margin normally pays for)."""
    for box in b.boxes:
        box.xmin, box.ymin, box.zmin = box.xmin - by, box.ymin - by, box.zmin - by
        box.xmax, box.ymax, box.zmax = box.xmax + by, box.ymax + by, box.zmax + by


def _noise_spheres(b, n, rnd, z=-2.6):
    """n spheres the camera sees, each with a noise texture -- a Perlin table -- of its own."""
    out = []
    for i in range(n):
        col, row = i % 8, i // 8
        out.append(b.sphere((-2.8 + 0.8 * col, 1.6 - 0.75 * row, z), 0.33, b.textured(b.noise(3.0 + i, rnd))))
    return out


def flat_scene(n_spheres, n_triangles, n_noise=0, n_materials=6, bvh_triangles=False):
    """A flat list for the fast-order kernels: the ground, a light, n_spheres small spheres, n_noise noise-textured spheres (the
    full-feature family when there is one, else the mesh family) and n_triangles triangles -- these under a BVH with grown boxes
    when `bvh_triangles`."""
    rnd = random.Random(99)
    b = DescBuilder()
    mats = _materials(b, n_materials)
    members = [b.sphere((0, -101, -5), 100.0, mats[0]), b.sphere((2.5, 4.0, -3.0), 1.5, b.light((10.0, 10.0, 9.0)))]
    members += _noise_spheres(b, n_noise, rnd)
    members += _sphere_field(b, n_spheres, mats, z=-7.0)
    tris = _triangle_field(b, n_triangles, mats, rnd)
    if bvh_triangles:
        members.append(b.bvh(tris, random.Random(7)))
        _grow_boxes(b)
    else:
        members += tris
    return b.finish(b.list(members))


def split_noise_scene(n_noise, real):
    """Reference order, full-feature family (F_TEXTURE), a slot program larger than LDS in `real` whose box table leaves room for
    some Perlin tables: a BVH over spheres, n_noise of them noise-textured and in front."""
    rnd = random.Random(5)
    b = DescBuilder()
    mats = _materials(b, 6)
    members = [b.sphere((0, -101, -5), 100.0, mats[0]), b.sphere((2.5, 4.0, -3.0), 1.5, b.light((10.0, 10.0, 9.0)))]
    members += _noise_spheres(b, n_noise, rnd)
    members += _sphere_field(b, 1500 if real == F64 else 2800, mats, z=-7.0)
    return b.finish(b.list([b.bvh(members, random.Random(7))]))


def _box_sides(b, mat, h=0.22):
    x0, y0, z0, x1, y1, z1 = -h, -h, -h, h, h, h                       # box(a, b): six quads (quad.h:71-90), around the origin
    dx, dy, dz = (x1 - x0, 0, 0), (0, y1 - y0, 0), (0, 0, z1 - z0)
    return [b.quad((x0, y0, z1), dx, dy, mat), b.quad((x1, y0, z1), (0, 0, -dz[2]), dy, mat), b.quad((x1, y0, z0), (-dx[0], 0, 0), dy, mat),
            b.quad((x0, y0, z0), dz, dy, mat), b.quad((x0, y1, z1), dx, (0, 0, -dz[2]), mat), b.quad((x0, y0, z0), dx, dz, mat)]


def instance_scene(n_transforms, real=None):
    """Box instances in view, each with an angle and an offset of its own: n_transforms // 2 of translate(rotate_y(box)) and, when
    n_transforms is odd, one translate(box) -- every transform node adds one chain record.  With `real` the scene also has a BVH
    of spheres too large for LDS in that type and a triangle: the full-feature family with a box table (F_LDS_BOXES)."""
    b = DescBuilder()
    mats = _materials(b, 7)
    members = [b.sphere((0, -101, -5), 100.0, mats[0]), b.quad((-1, 4.5, -6), (2, 0, 0), (0, 0, 2), b.light((9.0, 9.0, 8.0)))]
    for i in range((n_transforms + 1) // 2):
        offset = (-4.5 + 1.0 * (i % 10) + 0.03 * i, -0.6 + 0.75 * (i // 10), -6.0 - 0.05 * (i % 7))
        box = b.list(_box_sides(b, mats[i % 7]))
        single = n_transforms % 2 == 1 and i == n_transforms // 2
        members.append(b.translate(box if single else b.rotate_y(box, 7.0 + 5.0 * i), offset))
    if real is not None:
        members.append(b.triangle((-1.0, 2.6, -4.0), (1.0, 2.6, -4.0), (0.0, 3.4, -4.2), mats[2]))
        field = _sphere_field(b, 1400 if real == F64 else 2800, mats, z=-8.0)
        members.append(b.bvh(field, random.Random(7)))
    return b.finish(b.list(members))


# ------------------------------------------------------------------------------------------------ (a) the whole program
# order, real, FEAT, bytes one more sphere adds, a material count, a material count with which program + materials can be 163 840 exactly
ROW_A = [(REF, F64, 0, 64, 3, 4), (REF, F32, 0, 32, 3, 3), (OPT, F64, 256, 64, 3, 2)]


def _find_whole_program(rig, order, real, n_materials):
    def staged(n):
        rig.upload(lean_scene(n, n_materials), order)
        return rig.name(real).endswith("true>")
    return last_staged(staged, 1000, 6000)


@pytest.mark.parametrize("order,real,feat,record,n_materials,n_exact", ROW_A, ids=[f"{r[0]}-{r[1]}" for r in ROW_A])
def test_a_whole_program_at_the_capacity(rig, order, real, feat, record, n_materials, n_exact):
    n = _find_whole_program(rig, order, real, n_materials)
    _, fit = rig.check_side(lean_scene(n, n_materials), order, real, feat, True, km.V_GLOBAL)
    _, over = rig.check_side(lean_scene(n + 1, n_materials), order, real, feat, False, km.V_GLOBAL)
    rig.say("(a)", order, real, "spheres", n, "staged", fit, "| not staged", over)
    assert CAPACITY - record < fit.total <= CAPACITY
    assert fit[5:] == (0, 0, 0, 0, fit.total) and over[4:] == (0, 0, 0, 0, 0, 0)
    # the exact fit: the first launches that ask for every byte of a CU's LDS
    n = n if n_exact == n_materials else _find_whole_program(rig, order, real, n_exact)
    scene = lean_scene(n, n_exact)
    _, exact = rig.check_side(scene, order, real, feat, True, km.V_GLOBAL)
    assert exact.total == CAPACITY and exact.order == CAPACITY
    rig.say("(a)", order, real, "spheres", n, "materials", n_exact, "exact fit", exact)
    # ... a second frame, whose learned order finds no room; and a batch of three unlike views, which shares the plan
    _, _, again = rig.frame(real)
    assert [(g.total, g.order_in_lds) for g in again] == [(CAPACITY, 0)]
    cams, seeds = five_views(rig.rt, rig.cam)
    rig.capfd.readouterr()
    assert_views_are_their_frames(rig.renderer, cams[:3], seeds[:3], rig.mode(real))
    batch = [g for g in launches(rig.capfd.readouterr().err) if g.views]
    assert batch and all((g.feat, g.in_lds, g.total, g.order_in_lds) == (feat, 1, CAPACITY, 0) for g in batch), batch
    rig.say("(a) view batch", batch[0])


# ------------------------------------------------------------------------------------------------ (b) COMPACT, hot/cold, slots
def test_b_mesh_family_compact_program_or_the_slot_program(rig):
    def staged(n):
        rig.upload(flat_scene(n, 1900), OPT)
        return rig.name(F64) == km.kernel_name((F64, 66 | 256, False, True))
    n = last_staged(staged, 10, 1200)
    _, fit = rig.check_side(flat_scene(n, 1900), OPT, F64, 66 | 256, True, km.V_GLOBAL)
    _, over = rig.check_side(flat_scene(n + 1, 1900), OPT, F64, 66 | 128, False, km.V_GLOBAL)      # the slot program, in memory (a flat list has no boxes)
    rig.say("(b) mesh", n, fit, over)
    assert CAPACITY - 48 < fit.total <= CAPACITY and over.total == 0                               # a sphere is three 16-byte units
    assert rig.name(F64, km.V_SLOT) == km.kernel_name((F64, 66 | 128, False, False))


def test_b_full_family_compact_program_or_its_hot_cold_form(rig):
    def staged(n):
        rig.upload(flat_scene(n, 1900, n_noise=1), OPT)
        return rig.name(F64) == km.kernel_name((F64, 127 | 256, False, True))
    n = last_staged(staged, 10, 1200)
    up, fit = rig.check_side(flat_scene(n, 1900, n_noise=1), OPT, F64, 127 | 256, True, km.V_GLOBAL)
    up_over, over = rig.check_side(flat_scene(n + 1, 1900, n_noise=1), OPT, F64, 127 | 256 | 1024, False, km.V_NO_LDS_BOXES)
    rig.say("(b) full", n, fit, over)
    assert CAPACITY - 48 < fit.total <= CAPACITY
    compact, hot, _ = (int(x) for x in _HOT.search(up_over).groups())
    n_materials = (fit.total - int(_HOT.search(up).group(1))) // 48
    assert compact + 48 * n_materials == fit.total + 48 > CAPACITY
    # the hot part, the materials right behind it (no offset of their own), the one Perlin table behind them
    assert over.mats == 0 and over.perlin == hot + 48 * n_materials and over.total == over.perlin + 9216


def test_b_hot_part_at_the_capacity_or_the_slot_program_with_a_box_table(rig):
    def staged(n):
        rig.upload(flat_scene(n, 300, n_noise=1, bvh_triangles=True), OPT)
        return rig.name(F64) != km.kernel_name((F64, 127 | 128 | 1024, False, False))      # the whole COMPACT program in LDS, then its hot part
    n = last_staged(staged, 2000, 4500)
    up, fit = rig.check_side(flat_scene(n, 300, n_noise=1, bvh_triangles=True), OPT, F64, 127 | 256 | 1024, False, km.V_NO_LDS_BOXES)
    up_over, over = rig.check_side(flat_scene(n + 1, 300, n_noise=1, bvh_triangles=True), OPT, F64, 127 | 128 | 1024, False, km.V_NO_LDS_BOXES)
    rig.say("(b) hot", n, fit, over)
    assert CAPACITY - 48 < fit.total + 64 <= CAPACITY and fit[5:9] == (0, 0, 0, 0)                  # hot part + materials; no room behind them
    assert int(_HOT.search(up).group(2)) < fit.total and int(_HOT.search(up_over).group(2)) - int(_HOT.search(up).group(2)) == 48
    table = int(_BOX_TABLE.search(up_over).group(4))                                               # the slot program's box table, and room to spare
    assert over.mats == (table + 15) // 16 * 16 and over.perlin > over.mats and over.total == over.perlin + 9216


# ------------------------------------------------------------------------------------------------ (c) the box table at upload
def _first_tree_over(rig, real, target):
    """The smallest triangle count whose box table (the upload's own figure) exceeds `target` bytes."""
    def table(n):
        m = [m for m in _BOX_TABLE.finditer(rig.upload(mesh_scene(n, 3), REF)) if int(m.group(1)) == (8 if real == F64 else 4)]
        return int(m[0].group(4)) if m else 0
    return last_staged(lambda n: table(n) <= target, 100, 7000) + 1


@pytest.mark.parametrize("real", (F64, F32))
def test_c_box_table_built_or_not(rig, real):
    n = _first_tree_over(rig, real, CAPACITY - 64 - 4000)

    def staged(extra):
        rig.upload(mesh_scene(n, 3, extra), REF)
        return rig.name(real) == km.kernel_name((real, 66 | 1024, False, False))
    extra = last_staged(staged, 0, 200)
    up, fit = rig.check_side(mesh_scene(n, 3, extra), REF, real, 66 | 1024, False, km.V_NO_LDS_BOXES)
    up_over, over = rig.check_side(mesh_scene(n, 3, extra + 1), REF, real, 66, False, km.V_NO_LDS_BOXES)
    tables = [[int(m.group(4)) for m in _BOX_TABLE.finditer(u) if int(m.group(1)) == (8 if real == F64 else 4)][0] for u in (up, up_over)]
    rig.say("(c)", real, "triangles", n, "+", extra, "box tables", tables, fit, over)
    # one more triangle: one more box record and at most 8 bytes each of kind and rank words
    assert tables[0] + 64 <= CAPACITY < tables[1] + 64 and BOX_REC[real] <= tables[1] - tables[0] <= BOX_REC[real] + 16
    assert fit.total == tables[0] and fit[5:9] == (0, 0, 0, 0)        # no room for the six materials behind it
    assert over[4:] == (0, 0, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ (d) materials behind the boxes
@pytest.mark.parametrize("real", (F64, F32))
def test_d_material_table_of_16_kib(rig, real):
    feat, rec = 66 | 1024, MATERIAL_REC[real]
    m = last_staged(lambda m: rig.first_plan(mesh_scene(km.N_LARGE_TRIANGLES, m), REF, real).mats > 0, 3, 700)
    _, fit = rig.check_side(mesh_scene(km.N_LARGE_TRIANGLES, m), REF, real, feat, False, km.V_NO_LDS_BOXES)
    _, over = rig.check_side(mesh_scene(km.N_LARGE_TRIANGLES, m + 1), REF, real, feat, False, km.V_NO_LDS_BOXES)
    rig.say("(d) 16 KiB", real, "materials", m, "+ 3", fit, over)
    assert fit.mats > 0 and fit.mats % 16 == 0 and 16384 - rec < fit.total - fit.mats <= 16384 and fit.total - fit.mats == (m + 3) * rec
    assert over.mats == 0 and over.total <= fit.mats and fit.mats - over.total < 16           # the same box table, nothing behind it, and room for more
    assert over.total + (m + 4) * rec + 64 + 16 <= CAPACITY
    assert (fit.perlin, fit.chains, over.perlin, over.chains) == (0, 0, 0, 0)


@pytest.mark.parametrize("real", (F64, F32))
def test_d_small_material_table_without_room(rig, real):
    feat, rec = 66 | 1024, MATERIAL_REC[real]
    n = _first_tree_over(rig, real, CAPACITY - 64 - 9000)            # room for fewer than 9 000 B of materials: under 16 KiB on both sides
    m = last_staged(lambda m: rig.first_plan(mesh_scene(n, m), REF, real).mats > 0, 3, 400)
    _, fit = rig.check_side(mesh_scene(n, m), REF, real, feat, False, km.V_NO_LDS_BOXES)
    _, over = rig.check_side(mesh_scene(n, m + 1), REF, real, feat, False, km.V_NO_LDS_BOXES)
    rig.say("(d) no room", real, "triangles", n, "materials", m, "+ 3", fit, over)
    assert (m + 4) * rec <= 16384
    assert fit.mats > 0 and fit.total - fit.mats == (m + 3) * rec and CAPACITY - rec < fit.total + 64 <= CAPACITY
    assert over.mats == 0 and (over.total + 15) // 16 * 16 == fit.mats


# ------------------------------------------------------------------------------------------------ (e) Perlin tables
@pytest.mark.parametrize("real", (F64, F32))
def test_e_perlin_tables_behind_a_box_table(rig, real):
    feat, rec = 127 | 1024, PERLIN_REC[real]
    p = last_staged(lambda p: rig.first_plan(split_noise_scene(p, real), REF, real).perlin > 0, 1, 24)
    _, fit = rig.check_side(split_noise_scene(p, real), REF, real, feat, False, km.V_NO_LDS_BOXES)
    _, over = rig.check_side(split_noise_scene(p + 1, real), REF, real, feat, False, km.V_NO_LDS_BOXES)
    rig.say("(e) SPLIT", real, "noise textures", p, fit, over)
    assert fit.mats > 0 and fit.perlin > fit.mats and fit.total == fit.perlin + p * rec and CAPACITY - rec < fit.total + 64 <= CAPACITY
    assert over.mats > 0 and over.perlin == 0 and over.chains == fit.chains == 0
    assert over.total + (p + 1) * rec + 64 > CAPACITY


def test_e_perlin_tables_behind_a_hot_part(rig):
    feat = 127 | 256 | 1024
    p = last_staged(lambda p: rig.first_plan(flat_scene(1200, 2200, n_noise=p), OPT, F64).perlin > 0, 1, 24)
    _, fit = rig.check_side(flat_scene(1200, 2200, n_noise=p), OPT, F64, feat, False, km.V_NO_LDS_BOXES)
    _, over = rig.check_side(flat_scene(1200, 2200, n_noise=p + 1), OPT, F64, feat, False, km.V_NO_LDS_BOXES)
    rig.say("(e) COLD", "noise textures", p, fit, over)
    assert fit.mats == 0 and fit.perlin % 16 == 0 and fit.total == fit.perlin + p * 9216 and CAPACITY - 9216 < fit.total + 64 <= CAPACITY
    assert over.mats == 0 and over.perlin == 0 and over.total + (p + 1) * 9216 + 64 > CAPACITY


# ------------------------------------------------------------------------------------------------ (f) instance chains
@pytest.mark.parametrize("real", (F64, F32))
@pytest.mark.parametrize("boxes", (False, True), ids=("program-in-lds", "box-table"))
def test_f_instance_chains_of_8_kib(rig, real, boxes):
    feat, in_lds, twin = (127 | 1024, False, km.V_NO_LDS_BOXES) if boxes else (69, True, km.V_GLOBAL)
    with_real = real if boxes else None
    rec = CHAIN_REC[real]
    _, none = rig.check_side(instance_scene(0, with_real), REF, real, feat, in_lds, twin)       # one chain, world space: nothing to stage
    assert none.chains == 0
    _, two = rig.check_side(instance_scene(4, with_real), REF, real, feat, in_lds, twin)        # two instances: 1 + 4 chains
    assert two.chains > 0 and two.chains % 16 == 0 and two.total == two.chains + 5 * rec
    j = last_staged(lambda j: rig.first_plan(instance_scene(j, with_real), REF, real).chains > 0, 4, 160)
    _, fit = rig.check_side(instance_scene(j, with_real), REF, real, feat, in_lds, twin)
    scene_over = instance_scene(j + 1, with_real)
    _, over = rig.check_side(scene_over, REF, real, feat, in_lds, twin)
    rig.say("(f)", real, "box table" if boxes else "program in LDS", "transform nodes", j, fit, over)
    assert fit.chains > 0 and fit.chains % 16 == 0 and fit.total == fit.chains + (j + 1) * rec and 8192 - rec < (j + 1) * rec <= 8192
    assert over.chains == 0 and (j + 2) * rec > 8192 and over.total + 16 + (j + 2) * rec + 64 <= CAPACITY      # 8 KiB decided, not the room
    assert (fit.mats > 0) == (over.mats > 0) == boxes and fit.perlin == over.perlin == 0
    if not boxes:     # the K + 1 instances scene as a batch of three unlike views: the same plan, no tile order
        cams, seeds = five_views(rig.rt, rig.cam)
        rig.capfd.readouterr()
        assert_views_are_their_frames(rig.renderer, cams[:3], seeds[:3], rig.mode(real))
        batch = [g for g in launches(rig.capfd.readouterr().err) if g.views]
        assert batch and all((g.feat, g.in_lds, g.total, g.chains, g.order_in_lds) == (feat, 1, over.total, 0, 0) for g in batch), batch


# ------------------------------------------------------------------------------------------------ (g) the tile order
def _second_frame_against_fixed_order(rig, real, variant, cam):
    rig.frame(real, variant, cam)                                       # the first frame of a shape learns the order
    img, img8, got = rig.frame(real, variant, cam)
    fixed, fixed8, got_fixed = rig.frame(real, variant | 4, cam)
    assert np.array_equal(img, fixed) and np.array_equal(img8, fixed8)
    assert all(g.order_in_lds == 0 for g in got_fixed)
    assert len(got) == 1
    return got[0], got_fixed[0]


@pytest.mark.parametrize("height,staged", ((1280, True), (1288, False)))
def test_g_tile_order_with_nothing_else_in_lds(rig, height, staged):
    rig.upload(rig.view, REF)
    cam = rig.view.camera(2048, height, 1, 2)
    plan, fixed = _second_frame_against_fixed_order(rig, F64, km.V_GLOBAL, cam)
    tiles = 256 * (height // 8)
    rig.say("(g) lds == 0:", tiles, "tiles", plan)
    assert (plan.feat, plan.in_lds, plan.order) == (0, 0, 0) and fixed.total == 0
    assert (plan.order_in_lds, plan.total) == ((1, CAPACITY) if staged else (0, 0)) and (4 * tiles <= CAPACITY) == staged
    assert 4 * tiles == CAPACITY or not staged                          # 40 960 tiles are the capacity exactly; 41 216 the next frame height's


@pytest.mark.parametrize("real", (F64, F32))
def test_g_tile_order_never_costs_a_resident_workgroup(rig, real):
    order_bytes = 4 * 15
    # three_spheres: 102 workgroups' worth of program per CU in f64 -- 98 with the order behind it: not staged
    rig.upload(rig.view, REF)
    plan, fixed = _second_frame_against_fixed_order(rig, real, 0, rig.cam)
    rig.say("(g) residency, three_spheres", real, plan)
    assert plan.in_lds == 1 and plan.order_in_lds == 0 and plan.total == fixed.total and plan.order == (plan.total + 15) // 16 * 16
    assert CAPACITY // plan.total != CAPACITY // (plan.order + order_bytes)
    # a program whose count per CU the 60 bytes leave alone: staged.  The largest such program of at most 200 spheres.
    def staged(n):
        rig.upload(lean_scene(n, 3), REF)
        rig.frame(real)
        return rig.frame(real)[2][0].order_in_lds == 1
    n = next(n for n in range(200, 20, -1) if staged(n))
    rig.upload(lean_scene(n, 3), REF)
    plan, fixed = _second_frame_against_fixed_order(rig, real, 0, rig.cam)
    rig.say("(g) residency, spheres", n, real, plan)
    assert plan.in_lds == 1 and plan.order_in_lds == 1 and plan.order == (fixed.total + 15) // 16 * 16 and plan.total == plan.order + order_bytes
    assert CAPACITY // fixed.total == CAPACITY // plan.total
