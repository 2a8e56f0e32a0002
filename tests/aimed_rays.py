"""Scenes built around a camera's primary rays (CPU only), so that the float culling tests of the fast order's render kernels
decide rays that meet a primitive at a corner, an edge, a seam or inside a thin box.

A camera's sample-0 rays are known exactly on the CPU (orc_kat_get_ray; the device's get_ray is pinned to it bit for bit), so
every pixel's ray gets ONE primitive of its own, placed at P = o + s d of that ray: s d is 0.8 .. 1.2 of |lookfrom - lookat| long (DEPTH)
and the primitive is SIZE (a quarter) of the pixel's footprint there, L.  `build(rt, view, seed, family)` returns (cam, Aimed):

  desc      the ORIGINAL description: a flat DescBuilder.list (instances hold flat lists).  It has no bvh node, so the oracle on it
            performs no box test at all -- the truth that no culling can have touched;
  rays      the rays as rtk_ray records (pixel = j * width + i, sample 0, skip = get_ray's draws, tmin 0.001, tmax inf);
  rung      per ray, the index into LADDER (quads, triangles: the offset from the corner / edge in units of the primitive's edge
            vectors) or into SPHERE_LADDER (spheres: the radius in units of L);
  kind      per ray, the index into KINDS[family];
  own       per ray, the material indices of its own target (one, or two for a seam), -1 where there is none: every primitive has
            a lambertian of its own random colour, so the material of a hit names the primitive.  The colours are sixteenths and
            the background is dyadic too: a path's colour, albedo x albedo x background, is then an exact product in whatever order
            it is formed -- the oracle multiplies recursively (a1 * (a2 * bg)), the kernels iteratively ((a1 * a2) * bg), which on
            arbitrary colours differs in the last place (the 1e-17 of tests/test_gpu_parity.py) and has nothing to do with culling;
  instance  per ray, the instance that holds its target (-1: top level).

Families (each selects its kernel family in the fast order, FAMILY_FEAT):
  spheres    lean MIXED.  A sphere centred on the ray ("centre") or 0.9 r off it ("off_centre"), radius L * SPHERE_LADDER[rung];
             half of them move (_plan), with center0 = P - time * motion for the ray's own time.
  quads      quad/box COMPACT, min/max records.  "corner": a rotated quad with P at (r, r) of (Q, u, v), r = LADDER[rung];
             "axis_corner" / "axis_edge" / "axis_centre": an axis-aligned quad -- its box is 1e-4 thick -- with P at (r, r),
             (0.5, r), (0.5, 0.5); "seam": two coplanar quads sharing an edge, P at (1 - r, 0.5) or (1 + r, 0.5) of the first.  A third
             of the targets sit inside translate(rotate_y(list)) instances and are constructed in OBJECT space, around the ray as
             translate::hit and rotate_y::hit transform it; the offsets alternate between a small one and one most of the way to
             the camera, so that object-space origins lie both far from and close to the instances' content.  (Whether an
             object-space origin leaves [-extent, extent]^3 is not checked: scene_extent (rtk_api.cpp) adds four times the
             largest offset to the extent, which keeps most of them inside.)
  triangles  mesh COMPACT, centre / half-extent records.  "vertex" (r, r), "edge" (0.5, r), "interior" (0.3, 0.3) of (p0, p1 - p0,
             p2 - p0); three small spheres beside the frustum make the family's mix.
  full       the quads scene plus one noise-textured sphere, one fog ball and one triangle beside the frustum: the same targets under
             the full-feature COMPACT kernel.
  mesh_spheres  the spheres family's targets plus three triangles beside the frustum: the mesh COMPACT kernel again, but on boxes
             that carry nothing beyond the float budget -- rtk_scene_optimize grows a triangle's box by 2^-20 of the scene's extent
             for the float determinant of triangle::hit, more than the culling budgets together; a sphere's only by 2^-40.

Rungs 0 .. 2 (r <= 2^-48) are the rounding coin-flip -- the ray is AT the corner to f64 precision and the oracle's primitive test
accepts about half of them; _plan gives them enough rays that both outcomes are well populated.  In the quads family every other
target is aimed at the FAR corner / edge, (1 - r) instead of r, and so at the upper planes of its box.

CAMERAS names the views (VIEWS); `origins(rt, seed, family)` puts sixteen 8 x 8 cameras around one cloud in which each
camera's 64 rays have targets of their own."""
import ctypes as C
import math
import random

import numpy as np

from oracle import orc
from tests.desc_builder import DescBuilder

LADDER = (0.0, 2.0 ** -52, 2.0 ** -48, 2.0 ** -44, 2.0 ** -40, 2.0 ** -36, 2.0 ** -30, 2.0 ** -24, 2.0 ** -20, 2.0 ** -12, 0.5)
SPHERE_LADDER = tuple(2.0 ** -(8 + 3 * q) for q in range(11))
COIN_RUNGS = (0, 1, 2)                          # r <= 2^-48
# the share of the targets on each coin-flip rung (quads: all of them rotated corners; triangles: vertices and edges in turn, and
# most at 2^-48, which a ray along an axis -- small coordinates, a finer grid -- already resolves four times out of five)
COIN_SHARE = {"quads": (0.16, 0.16, 0.18), "full": (0.16, 0.16, 0.18), "triangles": (0.12, 0.12, 0.22)}
CENTRE_RUNG = 10                                # "axis_centre" and "interior" have no offset: filed under r = 0.5
KINDS = {"spheres": ("centre", "off_centre"),
         "quads": ("corner", "axis_corner", "axis_edge", "axis_centre", "seam"),
         "triangles": ("vertex", "edge", "interior")}
KINDS["full"] = KINDS["quads"]
KINDS["mesh_spheres"] = KINDS["spheres"]
FAMILIES = ("spheres", "quads", "triangles", "full", "mesh_spheres")
# rtk_device_layout.h feature words of the families (tests/kernel_matrix.py); every material here is a lambertian: F_MATTE 512
FAMILY_FEAT = {"spheres": 0, "quads": 69 | 512, "triangles": 66 | 512, "full": 127, "mesh_spheres": 66 | 512}
# Not 32 x 32: a COMPACT program has to fit one CU's LDS whole to be chosen at all, and the MIXED program is staged only if it fits.
# A quad is 144 B of program, a triangle 80 B, a moving sphere 96 B, a box or a list mark 32 B, and every target has a 48-byte material
# record of its own: 1 024 targets come to 160 KB or more in every family; 576 spheres or triangles and 400 quads (about 370 B a
# target, seams and instances included) stay below
FAMILY_WIDTH = {"spheres": 24, "quads": 20, "triangles": 24, "full": 20, "mesh_spheres": 24}
SIZE = 0.25
MAX_DEPTH = 3
BACKGROUND = (0.75, 0.8125, 1.0)
SEED = 7                                        # the render seed of every test on these scenes
N_INSTANCES = 8


def _camera(rt, width, lookfrom, lookat):
    cam = rt.derive_camera(width, 1.0, spp=1, max_depth=MAX_DEPTH, vfov=30.0, lookfrom=lookfrom, lookat=lookat, vup=(0.0, 1.0, 0.0), defocus_angle=0.0)
    cam.background = rt.Vec3(*BACKGROUND)
    return cam


SHIFT = (5000.0, -3000.0, 4000.0)
DEPTH = (0.8, 1.2)                                                    # of |lookfrom - lookat|, along the ray
# name -> (lookfrom, lookat, depth range).  The last two put the two shares of the float error apart: in `far_flat` every target lies
# within 2 % of the distance of the lookat point, so the central ones have boxes whose every coordinate is a tenth of |o| or less --
# the origin's share (the oi32 bracket, m2slack32, the rounding of the interval) is all that matters; in `outward` the camera sits
# beside the origin and looks at a cloud 5 400 away -- the boxes' own share is.
VIEWS = {"near": ((300.0, 200.0, 400.0), (0.0, 0.0, 0.0), DEPTH),
         "far": ((3e5, 2e5, 4e5), (0.0, 0.0, 0.0), DEPTH),            # |o| dominates every coordinate
         "axis": ((0.3, 0.2, 400.0), (0.0, 0.0, 0.0), DEPTH),         # central pixels: |d_x|, |d_y| << |d_z|, a large |o / d| on two axes
         "offset": (tuple(a + b for a, b in zip((300.0, 200.0, 400.0), SHIFT)), SHIFT, DEPTH),   # box coordinates large against box sizes
         "far_flat": ((3e5, 2e5, 4e5), (0.0, 0.0, 0.0), (0.98, 1.02)),
         "outward": ((3.0, 2.0, 4.0), (3000.0, 2000.0, 4000.0), DEPTH)}
CAMERAS = tuple(VIEWS)


def camera(rt, name, width):
    return _camera(rt, width, *VIEWS[name][:2])


def camera_rays(rt, cam, seed):
    """The sample-0 ray of every pixel, row-major, as rtk_ray records."""
    lib = orc.lib()
    w, h = cam.image_width, cam.image_height
    rays = np.zeros(w * h, rt.ray_dtype())
    out, drew = np.zeros(7), C.c_uint64()
    for j in range(h):
        for i in range(w):
            lib.orc_kat_get_ray(C.addressof(cam), seed, i, j, 0, out.ctypes.data, C.addressof(drew))
            rays[j * w + i] = (out[0:3], out[3:6], out[6], 0.001, np.inf, j * w + i, 0, drew.value, 0)
    return rays


class Aimed:
    def __init__(self, desc, rays, rung, kind, own, instance, family, ladder):
        self.desc, self.rays, self.rung, self.kind, self.own, self.instance, self.family, self.ladder = desc, rays, rung, kind, own, instance, family, ladder
        self.name = "aimed-" + family

    @property
    def desc_ptr(self):
        return self.desc.desc_ptr

    def describe(self, k):
        """Ray k for an assertion message: its rung and its target kind."""
        if self.kind[k] < 0:
            return f"ray {k}: no target"
        where = "" if self.instance[k] < 0 else f" in instance {self.instance[k]}"
        return f"ray {k}: {KINDS[self.family][self.kind[k]]} at rung {self.rung[k]} ({self.ladder[self.rung[k]]:.3g}){where}"


def _unit(v):
    return v / math.sqrt(float(v @ v))


def _frame(rnd, dn, length):
    """Two edge vectors of `length`, at 60 .. 120 degrees to each other, whose plane the ray (unit direction dn) crosses steeply."""
    while True:
        u, v = (_unit(np.array([rnd.gauss(0, 1) for _ in range(3)])) for _ in range(2))
        n = np.cross(u, v)
        if abs(float(u @ v)) < 0.5 and abs(float(_unit(n) @ dn)) > 0.4:
            return u * length, v * length


def _axis_frame(d, length):
    """Edge vectors along the two axes the ray is least aligned with: an axis-aligned quad facing the ray."""
    a = int(np.argmax(np.abs(d)))
    u, v = np.zeros(3), np.zeros(3)
    u[(a + 1) % 3], v[(a + 2) % 3] = length, length
    return u, v


def _plan(family, n):
    """(rung, kind, far, moving) of targets 0 .. n-1.  `far` (quads): the far corner / edge / side of the seam, 1 - r in place of r;
    `moving` (spheres).  Spheres walk the rungs, a kind per round, moving every other two rounds.  Quads and triangles: COIN_SHARE
    of the targets sit on each coin-flip rung, in the kinds that flip about evenly there -- an axis-aligned quad's hit point is often P
    itself, bit for bit, one side of a seam always accepts, and nothing flips in an interior -- and the rest walk the rungs from
    2^-44 up with every kind.  The whole is shuffled (by n alone), so that every part of the image holds every rung."""
    kinds = KINDS[family]
    if family in ("spheres", "mesh_spheres"):
        plan = [(k % len(SPHERE_LADDER), (k // len(SPHERE_LADDER)) % 2, False, (k // (2 * len(SPHERE_LADDER))) % 2 == 1) for k in range(n)]
    else:
        flipping = 2 if family == "triangles" else 1
        plan = [(rung, j % flipping, (j // flipping) % 2 == 1, False) for rung in COIN_RUNGS for j in range(int(round(COIN_SHARE[family][rung] * n)))]
        rungs = [r for r in range(len(LADDER)) if r not in COIN_RUNGS]
        for j in range(n - len(plan)):
            plan.append((rungs[j % len(rungs)], (j // len(rungs)) % len(kinds), (j // (len(rungs) * len(kinds))) % 2 == 1, False))
    random.Random(n).shuffle(plan)
    return plan


class _Targets:
    """One family's targets, added ray by ray to a DescBuilder."""

    def __init__(self, b, rnd, family, n_instances=N_INSTANCES, palette=0):
        self.b, self.rnd, self.family, self.palette = b, rnd, family, []
        self.palette = [self.material() for _ in range(palette)]
        self.top = []
        self.inst = [[] for _ in range(n_instances)]      # members of each instance's list, in object space
        self.inst_xf = []                                  # (degrees, offset) per instance, filled by the caller

    def material(self):
        return self.b.lambertian(tuple(self.rnd.randint(3, 15) / 16.0 for _ in range(3)))

    def object_ray(self, o, d, inst):
        """The ray in the space of instance `inst`, as translate::hit then rotate_y::hit compute it (rt_oracle.cpp)."""
        degrees, offset = self.inst_xf[inst]
        r = degrees * 3.1415926535897932385 / 180.0
        s, c = math.sin(r), math.cos(r)
        o = o - offset
        return (np.array([(c * o[0]) - (s * o[2]), o[1], (s * o[0]) + (c * o[2])]),
                np.array([(c * d[0]) - (s * d[2]), d[1], (s * d[0]) + (c * d[2])]))

    def add(self, k, o, d, time, s, length, inst):
        """Target number k, for the ray (o, d, time) at o + s d, edge length `length` -> (rung, kind, own materials)."""
        b, rnd, family = self.b, self.rnd, self.family
        rung, kind, far, moving = self.plan[k]
        if inst >= 0:
            o, d = self.object_ray(o, d, inst)
        P = o + s * d
        dn = _unit(d)
        members = self.top if inst < 0 else self.inst[inst]
        m = self.palette[k % len(self.palette)] if self.palette else self.material()
        if family in ("spheres", "mesh_spheres"):
            radius = length * SPHERE_LADDER[rung]
            centre = P
            if kind == 1:
                centre = P + (0.9 * radius) * _unit(np.cross(dn, np.array([rnd.gauss(0, 1) for _ in range(3)])))
            if moving:
                motion = np.array([rnd.uniform(-1, 1) for _ in range(3)]) * length
                members.append(b.sphere(tuple(centre - time * motion), radius, m, tuple(motion)))
            else:
                members.append(b.sphere(tuple(centre), radius, m))
            return rung, kind, (m, -1)
        r = LADDER[rung]
        near = 1.0 - r if far else r
        if family == "triangles":
            u, v = _frame(rnd, dn, length)
            a, bb = ((r, r), (0.5, r), (0.3, 0.3))[kind]
            if kind == 2:
                rung = CENTRE_RUNG
            p0 = P - a * u - bb * v
            members.append(b.triangle(tuple(p0), tuple(p0 + u), tuple(p0 + v), m))
            return rung, kind, (m, -1)
        if kind == 0:
            u, v = _frame(rnd, dn, length)
            Q = P - near * u - near * v
        elif kind in (1, 2, 3):
            u, v = _axis_frame(d, length)
            a, bb = ((near, near), (0.5, near), (0.5, 0.5))[kind - 1]
            if kind == 3:
                rung = CENTRE_RUNG
            Q = P - a * u - bb * v
        else:
            u, v = _frame(rnd, dn, length)
            alpha = 1.0 + r if far else 1.0 - r
            Q = P - alpha * u - 0.5 * v
            m2 = self.palette[(k + 1) % len(self.palette)] if self.palette else self.material()
            members.append(b.quad(tuple(Q), tuple(u), tuple(v), m))
            members.append(b.quad(tuple(Q + u), tuple(u), tuple(v), m2))
            return rung, kind, (m, m2)
        members.append(b.quad(tuple(Q), tuple(u), tuple(v), m))
        return rung, kind, (m, -1)


def _extras(b, rnd, family, centre, dist, side):
    """What only completes a family's mix, beside the frustum (`side`: a unit vector across the view): -> top-level members."""
    at = lambda f: tuple(centre + side * (f * dist))   # noqa: E731
    if family == "triangles":
        return [b.sphere(at(0.50 + 0.03 * i), 0.01 * dist, b.lambertian((0.5, 0.375 + 0.125 * i, 0.25))) for i in range(3)]
    if family == "mesh_spheres":
        e = 0.02 * dist
        return [b.triangle(at(0.50 + 0.04 * i), tuple(np.array(at(0.50 + 0.04 * i)) + np.array([e, 0.0, 0.0])), tuple(np.array(at(0.50 + 0.04 * i)) + np.array([0.0, 0.0, e])),
                           b.lambertian((0.5, 0.375 + 0.125 * i, 0.25))) for i in range(3)]
    if family == "full":
        p = centre + side * (0.62 * dist)
        e = 0.02 * dist
        return [b.sphere(at(0.50), 0.01 * dist, b.textured(b.noise(4.0 / dist, rnd))),
                b.medium(b.sphere(at(0.55), 0.012 * dist, b.dielectric(1.5)), 20.0 / dist, (0.75, 0.75, 0.875)),
                b.triangle(tuple(p), tuple(p + np.array([e, 0.0, 0.0])), tuple(p + np.array([0.0, 0.0, e])), b.lambertian((0.25, 0.625, 0.375)))]
    return []


def _populate(rt, t, cams, seed, size, with_instances, first=0):
    """Targets for the sample-0 rays of every camera -> (rays, rung, kind, own, instance), concatenated over the cameras."""
    parts = []
    k = first
    for cam in cams:
        rays = camera_rays(rt, cam, seed)
        n = len(rays)
        rung, kind, own, instance = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full((n, 2), -1, np.int64), np.full(n, -1, np.int64)
        span = math.sqrt(sum((getattr(cam.pixel00_loc, c) - getattr(cam.center, c)) ** 2 for c in "xyz"))   # ~ the focus distance
        pixel = math.sqrt(sum(getattr(cam.pixel_delta_u, c) ** 2 for c in "xyz"))
        for i in range(n):
            o, d = rays["origin"][i].copy(), rays["direction"][i].copy()
            s = t.rnd.uniform(*t.depth) * t.view_dist / math.sqrt(float(d @ d))
            inst = -1
            if with_instances and k % 3 == 0:
                inst = (k // 3) % len(t.inst)
            rung[i], kind[i], own[i] = t.add(k, o, d, float(rays["time"][i]), s, size * pixel * s * math.sqrt(float(d @ d)) / span, inst)
            instance[i] = inst
            k += 1
        parts.append((rays, rung, kind, own, instance))
    return tuple(np.concatenate([p[f] for p in parts]) for f in range(5))


def _instances(t, lookfrom, lookat):
    """Transforms of the instances: the offsets alternate between 5 % of the viewing distance and 60 % of the way to the camera."""
    away = np.array(lookfrom) - np.array(lookat)
    for i in range(len(t.inst)):
        jitter = np.array([t.rnd.uniform(-1, 1) for _ in range(3)]) * (0.05 * t.view_dist)
        t.inst_xf.append((t.rnd.uniform(-60.0, 60.0), jitter + (0.6 * away if i % 2 else 0.0)))


def _finish(t, extras):
    b = t.b
    top = list(t.top)
    for members, (degrees, offset) in zip(t.inst, t.inst_xf):
        if members:
            top.append(b.translate(b.rotate_y(b.list(members), degrees), tuple(offset)))
    return b.finish(b.list(top + extras))


def build(rt, view, seed, family, size=SIZE, width=0):
    """The scene around the sample-0 rays of camera `view` (a name of CAMERAS) -> (cam, Aimed)."""
    lookfrom, lookat, depth = VIEWS[view]
    cam = camera(rt, view, width or FAMILY_WIDTH[family])
    rnd = random.Random(f"{view}/{family}/{seed}")
    t = _Targets(DescBuilder(), rnd, family)
    t.view_dist, t.depth = math.dist(lookfrom, lookat), depth
    t.plan = _plan(family, cam.image_width * cam.image_height)
    with_instances = family in ("quads", "full")
    if with_instances:
        _instances(t, lookfrom, lookat)
    rays, rung, kind, own, instance = _populate(rt, t, [cam], seed, size, with_instances)
    side = _unit(np.cross(np.array(lookfrom) - np.array(lookat), np.array([0.0, 1.0, 0.0])))
    desc = _finish(t, _extras(t.b, rnd, family, np.array(lookat), t.view_dist, side))
    return cam, Aimed(desc, rays, rung, kind, own, instance, family, SPHERE_LADDER if family in ("spheres", "mesh_spheres") else LADDER)


N_ORIGINS = 16
ORIGIN_WIDTH = 8
ORIGIN_SIZE = 0.125     # of a pixel that is four times as wide: the cloud holds sixteen cameras' targets, each has to stay small


def origins(rt, seed, family):
    """Sixteen 8 x 8 cameras on a sphere around one cloud; each camera's 64 rays have their own targets in the SAME scene
    -> (cams, [Aimed per camera, all over one description]).  The 1 024 targets share a palette of 64 lambertians (pixel p of
    every camera wears colour p), so that the program and its material table fit one CU's LDS and the view-batch kernel runs."""
    rnd = random.Random(f"origins/{family}/{seed}")
    dist = 540.0
    cams, froms = [], []
    for c in range(N_ORIGINS):
        while True:
            v = _unit(np.array([rnd.gauss(0, 1) for _ in range(3)]))
            if abs(v[1]) < 0.9 and min(abs(v)) > 0.05:         # not along vup, no direction component near zero at the centre
                break
        froms.append(tuple(v * dist))
        cams.append(_camera(rt, ORIGIN_WIDTH, froms[-1], (0.0, 0.0, 0.0)))
    t = _Targets(DescBuilder(), rnd, family, palette=ORIGIN_WIDTH * ORIGIN_WIDTH)
    t.view_dist, t.depth = dist, DEPTH
    t.plan = _plan(family, N_ORIGINS * ORIGIN_WIDTH * ORIGIN_WIDTH)
    rays, rung, kind, own, instance = _populate(rt, t, cams, seed, ORIGIN_SIZE, False)
    extras = _extras(t.b, rnd, family, np.array([0.0, 0.0, 0.0]), 1.6 * dist, np.array([0.0, 1.0, 0.0]))
    desc = _finish(t, extras)
    n = ORIGIN_WIDTH * ORIGIN_WIDTH
    ladder = SPHERE_LADDER if family == "spheres" else LADDER
    return cams, [Aimed(desc, *(a[c * n:(c + 1) * n] for a in (rays, rung, kind, own, instance)), family, ladder) for c in range(N_ORIGINS)]


def desc_bytes(desc):
    """Every table of a BuiltDesc, for the determinism test."""
    return b"".join(bytes(v) for _, v in sorted(desc._keep.items()))
