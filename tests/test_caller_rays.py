"""Caller-ray queries against the oracle, in both visiting orders, on rays the camera never produces (tests/caller_rays.py).

No device (conditions on the inputs, not measurements: the rays and the scene seeds were shaped until they hold):
  1. the oracle's new entry points are its old ones: orc.hits with skip = 0 is orc_kat_node_hit of the root, and orc.ray_color
     of a camera ray with skip = get_ray's draws is orc_sample, bit for bit;
  2. orc.hits on the original description equals orc.hits on rtk_scene_optimize's output (with the case's eye and with none) bit
     for bit on every field -- except u, v where the record is a constant medium's, which the reference leaves as they were
      and the device writes as 0;
  3. each of four one-word deviations of a kernel changes the oracle's outcome on at least 1 % of the rays (at least 16);
  4. back faces, medium hits from inside and outside, hits and misses all occur, and every ray that aims away misses;
  5. on the F32 ray set (`Case.f32_set`) the share of rays an F32 walk cannot be held to (test_f32_parity's classifier, the
     perturbed copies taken through the oracle) is at most HIT_MAX_UNSTABLE.

Device (-m gpu), each in both visiting orders:
  6. rtk_query_hits in F64 against orc.hits of the original description (the tolerances of
     test_device_hit_records_match_reference_known_answers), fast-order records = reference-order records bit for bit;
  7. rtk_query_occluded against the oracle's hit flag;
  8. rtk_query_hits in F32 on the F32 ray set under test_f32_parity's judge;
  9. rtk_query_radiance in F64 against orc.ray_color on the first half of the rays (interior, axis, keys).
The bake is held to the oracle in tests/test_light_probes.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests.caller_rays import CLASSES, QUERY_SEED, caller_rays
from tests.conftest import GOLDEN
from tests.desc_builder import SceneDesc
from tests.scene_cases import IMAGE_CASES, RENDER_SEED, SCENE_SEED, scene_file
from tests.test_f32_parity import CAP, HIT_MAX_UNSTABLE, N_COPIES, U, _sphere_terms, classify, judge, perturbed_copies
from tests.test_fast_order_random import random_big_scene, random_fog_scene, random_scene, random_zoo_scene
from tests.test_ray_query import F64_BOUND, identity_scene

N_RAYS = 4096 + 37
RAY_SEED = 2025
ORDERS = ("reference", "fast")
DEPTHS = {c[0]: c[4] for c in IMAGE_CASES}

# name -> (how the scene is made, the bounds the rays are drawn in).  The bounds hold everything but a ground sphere (below)
# and a haze around the whole scene; those of the 400-primitive scene are drawn closer around its fog ball and its moving
# spheres than the primitives reach, so that both are met often enough (condition 3).
SOUP_BOUNDS = ((-7.0, -1.5, -13.0), (7.0, 5.0, 1.0))
CORNELL_BOUNDS = ((-20.0, -20.0, -300.0), (575.0, 575.0, 575.0))


def _named(name):
    return lambda rt: rt.Scene.build(name, SCENE_SEED, scene_file(name, GOLDEN))


SCENES = {
    "three_spheres": (_named("three_spheres"), ((-2.5, -1.0, -3.0), (2.5, 1.5, 1.0))),
    "cornell_box": (_named("cornell_box"), CORNELL_BOUNDS),
    "cornell_smoke": (_named("cornell_smoke"), CORNELL_BOUNDS),
    "material_zoo": (_named("material_zoo"), ((-6.5, -0.5, 2.0), (6.5, 6.0, 9.5))),
    "mesh": (_named("mesh"), ((-3.0, -1.5, -3.0), (4.5, 6.0, 4.5))),
    "random_zoo": (lambda rt: random_zoo_scene(7008), SOUP_BOUNDS),
    "random_fog": (lambda rt: random_fog_scene(4007), SOUP_BOUNDS),
    "random_big": (lambda rt: random_big_scene(9000, 400), ((-3.5, -1.2, -8.0), (3.5, 3.5, -1.0))),
    "random_soup": (lambda rt: random_scene(3003, True), SOUP_BOUNDS),
    "identity": (lambda rt: identity_scene()[0], ((-8.0, -2.0, -2.0), (8.0, 6.0, 2.0))),
}
ALL = pytest.mark.parametrize("name", list(SCENES))
RADIANCE_SCENES = ["three_spheres", "cornell_box", "cornell_smoke", "material_zoo", "random_zoo", "random_fog"]
HIT_FIELDS = ("t", "p", "normal", "u", "v", "hit", "front_face", "material", "prim_kind", "draws")
MEDIUM = 8                                                        # RTK_NODE_MEDIUM


def world_spheres(desc):
    """(centre0, centre_dir, radius) of every sphere the root reaches, in world coordinates: the description's sphere table
    as `_sphere_terms` takes it, each entry once per instance, carried out through the translate (p + offset, hittable.h:55) and
    rotate_y (x = c x' + s z', z = -s x' + c z', hittable.h:128-131) nodes above it.  A medium's boundary sphere is listed too;
    no record lies on it, so it matches nothing."""
    found = []

    def walk(node, to_world):
        n = desc.nodes[node]
        if n.kind == 1:                                           # RTK_NODE_SPHERE
            sp = desc.spheres[n.a]
            c0 = np.array([sp.center0.x, sp.center0.y, sp.center0.z])
            c1 = c0 + np.array([sp.center_dir.x, sp.center_dir.y, sp.center_dir.z])
            w0, w1 = to_world(c0), to_world(c1)
            found.append((w0, w1 - w0, sp.radius))
        elif n.kind == 4:                                         # list
            for k in range(n.b):
                walk(desc.list_children[n.a + k], to_world)
        elif n.kind == 5:                                         # bvh
            walk(n.a, to_world)
            if n.b != n.a:
                walk(n.b, to_world)
        elif n.kind == 6:                                         # translate
            off = desc.translates[n.a].offset
            walk(n.b, lambda q, off=np.array([off.x, off.y, off.z]): to_world(q + off))
        elif n.kind == 7:                                         # rotate_y
            sn, cs = desc.rotates[n.a].sin_theta, desc.rotates[n.a].cos_theta
            walk(n.b, lambda q: to_world(np.array([cs * q[0] + sn * q[2], q[1], -sn * q[0] + cs * q[2]])))
        elif n.kind == 8:                                         # medium: its boundary
            walk(n.b, to_world)

    walk(desc.root, lambda q: q)
    uniq = {(tuple(a), tuple(b), r) for a, b, r in found}
    c0 = np.array([u[0] for u in uniq]).reshape(-1, 3)
    return c0, np.array([u[1] for u in uniq]).reshape(-1, 3), np.array([u[2] for u in uniq])


class Case:
    """One scene, its rays and the oracle's answers on the original description -- computed once, never changed."""

    def __init__(self, rt, orc, name):
        make, self.bounds = SCENES[name]
        self.name, self.scene = name, make(rt)
        self.eye = self.scene.camera(8, 8, 1, 1).center if hasattr(self.scene, "camera") else rt.Vec3(0.0, 0.0, 0.0)
        self.rays, self.cls, self.aims_away = caller_rays(self.scene, self.bounds, N_RAYS, RAY_SEED)
        self.gold = orc.hits(self.scene.desc_ptr, self.rays, QUERY_SEED)
        self.hit = self.gold["hit"] == 1
        self.medium = self.hit & (self.gold["prim_kind"] == MEDIUM)
        desc = SceneDesc.from_address(self.scene.desc_ptr)
        self.spheres = world_spheres(desc)
        self.has_media, self.has_moving = desc.n_media > 0, bool(self.spheres[1].any())
        self._f32 = None

    def upload(self, renderer, order):
        if order == "fast":
            renderer.upload_fast(self.scene, self.eye)
        else:
            renderer.upload(self.scene)


    # -- the F32 ray set and what test_f32_parity's classifier needs, from the inputs and the oracle alone --------------
    def f32_set(self, orc):
        """The rays the F32 walk is judged on: conditions on the inputs under which float arithmetic can decide what the
        reference's formulas ask of it.  Left out are
          * the outside class.  From |oc| = 1e3 .. 1e6 the sphere discriminant h^2 - a c rounds by 8 u a |oc|^2, that is 8 u
            |oc|^2 / r in impact distance -- units on a sphere of radius 100 from 1e4 away -- and a ray that leaves the scene has
            roots (h +- sd) / a = +- 4 u |h| / a, on either side of tmin;
          * in a scene with media, rays with |d| < 2 sqrt(3) extent / 512 (extent: the largest coordinate of any hit point).
            constant_medium::hit restarts its second boundary query at rec1.t + 0.0001 (constant_medium.h:24); a float keeps
            that step only where 0.0001 > ulp(t) / 2, safely for |t| < 512, and |t| <= (|o| + sqrt(3) extent) / |d|;
          * hits on a sphere of the description's table within sin(theta) < 0.02 of its poles (theta from the y axis).  There
            u = atan2(-n_z, n_x) / 2 pi and v = acos(-n_y) / pi move by dn / sin(theta) (`_sphere_terms`), which passes the
            judge's cap 2^-12 for the 64 u a normal always carries once sin(theta) < 64 * 2^-24 * 2^12 / pi = 0.005; four
            times that leaves room for the terms that grow with the sphere's radius.  (Every hit on the radius-1000 ground
            under the mesh lies there.);
          * interval edges around a medium's record (the oracle's answer for the same ray with tmin = 0.001, tmax = inf).  Such
            a ray has three outcomes -- the interval ends before the medium is entered: no draw; between the entry and the
            scattering point: a draw and a miss; beyond it: the hit -- and the middle one is as narrow as the free path (1e-6
            in `identity`), far below what sixteen copies moved by 2^-21 sample, so the judge's set of plausible outcomes
            would lack an outcome the reference itself has."""
        g, d = self.gold, np.linalg.norm(self.rays["direction"], axis=1)
        keep = self.cls != CLASSES.index("outside")
        if self.has_media:
            keep &= d >= 2.0 * math.sqrt(3.0) * self.extent() / 512.0
        on_table = np.zeros(len(g), bool)
        c0, cdir, rad = self.spheres
        for k in np.nonzero(self.hit & (g["prim_kind"] == 1))[0]:
            c = c0 + self.rays["time"][k] * cdir
            on_table[k] = (np.abs(np.linalg.norm(g["p"][k] - c, axis=1) - rad) <= 1e-9 * np.maximum(rad, 1.0)).any()
        keep &= ~(on_table & (np.sqrt(np.maximum(1.0 - g["normal"][:, 1] ** 2, 0.0)) < 0.02))
        edges = self.cls == CLASSES.index("edges")
        if self.has_media:
            unbounded = self.rays[edges].copy()
            unbounded["tmin"], unbounded["tmax"] = 0.001, np.inf
            keep[edges] &= orc.hits(self.scene.desc_ptr, unbounded, QUERY_SEED)["prim_kind"] != MEDIUM
        return keep

    def extent(self):
        return max(float(np.abs(self.gold["p"][self.hit]).max()), 1.0)

    def f32_inputs(self, orc):
        """keep, stable, gold_d, copies_d, bound, scale, gold_c as hit_kat (tests/test_f32_parity.py) makes them for one object
        root, with the oracle in the place of the F64 kernel -- for a whole scene, whose coordinates span far more than one
        ray's do (a ground sphere of radius 1000 under spheres of radius 0.5).  Two sets of perturbed copies:
          * coordinates moved by 2^-21 of the SCENE's extent (the farthest hit point: the far side of the ground sphere).  An F32
            walk rounds centre - origin of every sphere it tests at that sphere's scale, so a hit-or-miss decision within that
            of its boundary is not the ray's to make: these copies, and the next, decide `stable` and are the outcomes an
            unstable ray may show;
          * coordinates moved by 2^-21 of the RAY's own scale S = max(|o|, |p|, 1): the spread of the continuous outputs over
            these is the ray's conditioning, and the bound is spread + 64 u S + the sphere terms -- those carry the rounding of
            the sphere that was hit at its own scale (|centre - origin|), whatever S is.  hit_kat's bound with S the object's
            extent is never smaller than this one.
        u, v of a medium's record are 0, as the device writes them."""
        if self._f32 is None:
            keep = self.f32_set(orc)
            rays, gold, n = self.rays[keep], self.gold[keep], int(keep.sum())
            x = np.column_stack([rays["origin"], rays["direction"], rays["time"], rays["tmin"], rays["tmax"]])
            S = np.maximum.reduce([np.abs(x[:, :3]).max(1), np.abs(gold["p"]).max(1), np.ones(n)])

            def through_the_oracle(abs_scale, seed):
                cp = perturbed_copies(x, np.zeros_like(x, bool), pos_cols=(0, 1, 2), abs_scale=abs_scale, seed=seed).reshape(-1, 9)
                moved = np.tile(rays, N_COPIES)
                moved["origin"], moved["direction"], moved["time"], moved["tmin"], moved["tmax"] = cp[:, 0:3], cp[:, 3:6], cp[:, 6], cp[:, 7], cp[:, 8]
                return orc.hits(self.scene.desc_ptr, moved, QUERY_SEED)

            wide, own = through_the_oracle(np.maximum(S, self.extent()), len(self.name)), through_the_oracle(S, len(self.name) + 100)
            gold_d, gold_c = _discrete(gold), _continuous(gold)
            copies_d = np.concatenate([_discrete(wide).reshape(N_COPIES, n, 4), _discrete(own).reshape(N_COPIES, n, 4)])
            stable, spread = classify(gold_d, copies_d, _continuous(own).reshape(N_COPIES, n, 9), gold_c)
            dlen = np.linalg.norm(x[:, 3:6], axis=1)
            scale = np.concatenate([(S / np.maximum(dlen, 1e-300))[:, None], np.repeat(S[:, None], 3, 1), np.ones((n, 5))], 1)
            radii = self.spheres[2][self.spheres[2] > 0]
            as_kat = np.column_stack([gold["hit"], gold["t"], gold["p"], gold["normal"]])        # the columns _sphere_terms reads
            terms = _sphere_terms(x, as_kat, self.spheres, float(radii.min()) if len(radii) else None) if len(self.spheres[2]) else np.zeros((n, 9))
            bound = spread + 64.0 * U * scale + terms
            self._f32 = dict(keep=keep, stable=stable, gold_d=gold_d, copies_d=copies_d, bound=bound, scale=scale, gold_c=gold_c)
        return self._f32


def _discrete(h):
    return np.stack([h["hit"], h["material"], h["front_face"] * h["hit"], h["draws"]], 1).astype(np.float64)


def _continuous(h):
    """t, p, normal, u, v of a hit, 0 on a miss; u, v 0 on a medium's record (prim_kind is the oracle's and the device's)."""
    uv = np.where((h["prim_kind"] == MEDIUM)[:, None], 0.0, np.stack([h["u"], h["v"]], 1))
    return np.where((h["hit"] == 1)[:, None], np.column_stack([h["t"], h["p"], h["normal"], uv]), 0.0)


@pytest.fixture(scope="module")
def cases(rt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(rt, orc, name)
        return cache[name]
    return get


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def differing(a, b, fields=HIT_FIELDS, but_uv_of=None):
    """Rays on which any of `fields` differs in any bit (NaNs compared as bits); u, v are left out where `but_uv_of` is set."""
    out = np.zeros(len(a), bool)
    for f in fields:
        d = _bits(np.ascontiguousarray(a[f])) != _bits(np.ascontiguousarray(b[f]))
        d = d.any(axis=1) if d.ndim == 2 else d
        out |= d & ~but_uv_of if (but_uv_of is not None and f in ("u", "v")) else d
    return out


def need(n):
    return max(16, math.ceil(0.01 * n))


# ----------------------------------------------------------------------------------------------------- no device --
def test_the_rays_are_laid_out_as_the_generator_says(rt, cases):
    c = cases("three_spheres")
    rays, cls = c.rays, c.cls
    assert rays.dtype == rt.ray_dtype() and len(rays) == N_RAYS and N_RAYS % 256 != 0
    assert all((cls[w * 64:(w + 1) * 64] == cls[w * 64]).all() for w in range(N_RAYS // 64))           # whole waves of one class
    assert list(cls[:32 * 64]) == sorted(cls[:32 * 64]) and set(cls[:32 * 64]) == {0, 1, 2}              # interior, axis, keys first
    assert len(set(cls[64 * 64:].tolist())) == len(CLASSES)                                             # the tail interleaves all
    zero = rays["direction"] == 0.0
    axis = cls == CLASSES.index("axis")
    assert zero[axis].any(axis=1).all() and not zero[axis].all(axis=1).any() and (zero[axis].sum(axis=1) == 2).any() and not zero[~axis].any()
    assert not rays["reserved"].any() and set(rays["skip"].tolist()) == {0, 1, 7, 1000}
    keys = rays[cls == CLASSES.index("keys")]
    assert (keys["time"] == 0.0).sum() >= 100 and (keys["time"] == 1.0).sum() >= 100 and ((rays["time"] >= 0) & (rays["time"] <= 1)).all()
    seg = rays[cls == CLASSES.index("segments")]
    assert (seg["tmin"] == 0.001).all() and (seg["tmax"] == 1 - 0.001).all()
    edges = rays[cls == CLASSES.index("edges")]
    assert (edges["tmin"] > edges["tmax"]).sum() >= 16 and np.isfinite(edges["tmax"]).sum() > 100 and (edges["tmin"] != 0.001).sum() > 100
    lo, hi = np.array(c.bounds[0]), np.array(c.bounds[1])
    dist = np.linalg.norm(rays["origin"][cls == CLASSES.index("outside")] - 0.5 * (lo + hi), axis=1)
    assert dist.min() >= 1e3 and dist.max() <= 2.1e6 and dist.max() > 1e5
    again, _, _ = caller_rays(c.scene, c.bounds, N_RAYS, RAY_SEED)
    assert again.tobytes() == rays.tobytes()


def test_the_oracles_ray_entry_points_are_its_old_ones(rt, orc):
    """skip = 0: orc_ray_hit is orc_kat_node_hit of the root.  A camera ray with skip = get_ray's draws: orc.ray_color is
    orc_sample, radiance and draws, bit for bit -- so the caller-ray oracle inherits what test_oracle_goldens pins."""
    lib = orc.lib()
    for name in ("three_spheres", "cornell_smoke", "material_zoo"):
        scene = _named(name)(rt)
        depth = DEPTHS[name]
        cam = scene.camera(16, 12, 1, depth)
        rays = np.zeros(16 * 12, rt.ray_dtype())
        want, want_draws = np.zeros((len(rays), 3)), np.zeros(len(rays), np.uint64)
        for k in range(len(rays)):
            i, j, out, drew = k % 16, k // 16, np.zeros(7), C.c_uint64()
            lib.orc_kat_get_ray(C.addressof(cam), RENDER_SEED, i, j, 2, out.ctypes.data, C.addressof(drew))
            rays[k] = (out[0:3], out[3:6], out[6], 0.001, np.inf, k, 2, drew.value, 0)
            assert lib.orc_sample(scene.desc_ptr, C.addressof(cam), RENDER_SEED, i, j, 2, want[k].ctypes.data, want_draws[k:].ctypes.data) == 0
        got, draws = orc.ray_color(scene.desc_ptr, rays, max_depth=depth, background=cam.background, seed=RENDER_SEED)
        assert got.tobytes() == want.tobytes() and np.array_equal(draws + rays["skip"], want_draws), name
        two, two_draws = orc.ray_color(scene.desc_ptr, rays, max_depth=depth, background=cam.background, samples=2, seed=RENDER_SEED)
        shifted = rays.copy()
        shifted["sample"] += 1
        second, second_draws = orc.ray_color(scene.desc_ptr, shifted, max_depth=depth, background=cam.background, seed=RENDER_SEED)
        assert np.array_equal(two, (got + second) / 2.0) and np.array_equal(two_draws, draws + second_draws)
        plain = rays.copy()
        plain["skip"] = 0
        h = orc.hits(scene.desc_ptr, plain, RENDER_SEED)
        root = SceneDesc.from_address(scene.desc_ptr).root
        for k in range(0, len(rays), 7):
            odt, rec, drew = np.concatenate([rays["origin"][k], rays["direction"][k], [rays["time"][k]]]), np.zeros(11), C.c_uint64()
            flag = lib.orc_kat_node_hit(scene.desc_ptr, root, odt.ctypes.data, 0.001, np.inf, RENDER_SEED, k, 2, rec.ctypes.data, C.addressof(drew))
            assert (flag, drew.value) == (h["hit"][k], h["draws"][k])
            if flag:
                assert np.array_equal(rec, np.concatenate([[h["t"][k]], h["p"][k], h["normal"][k], [h["front_face"][k], h["u"][k], h["v"][k], h["material"][k]]]), equal_nan=True)


@ALL
def test_the_oracle_agrees_in_both_visiting_orders(rt, orc, cases, name):
    """Every field of every record, bit for bit, between the original description and rtk_scene_optimize's, priced for the
    case's eye and for none: the pruning boxes of the fast order are cost, never correctness, for any origin, direction and
    interval -- not only for what a camera path produces."""
    c = cases(name)
    for eye in (c.eye, None):
        fast = rt.FastOrderScene(c.scene, eye)
        assert fast.exact
        got = orc.hits(fast.desc_ptr, c.rays, QUERY_SEED)
        bad = differing(got, c.gold, but_uv_of=c.medium)
        stale = int((differing(got, c.gold) & ~bad).sum())
        print(f"{name} eye {'none' if eye is None else 'the case`s'}: {int(bad.sum())} records differ; {stale} more in a medium's stale u, v")
        assert not bad.any(), (name, np.nonzero(bad)[0][:8], c.rays[bad][:2], got[bad][:2], c.gold[bad][:2])


DEVIATIONS = {"tmin read as 0.001": ("tmin", 0.001, lambda c: True), "tmax read as inf": ("tmax", np.inf, lambda c: True),
              "time read as 0": ("time", 0.0, lambda c: c.has_moving), "skip read as 0": ("skip", 0, lambda c: c.has_media)}


@ALL
def test_each_deviation_changes_the_oracles_outcome(orc, cases, name):
    """What a subtly wrong kernel would compute, one word at a time: the record of at least 1 % of the rays (at least 16)
    changes in some bit, so a comparison with the oracle on these rays sees it."""
    c = cases(name)
    seen = {}
    for what, (field, value, applies) in DEVIATIONS.items():
        if not applies(c):
            continue
        rays = c.rays.copy()
        rays[field] = value
        seen[what] = int(differing(orc.hits(c.scene.desc_ptr, rays, QUERY_SEED), c.gold).sum())
    print(f"{name}: rays whose record changes, of {len(c.rays)} (needed {need(len(c.rays))}): {seen}")
    assert all(count >= need(len(c.rays)) for count in seen.values()), (name, seen)
    assert len(seen) == 2 + c.has_moving + c.has_media


def test_the_scene_set_has_media_and_moving_spheres(cases):
    assert sum(cases(n).has_media for n in SCENES) >= 5 and sum(cases(n).has_moving for n in SCENES) >= 4
    assert all(cases(n).has_media for n in ("cornell_smoke", "random_zoo", "random_fog", "random_big", "identity"))


def _starts_in_its_medium(c, orc):
    """Rays whose medium record belongs to a medium entered before the ray's own tmin = 0.001 -- the free path then starts at
    tmin (constant_medium.h:33), so the record moves when tmin grows by 2^-20 of itself; a medium entered later keeps its entry
    and the record.  The oracle decides."""
    rays = c.rays.copy()
    rays["tmin"] *= 1.0 + 2.0 ** -20
    moved = orc.hits(c.scene.desc_ptr, rays, QUERY_SEED)
    return c.medium & (c.rays["tmin"] == 0.001) & (moved["prim_kind"] == MEDIUM) & (moved["t"] != c.gold["t"])


@ALL
def test_the_rays_meet_every_kind_of_outcome(orc, cases, name):
    """Hits and misses at least 10 % each; at least 10 % of the hits show a back face; every ray that aims away misses; in a
    scene with media at least 32 records are a medium's, some of rays that start inside it, and rays that miss drew too."""
    c = cases(name)
    g = c.gold
    back = c.hit & (g["front_face"] == 0)
    starts_inside = _starts_in_its_medium(c, orc)
    print(f"{name}: hits {c.hit.mean():.3f} of the rays, back faces {back.sum() / c.hit.sum():.3f} of the hits, {int(c.medium.sum())} hits in a medium, "
          f"{int(starts_inside.sum())} of them on rays that start inside it; {int(c.aims_away.sum())} rays aim away")
    assert 0.10 <= c.hit.mean() <= 0.90
    assert back.sum() >= 0.10 * c.hit.sum()
    assert c.aims_away.sum() >= 150 and not c.hit[c.aims_away].any()
    if c.has_media:
        assert c.medium.sum() >= 32 and starts_inside.sum() >= 16 and g["draws"][~c.hit].any()
    else:
        assert not c.medium.any() and not g["draws"].any()


@ALL
def test_the_share_of_rays_an_f32_walk_cannot_be_held_to(orc, cases, name):
    """test_f32_parity's classifier on the F32 ray set (`Case.f32_set`), from the inputs and the oracle alone: a ray is unstable
    when one of sixteen copies perturbed by 2^-21 changes the oracle's discrete outcome, or when its measured conditioning puts
    the bound past 2^-12 of its scale.  The interval edges are unstable by construction; the share of the set stays under the cap
    the known-answer rays are held to, and the set keeps at least 1000 rays of five classes."""
    c = cases(name)
    f = c.f32_inputs(orc)
    keep = f["keep"]
    well = f["stable"] & (f["bound"] <= CAP * f["scale"]).all(axis=1)
    frac = float((~well).mean())
    print(f"{name}: {int(keep.sum())} rays in the F32 set, unstable share {frac:.4f}; per class",
          {CLASSES[k]: round(float((~well)[c.cls[keep] == k].mean()), 3) for k in range(len(CLASSES)) if (c.cls[keep] == k).any()})
    assert frac <= HIT_MAX_UNSTABLE, (name, frac)
    assert keep.sum() >= 1000 and len(set(c.cls[keep].tolist())) == len(CLASSES) - 1
    assert (well & (f["gold_d"][:, 0] == 1)).sum() >= 200         # the continuous checks have work to do


# --------------------------------------------------------------------------------------------------------- device --
def _worst(got, want, tol, scale):
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - want) / (tol * scale)
    return np.where(np.isnan(got) & np.isnan(want), 0.0, np.where(np.isnan(ratio), np.inf, ratio))


@pytest.mark.gpu
@ALL
def test_f64_hits_are_the_oracles_in_both_orders(rt, renderer, cases, name):
    """hit, front_face, material, prim_kind and draws equal; t, p, normal within 1e-13 max(1, |want|); u, v within 1e-13 (NaN
    where the oracle has NaN), and 0 on a medium's record.  The fast order's records are the reference order's bit for bit,
    prim_kind and prim_index included."""
    c = cases(name)
    g, hit = c.gold, c.hit
    results = {}
    for order in ORDERS:
        c.upload(renderer, order)
        h = renderer.query_hits(c.rays, seed=QUERY_SEED)
        for f in ("hit", "front_face", "material", "prim_kind", "draws"):
            bad = np.nonzero(h[f] != g[f])[0]
            assert not len(bad), (name, order, f, bad[:8], [CLASSES[k] for k in c.cls[bad[:8]]], h[f][bad[:8]], g[f][bad[:8]])
        worst = {}
        for f in ("t", "p", "normal"):
            worst[f] = float(_worst(h[f][hit], g[f][hit], 1e-13, np.maximum(1.0, np.abs(g[f][hit]))).max())
        surface = hit & ~c.medium
        worst["uv"] = float(max(_worst(h[f][surface], g[f][surface], 1e-13, 1.0).max() for f in ("u", "v")))
        print(f"{name} {order}: worst ratio to the tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, (name, order, worst)
        assert not h["u"][c.medium].any() and not h["v"][c.medium].any()
        miss = h[~hit]
        assert not miss["t"].any() and not miss["p"].any() and (miss["prim_index"] == -1).all() and (h["prim_index"][hit] >= 0).all()
        results[order] = h
    assert results["reference"].tobytes() == results["fast"].tobytes()


@pytest.mark.gpu
@ALL
def test_occlusion_is_the_oracles_hit_flag_in_both_orders(rt, renderer, cases, name):
    """rtk_query_occluded against the oracle -- not against rtk_query_hits.  Scenes without a medium take the early exit under
    the rays' own tmax (the segments, the interval edges); scenes with one the closest-hit walk."""
    c = cases(name)
    for order in ORDERS:
        c.upload(renderer, order)
        occluded = renderer.query_occluded(c.rays, seed=QUERY_SEED)
        bad = np.nonzero(occluded != c.gold["hit"])[0]
        print(f"{name} {order}: {int(occluded.sum())} of {len(occluded)} occluded, {len(bad)} differ from the oracle")
        assert occluded.dtype == np.int32 and not len(bad), (name, order, bad[:8], [CLASSES[k] for k in c.cls[bad[:8]]])


@pytest.mark.gpu
@ALL
def test_f32_hits_under_the_known_answer_judge(rt, orc, renderer, cases, name):
    """test_f32_parity's judge on the F32 ray set with the oracle's perturbed copies, both orders: on a stable ray the F32
    discrete outcome (hit, material, front face, draws) is the oracle's and t, p, normal, u, v lie within spread + 64 u S + the
    sphere terms; on an unstable one the outcome is the oracle's or one a copy gave."""
    c = cases(name)
    f = c.f32_inputs(orc)
    rays = c.rays[f["keep"]]
    for order in ORDERS:
        c.upload(renderer, order)
        h = renderer.query_hits(rays, seed=QUERY_SEED, real_mode=rt.RTK_REAL_F32)
        f32_d, f32_c = _discrete(h), _continuous(h)
        assert not h["u"][h["prim_kind"] == MEDIUM].any() and not h["v"][h["prim_kind"] == MEDIUM].any()
        err = np.abs(f32_c - f["gold_c"])
        err = np.where(np.isnan(f32_c) & np.isnan(f["gold_c"]), 0.0, err)
        err = np.where((f32_d[:, :1] == f["gold_d"][:, :1]) & (f["gold_d"][:, :1] == 1), err, 0.0)
        r = judge(f"{name} {order}", f["stable"], f["gold_d"], f32_d, f["copies_d"], err, f["bound"], f["scale"], HIT_MAX_UNSTABLE)
        print(f"{name} {order}: {r}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RADIANCE_SCENES)
def test_f64_radiance_is_the_oracles_in_both_orders(rt, orc, renderer, cases, name):
    """The 2048 rays of the interior, axis and keys classes (radiance ignores tmin and tmax), depth 1 and the case's (at most
    8), samples 1 and 3: |got - want| <= 1e-12 max(1, |want|) per channel, the draws equal, the counting build's bits the plain
    build's."""
    c = cases(name)
    rays = c.rays[:32 * 64]
    assert set(c.cls[:32 * 64]) == {0, 1, 2}
    bg = (0.3, 0.4, 0.6)
    worst = {}
    for depth in sorted({1, min(DEPTHS.get(name, 8), 8)}):
        for samples in (1, 3):
            want, want_draws = orc.ray_color(c.scene.desc_ptr, rays, max_depth=depth, background=bg, samples=samples, seed=QUERY_SEED)
            assert np.isfinite(want).all() and want_draws.any()
            assert depth == 1 or len(np.unique(want, axis=0)) > 16      # (depth 1 is emission, background or black)
            for order in ORDERS:
                c.upload(renderer, order)
                got, draws = renderer.query_radiance(rays, max_depth=depth, background=bg, samples=samples, count=True, seed=QUERY_SEED)
                ratio = np.abs(got - want) / (F64_BOUND * np.maximum(1.0, np.abs(want)))
                worst[order] = max(worst.get(order, 0.0), float(ratio.max()))
                assert ratio.max() <= 1.0, (name, order, depth, samples, float(ratio.max()), int(np.argmax(ratio.max(axis=1))))
                assert np.array_equal(draws.astype(np.uint64), want_draws), (name, order, depth, samples)
                plain = renderer.query_radiance(rays, max_depth=depth, background=bg, samples=samples, seed=QUERY_SEED)
                assert plain.tobytes() == got.tobytes(), (name, order, depth, samples)
    print(f"{name}: worst |query - oracle| / (1e-12 max(1, |oracle|)): " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
