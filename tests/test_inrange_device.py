"""The guarded short f64 square roots and reciprocals (csrc/rtk_device_math.h: sqrt_inrange, rcp_inrange, the sites' guards)
on the device, against the CPU oracle, bit for bit.

The f64 known-answer entry points run the same device functions with the same guards as the lean MIXED render kernel:
rtk_debug_closest_hit reaches the sphere discriminant's square root (sphere_root), rtk_debug_scatter the sites of the shade
step (random_unit_vector, unit_vector of the incoming / reflected direction, the dielectric's sin_theta and refract).  A
lane-per-ray kernel puts 64 consecutive cases into one wave and a guard is decided per wave, so the inputs come in runs of
whole waves that stay on the short forms, whole waves of edge operands, and waves that mix both (then the in-range lanes
take the full expansion too and must still give the same bits).

Not among the cases: a random_unit_vector draw of (0, 0, 0).  A draw is zero when the generator's 24-bit output is 2^23; an
exhaustive walk over all 2^32 generator states finds 256 states whose next draw is zero and none whose next two are, so no
key yields it (the guard sends that operand to the full expansion all the same: tests/test_inrange_identities.py).

The last test renders the smallest frame in which all three materials and the defocus lens occur through the lean MIXED
kernel itself, in both visiting orders."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.desc_builder import DescBuilder
from tests.scene_cases import RENDER_SEED, SCENE_SEED, scene_file

pytestmark = pytest.mark.gpu

N = 4096
WAVE = 64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def edge_scene():
    """Three spheres at integer coordinates with integer radii (3, 5, 13: circles with integer points), one per material."""
    b = DescBuilder()
    matte, metal, glass, mirror = b.lambertian((0.5, 0.4, 0.3)), b.metal((0.7, 0.6, 0.5), 0.5), b.dielectric(1.5), b.metal((0.9, 0.9, 0.9), 0.0)
    spheres = [((0.0, 0.0, -10.0), 5.0, matte), ((20.0, 0.0, -10.0), 3.0, metal), ((-20.0, 0.0, -10.0), 13.0, glass)]
    root = b.list([b.sphere(c, r, m) for c, r, m in spheres])
    return b.finish(root), root, spheres, (matte, metal, glass, mirror)


def _circle_points(r):
    r = int(r)
    return [(x, y) for x in range(-r, r + 1) for y in range(-r, r + 1) if x * x + y * y == r * r]


def tangent_rays(spheres, n):
    """Rays along -z through an integer point of a sphere's silhouette circle: every term of sphere.h:33-39 is an integer, so
    the discriminant h*h - a*c is EXACTLY 0.  Returns the rays and, per ray, which origin coordinate may be nudged."""
    rays, axis = [], []
    for k in (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0):
        for oz in (0.0, 1.0, 2.0, 5.0, 11.0):
            for (c, r, _m) in spheres:
                for (x, y) in _circle_points(r):
                    rays.append([c[0] + x, c[1] + y, oz, 0.0, 0.0, -k, 0.0, 0.001, np.inf])
                    axis.append(0 if x != 0 else 1)
    assert len(rays) >= n
    return np.array(rays[:n]), np.array(axis[:n])


def generic_rays(rng, spheres, n):
    """Rays from around (0, 0, 8) towards points inside the spheres: ordinary discriminants, most of them hits."""
    idx = rng.integers(0, len(spheres), n)
    centres = np.array([s[0] for s in spheres])[idx]
    radii = np.array([s[1] for s in spheres])[idx]
    target = centres + rng.uniform(-1.1, 1.1, (n, 3)) * radii[:, None]
    origin = np.array([0.0, 0.0, 8.0]) + rng.uniform(-3, 3, (n, 3))
    d = (target - origin) * rng.uniform(0.25, 4.0, (n, 1))
    return np.concatenate([origin, d, rng.uniform(0, 1, (n, 1)), np.full((n, 1), 0.001), np.full((n, 1), np.inf)], 1)


def interleave(parts, n):
    """Waves that mix the parts: consecutive cases come from different parts."""
    rows = [p[i] for i in range(max(len(p) for p in parts)) for p in parts if i < len(p)]
    return np.array(rows[:n])


@pytest.fixture(scope="module")
def uploaded(renderer):
    scene, root, spheres, mats = edge_scene()
    renderer.upload(scene)
    return scene, root, spheres, mats


def test_sphere_discriminant_site_at_its_edges(orc, renderer, uploaded):
    """4 096 rays through rtk_debug_closest_hit: t, p, normal, front face, material and the draw counts equal the oracle's,
    bit for bit (u and v, which come from acos / atan2, to 1e-13).  Runs of whole waves: discriminants of exactly 0 (the wave takes the full expansion); discriminants
    within a few ulp of 0 (tangent rays with one origin coordinate moved by 1 .. 4 ulp either way: tiny but admitted, or
    negative -- a miss); ordinary rays (short form); directions 1e-150 and 1e150 long (discriminants near 1e-300 / 1e300:
    outside the admitted range); and waves that mix all of these."""
    scene, root, spheres, _ = uploaded
    rng = np.random.default_rng(20251)
    q = N // 4
    exact, axis = tangent_rays(spheres, q)
    near = exact.copy()
    steps = np.array([1, -1, 2, -2, 3, -3, 4, -4])[np.arange(q) % 8]
    for i in range(q):
        v = near[i, axis[i]]
        for _ in range(abs(steps[i])):
            v = np.nextafter(v, np.inf if steps[i] > 0 else -np.inf)
        near[i, axis[i]] = v
    plain = generic_rays(rng, spheres, q // 2)
    tiny, huge = generic_rays(rng, spheres, q // 4), generic_rays(rng, spheres, q // 4)
    tiny[:, 3:6] *= 1e-150
    huge[:, 3:6] *= 1e150
    mixed = interleave([exact[::4], near[::4], generic_rays(rng, spheres, q // 4), tiny[::2], huge[::2]], q)
    rays = np.concatenate([exact, near, plain, tiny, huge, mixed])
    assert rays.shape == (N, 9) and q % WAVE == 0 and (q // 4) % WAVE == 0      # every run is whole waves
    keys = np.stack([np.full(N, 11), np.arange(N), np.arange(N) % 7], 1).astype(np.uint32)

    want = np.zeros((N, 12))
    want[:, 11] = -1
    want_draws = np.zeros(N, np.uint64)
    lib, rec, draws = orc.lib(), (C.c_double * 11)(), C.c_uint64()
    for k in range(N):
        ray = (C.c_double * 7)(*rays[k, 0:7])
        if lib.orc_kat_node_hit(scene.desc_ptr, root, C.addressof(ray), float(rays[k, 7]), float(rays[k, 8]), int(keys[k, 0]), int(keys[k, 1]), int(keys[k, 2]),
                                C.addressof(rec), C.byref(draws)):
            want[k, 0] = 1
            want[k, 1:12] = rec[:]
        want_draws[k] = draws.value
    got, got_draws = renderer.closest_hit(rays, keys)

    hit = want[:, 0] == 1
    assert hit[:q].all()                                   # a discriminant of exactly 0 is a hit (sphere.h:40: only disc < 0 misses) ...
    assert np.array_equal(want[:q, 1], (10.0 + exact[:, 2]) / -exact[:, 5])   # ... at t = h / a, the distance to the sphere's equator plane
    assert 0.2 * q < hit[q:2 * q].sum() < 0.8 * q          # a few ulp either way: both outcomes
    assert hit[2 * q:3 * q].mean() > 0.3 and hit[3 * q:].mean() > 0.3     # (the inputs: a good share of the other rays hit something)
    assert np.array_equal(got[:, 0], want[:, 0])
    exact_cols = [1, 2, 3, 4, 5, 6, 7, 8, 11]              # t, p, normal, front face, material: bit for bit
    same = same_bits(got[hit][:, exact_cols], want[hit][:, exact_cols])
    assert same.all(), np.argwhere(~same)[:5]
    # u, v (sphere.h:67-78: acos, atan2) are no part of the changed sites; the device's acos / atan2 differ from libm by an ulp
    # here and there, as in tests/test_gpu_parity.py's known answers: 1e-13
    guv, wuv = got[hit][:, 9:11], want[hit][:, 9:11]
    with np.errstate(invalid="ignore"):
        uv_ok = same_bits(guv, wuv) | (np.abs(guv - wuv) <= 1e-13)     # (NaN where the oracle has NaN: acos of an argument an ulp past 1)
    assert uv_ok.all(), (guv[~uv_ok.all(axis=1)][:5], wuv[~uv_ok.all(axis=1)][:5])
    assert np.array_equal(got_draws, want_draws)


def scatter_cases(rng, mats):
    matte, metal, glass, mirror = mats
    q = N // 4

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def generic(n, kinds):
        normal = unit(rng.normal(size=(n, 3)))
        d = -0.35 * normal + 0.9 * unit(rng.normal(size=(n, 3)))        # any angle, grazing ones and some from below the surface among them
        d *= rng.uniform(0.25, 4.0, (n, 1))
        p = rng.uniform(-20, 20, (n, 3))
        front = rng.integers(0, 2, n).astype(np.float64)
        ray = np.concatenate([p - d, d, rng.uniform(0, 1, (n, 1))], 1)
        rec = np.concatenate([np.ones((n, 1)), p, normal, front[:, None], rng.uniform(0, 1, (n, 2)), np.zeros((n, 1))], 1)
        return np.array(kinds)[rng.integers(0, len(kinds), n)], ray, rec

    # A: lambertian and metal on ordinary inputs (short forms throughout)
    a = generic(q, [matte, metal, mirror])
    # B: the dielectric at its edges -- axis-aligned directions of integer length against axis-aligned normals: cos_theta is
    # exactly 1 (sin_theta = sqrt(0): full expansion) or exactly 0 (sin_theta = sqrt(1) = 1); 3-4-5 directions against the
    # matching normals: within an ulp of those; front and back faces (total internal reflection from inside); then ordinary ones
    edge_dirs = [((0.0, 0.0, -1.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, -2.0), (0.0, 0.0, 1.0)), ((0.0, -4.0, 0.0), (0.0, 1.0, 0.0)),   # head-on
                 ((0.0, 0.0, -1.0), (1.0, 0.0, 0.0)), ((0.0, 0.0, -2.0), (0.0, 1.0, 0.0)), ((4.0, 0.0, 0.0), (0.0, 0.0, 1.0)),     # grazing
                 ((-3.0, -4.0, 0.0), (0.6, 0.8, 0.0)), ((-6.0, 0.0, -8.0), (0.6, 0.0, 0.8)),                                      # head-on, inexact
                 ((-3.0, -4.0, 0.0), (0.8, -0.6, 0.0)), ((0.0, -5.0, -12.0), (0.0, 12.0 / 13.0, -5.0 / 13.0))]                   # grazing, inexact
    nb = q // 2
    b_kind = np.full(nb, glass)
    b_ray = np.zeros((nb, 7))
    b_rec = np.zeros((nb, 11))
    for i in range(nb):
        d, nrm = edge_dirs[(i // WAVE) % len(edge_dirs)] if i < nb // 2 else edge_dirs[i % len(edge_dirs)]   # whole waves of one edge, then mixed
        b_ray[i] = [1.0 - d[0], 2.0 - d[1], 3.0 - d[2], d[0], d[1], d[2], 0.5]
        b_rec[i] = [1.0, 1.0, 2.0, 3.0, nrm[0], nrm[1], nrm[2], float((i // 2) % 2), 0.25, 0.75, 0.0]
    b2 = generic(q - nb, [glass])
    # C: directions 1e-150 and 1e150 long on every material (squared lengths near 1e-300 / 1e300: outside the admitted range)
    c = generic(q, [matte, metal, glass, mirror])
    c[1][:q // 2, 3:6] *= 1e-150
    c[1][q // 2:, 3:6] *= 1e150
    # D: waves that mix all of the above
    d1, d2 = generic(q // 4, [matte, metal, glass]), generic(q // 4, [metal, glass])
    d2[1][:, 3:6] *= np.where(np.arange(q // 4) % 2 == 0, 1e-150, 1e150)[:, None]
    parts = [(a[0][::4], a[1][::4], a[2][::4]), (b_kind[::2], b_ray[::2], b_rec[::2]), d1, d2]
    d_all = tuple(interleave([p[j] for p in parts], q) for j in range(3))
    kinds = np.concatenate([a[0], b_kind, b2[0], c[0], d_all[0]]).astype(np.int32)
    rays = np.concatenate([a[1], b_ray, b2[1], c[1], d_all[1]])
    recs = np.concatenate([a[2], b_rec, b2[2], c[2], d_all[2]])
    return kinds, rays, recs, (q, nb)


def test_shade_step_sites_at_their_edges(orc, renderer, uploaded):
    """4 096 hit records through rtk_debug_scatter: the scattered-or-not decision, the scattered ray (origin, direction, time),
    the attenuation and the draw counts equal the oracle's, bit for bit."""
    scene, _root, _spheres, mats = uploaded
    rng = np.random.default_rng(20252)
    kinds, rays, recs, (q, nb) = scatter_cases(rng, mats)
    assert len(kinds) == N and rays.shape == (N, 7) and recs.shape == (N, 11)
    keys = np.stack([np.full(N, 13), np.arange(N) * 3 + 1, np.arange(N) % 5], 1).astype(np.uint32)

    want, want_draws = np.zeros((N, 11)), np.zeros(N, np.uint64)
    lib, res, em, draws = orc.lib(), (C.c_double * 10)(), (C.c_double * 3)(), C.c_uint64()
    for k in range(N):
        ray, rec = (C.c_double * 7)(*rays[k]), (C.c_double * 11)(*recs[k])
        want[k, 0] = lib.orc_kat_scatter(scene.desc_ptr, int(kinds[k]), C.addressof(ray), C.addressof(rec), int(keys[k, 0]), int(keys[k, 1]), int(keys[k, 2]),
                                         C.addressof(res), C.addressof(em), C.byref(draws))
        want[k, 1:11] = res[:]
        want_draws[k] = draws.value
    got, got_draws = renderer.debug_scatter(kinds, rays, recs, keys)

    sc = want[:, 0] == 1
    glass_edges = slice(q, q + nb)
    assert sc[glass_edges].all() and (want_draws[glass_edges] <= 1).all()      # a dielectric always scatters, with at most Schlick's draw
    assert (want_draws[glass_edges] == 0).sum() > nb // 8                      # total internal reflection took part (no draw)
    assert 0.05 < (~sc[:q]).mean() < 0.6                                       # fuzzed metal: absorbed below the surface, both outcomes
    assert np.isfinite(want[sc, 1:11]).all()
    assert np.array_equal(got[:, 0], want[:, 0])
    assert same_bits(got[sc, 1:11], want[sc, 1:11]).all(), np.argwhere(~same_bits(got[sc, 1:11], want[sc, 1:11]))[:5]
    assert np.array_equal(got_draws, want_draws)


def test_lean_kernel_small_frame_in_both_orders(rt, orc, renderer):
    """book1_final at 64x64, 8 spp, through the lean MIXED kernel and through the reference-order kernel: the bytes of both equal
    the oracle's, and the two linear images each other."""
    scene = rt.Scene.build("book1_final", SCENE_SEED, scene_file("book1_final", GOLDEN))
    cam = scene.camera(64, 64, 8, 50)
    ref, ref8, _ = orc.render(scene.desc_ptr, cam, RENDER_SEED, 8)
    renderer.upload(scene)
    base, base8, _ = renderer.render_host(cam)
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"] and "double, 256u" in renderer.kernel_name()
    fast, fast8, _ = renderer.render_host(cam)
    assert np.array_equal(base8, ref8) and np.array_equal(fast8, ref8)
    assert np.array_equal(fast, base)
    assert float(np.sqrt(np.mean((fast - ref) ** 2))) < 1e-12
