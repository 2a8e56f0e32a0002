"""Rich analytic inputs for the post-processing rules (a-trous filter, temporal accumulation, guided upsampling).

The scene is tests/test_temporal.py's: ground y = 0 (|x|, |z| < 8), wall x = -3 (0 < y < 3, |z| < 4), unit sphere at (0, 1, 0), seen
by a real pinhole camera.  First-hit depth is the true distance along the pixel's ray.  Every other guide channel is a
deterministic function of the world hit point (of the ray direction where noted), so the views of a moved camera and of a low
camera agree about the world:
  hit fractions   2x2 sub-pixel coverage of the scene, {0, 0.25, 0.5, 0.75, 1} at silhouettes
  mean normals    a bumped ground and wall and the sphere, times a smooth length in [0.3, 1]
  albedo          a smooth gradient, a checker edge and a few dark spots below the demodulation floor of 0.02
  set 2           the wall and the sphere are "mirrors": their own seen albedo (stripes whose step straddles the temporal
                  albedo_tol, plus a term of the ray direction), a tilted, varying end normal, a longer sloped path, an end-hit
                  fraction from {0, 0.25, .., 1} that differs from the first-hit fraction and is 0 near the wall's top; a patch of
                  sky (by ray direction) has first hit 0 and end hit 0.5.  Elsewhere set 2 is set 1 bit for bit.
Nothing here touches a device or the package: a view is a dict of numpy vectors."""
import numpy as np

SPHERE = np.array([0.0, 1.0, 0.0])
# The 2x2 sub-pixel positions are the pixel centre -+ SUB.  Which silhouette pixels are covered decides which taps of the temporal
# rule lie within 1e-3 of a threshold; with 0.3 (not 0.25) no 8x8 frame of the camera paths has more than the one such pixel
# the comparison may leave out (tests/test_temporal.py, fragile_cap).
SUB = 0.3


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def pinhole(w, h, lookfrom=(0.0, 2.0, 6.0), lookat=(0.0, 1.0, 0.0), vfov=40.0):
    """The view of a pinhole camera (the book's construction): {"center", "p00", "du", "dv", "w", "h"}."""
    lookfrom, lookat = np.asarray(lookfrom, np.float64), np.asarray(lookat, np.float64)
    focus = np.sqrt(((lookfrom - lookat) ** 2).sum())
    vh = 2.0 * np.tan(np.radians(vfov) / 2.0) * focus
    vw = vh * w / h
    back = _unit(lookfrom - lookat)
    right = _unit(np.cross([0.0, 1.0, 0.0], back))
    up = np.cross(back, right)
    du, dv = vw * right / w, -vh * up / h
    p00 = lookfrom - focus * back - (vw * right - vh * up) / 2.0 + 0.5 * (du + dv)
    return {"center": lookfrom, "p00": p00, "du": du, "dv": dv, "w": w, "h": h}


def view_of(cam):
    """The view of an rtk_camera."""
    v = lambda a: np.array([a.x, a.y, a.z], np.float64)  # noqa: E731
    return {"center": v(cam.center), "p00": v(cam.pixel00_loc), "du": v(cam.pixel_delta_u), "dv": v(cam.pixel_delta_v), "w": cam.image_width, "h": cam.image_height}


def _trace(o, d):
    """Closest hit of unit directions d (.., 3) from o: (surface 0 none / 1 ground / 2 wall / 3 sphere, t, point)."""
    best = np.full(d.shape[:-1], np.inf)
    surf = np.zeros(d.shape[:-1], np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = -o[1] / d[..., 1]
        p = o + t[..., None] * d
        ok = (t > 0) & (np.abs(p[..., 0]) < 8) & (np.abs(p[..., 2]) < 8)
        best, surf = np.where(ok, t, best), np.where(ok, 1, surf)
        t = (-3.0 - o[0]) / d[..., 0]
        p = o + t[..., None] * d
        ok = (t > 0) & (t < best) & (p[..., 1] > 0) & (p[..., 1] < 3) & (np.abs(p[..., 2]) < 4)
        best, surf = np.where(ok, t, best), np.where(ok, 2, surf)
        oc = o - SPHERE
        bq = (d * oc).sum(-1)
        disc = bq * bq - ((oc * oc).sum() - 1.0)
        t = -bq - np.sqrt(disc)
        ok = (disc > 0) & (t > 0) & (t < best)
        best, surf = np.where(ok, t, best), np.where(ok, 3, surf)
    t = np.where(surf > 0, best, 0.0)
    return surf, t, o + t[..., None] * d


def _quarter(x):
    return np.clip(np.round(4.0 * x) / 4.0, 0.0, 1.0)


def rich_guides(view):
    """Guides (H, W, 16) float32 of the analytic scene as described at the top."""
    h, w, o = view["h"], view["w"], view["center"]
    jj, ii = np.mgrid[0:h, 0:w].astype(np.float64)

    def rays(oi, oj):
        return _unit(view["p00"] + (ii + oi)[..., None] * view["du"] + (jj + oj)[..., None] * view["dv"] - o)

    d = rays(0.0, 0.0)
    surf, t, p = _trace(o, d)
    cover = np.zeros((h, w))
    for oj in (-SUB, SUB):
        for oi in (-SUB, SUB):
            s_surf, s_t, s_p = _trace(o, rays(oi, oj))
            cover += (s_surf > 0) / 4.0
            take = (surf == 0) & (s_surf > 0)                     # the centre misses: the first sub-sample that hits stands for the pixel
            surf, t, p = np.where(take, s_surf, surf), np.where(take, s_t, t), np.where(take[..., None], s_p, p)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    ground, wall, sphere = surf == 1, surf == 2, surf == 3
    mirror = wall | sphere

    # first albedo: a gradient per channel, a checker edge, dark spots
    base = np.stack([0.55 + 0.25 * np.sin(0.9 * x + 0.3 * z + 0.5 * y), 0.5 + 0.25 * np.sin(0.5 * x - 0.8 * z + 1.0 + 0.7 * y),
                     0.45 + 0.25 * np.sin(0.4 * x + 0.6 * z + 2.0 - 0.6 * y)], -1)
    checker = (np.floor(x / 1.5 + 0.25) + np.floor(z / 1.5) + np.floor(y / 0.9)) % 2 == 0
    a1 = base * np.where(checker, 0.6, 1.0)[..., None]
    dark = np.sin(2.1 * x + 0.4) * np.sin(1.7 * z + 1.9 * y) > 0.93
    a1 = np.where(dark[..., None], [0.012, 0.008, 0.015], a1)

    # first normal: bumps on the ground and the wall, the sphere's own; length in [0.3, 1]
    bump_g = np.stack([0.22 * np.cos(1.6 * x), np.ones_like(x), 0.22 * np.cos(1.3 * z + 0.5)], -1)
    bump_w = np.stack([np.ones_like(x), 0.2 * np.cos(2.0 * y), 0.2 * np.cos(1.4 * z)], -1)
    n1 = np.where(ground[..., None], bump_g, np.where(wall[..., None], bump_w, p - SPHERE))
    length = 0.65 + 0.35 * np.sin(1.1 * x + 0.7 * y + 0.9 * z)
    with np.errstate(invalid="ignore"):
        n1 = _unit(n1) * length[..., None]

    # set 2 inside the mirrors
    stripes = np.floor(1.1 * z + 0.9 * y + 0.4 * x) % 2 == 0
    step = 0.25 + 0.12 * np.sin(0.8 * z + 1.7 * y)               # the stripes' step straddles albedo_tol = 0.25
    a2 = np.stack([0.35 + 0.2 * np.sin(0.7 * z + 0.9 * y), 0.4 + 0.2 * np.sin(1.2 * y - 0.5 * z + 0.4 * x), 0.45 + 0.2 * np.sin(0.6 * z + 2.0 + 0.5 * x)], -1)
    a2 = a2 + np.where(stripes, step, 0.0)[..., None] * [1.0, 0.6, 0.3] + 0.2 * np.sin(6.0 * d[..., 0:1] + 4.0 * d[..., 2:3] + [0.0, 1.0, 2.0])
    a2 = np.clip(a2, 0.0, 1.0)
    a2 = np.where((np.sin(2.6 * z + 0.3) * np.sin(2.2 * y + 1.0 + x) > 0.93)[..., None], [0.01, 0.015, 0.005], a2)
    n2 = np.stack([0.6 + 0.25 * np.sin(1.5 * y + 0.4 * z), 0.3 * np.sin(1.2 * z + x), 0.8 + 0.2 * np.cos(1.7 * y - 0.6 * z)], -1)
    len2_n = 0.65 + 0.35 * np.sin(0.8 * x - 1.3 * y + 1.1 * z + 1.0)
    n2 = _unit(n2) * len2_n[..., None]
    path = t + 3.0 + 0.6 * y + 0.35 * (z + 4.0) + 0.5 * x
    hit2 = np.maximum(_quarter(0.65 + 0.45 * np.sin(1.3 * z + 2.1 * y + 0.7 * x)), 0.25)
    hit2 = np.where(wall & (y > 2.45), 0.0, hit2)                  # the mirror shows the sky: first hit > 0, end hit 0

    g = np.zeros((h, w, 16))
    hit = cover > 0
    g[..., 0:3], g[..., 3], g[..., 4:7], g[..., 7] = a1, cover, n1, t
    g[~hit, 0:8] = 0.0
    g[..., 8:16] = g[..., 0:8]
    seen_end = mirror & (hit2 > 0)
    g[mirror, 8:11] = a2[mirror]
    g[mirror, 11] = hit2[mirror]
    g[mirror, 12:16] = 0.0
    g[seen_end, 12:15] = n2[seen_end]
    g[seen_end, 15] = path[seen_end]
    # a patch of sky, by ray direction: first hit 0, end hit 0.5
    patch = ~hit & (d[..., 0] > 0.12) & (d[..., 1] > -0.1)
    g[patch, 8:11] = np.stack([0.5 + 0.3 * np.sin(9.0 * d[..., 0]), 0.5 + 0.3 * np.sin(7.0 * d[..., 1] + 1.0), 0.4 + 0.3 * np.sin(5.0 * d[..., 0] + 8.0 * d[..., 1])], -1)[patch]
    g[patch, 11] = 0.5
    g[patch, 12:15] = (0.5 * _unit(np.stack([np.sin(8.0 * d[..., 0]), np.cos(6.0 * d[..., 1]), np.ones_like(x)], -1)))[patch]
    g[patch, 15] = (9.0 + 12.0 * d[..., 0] + 6.0 * d[..., 1])[patch]
    return g.astype(np.float32)


def shade(g):
    """A clean colour for guides g: the seen albedo under a smooth light (0.35 .. 1.15, by first-hit depth and normal)."""
    g = g.astype(np.float64)
    return g[..., 8:11] * (0.75 + 0.25 * np.sin(0.8 * g[..., 7:8]) + 0.15 * g[..., 5:6])


def rich_filter_case(h=48, w=64, seed=5):
    """(noisy colour float64, guides (H, W, 16) float32, se float32) for the a-trous filter at any size: se varies per pixel.  The
    filter needs no particular camera; this one stands nearer with a wider angle, which puts more pixels around the sphere's
    nearest point, the only place where the 1e-3 z_p term of w_z outweighs the depth gradient."""
    rng = np.random.default_rng(seed)
    g = rich_guides(pinhole(w, h, lookfrom=(0.5, 2.2, 4.5), vfov=50.0))
    se = (0.03 + 0.1 * rng.random((h, w)) ** 2).astype(np.float32)
    return shade(g) + rng.normal(0.0, 1.0, (h, w, 3)) * se[..., None], g, se
