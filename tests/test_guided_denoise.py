"""Guides that follow mirrors and albedo demodulation (rtk_render_guides, rtk_denoise_guided, rtk_progressive_denoise_guided).

CPU tests: the entry points are declared and exported; option refusals need no device; the numpy restatement of the guided filter
below with set 2 := set 1 is reference_denoise exactly; run on the oracle-rendered test room (guide chains composed from
orc_kat_get_ray / _node_hit / _scatter / _texture) it lowers the error on the mirror, on the textured wall and over the image.
GPU tests (-m gpu): guides equal the composition of the known-answer entry points bit for bit and their first half is
rtk_render_aovs; without anything to follow the guided filter is rtk_denoise bit for bit; the filter matches the restatement; the
error ratios on the device; sessions; caller streams; refusals; the C++ camera."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import EARTH, ROOT
from tests.desc_builder import (MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC, MAT_LAMBERTIAN, MAT_METAL, MAT_SPECULAR, DescBuilder, SceneDesc)
from tests.test_denoise import (BINOMIAL3, DEFAULTS, H5, RAGGED, RICH_OPTIONS, _aov_of_samples, _clamped, _read_png, _shift, _synthetic, _to_byte, reference_denoise)

ENTRY_POINTS = ("rtk_render_guides", "rtk_render_guides_host", "rtk_denoise_guided", "rtk_denoise_guided_host", "rtk_progressive_denoise_guided",
                "rtk_progressive_denoise_guided_host")
MIRROR, DIELECTRIC = 1, 2


# ------------------------------------------------------------------------------------------------------ numpy reference --
# Deliberate one-term deviations from the rule: what a subtly wrong kernel would compute.  tests/test_rule_sensitivity.py shows
# that the device comparison's inputs tell each of them from the rule; none is ever run against the device.
VARIANTS = ("cos_without_lengths", "no_z_term", "gradient_min", "hit_below_1", "wn_set1_only", "wz_set1_only", "wz2_with_hit1", "wz2_with_grad1",
            "wa_first_albedo", "gv_centre", "variance_w", "floor_0", "variance_per_channel")


def reference_denoise_guided(linear, guides, noise, demodulate=False, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, sigma_a=0.1, variant=None):
    """include/rtk.h, rtk_denoise_guided, in float64 (reference_denoise's conventions).  variant: one of VARIANTS, a deliberately
    wrong rule."""
    assert variant is None or variant in VARIANTS, variant
    c = np.asarray(linear, np.float32).astype(np.float64)
    se = np.asarray(noise, np.float32)
    var = (se * se).astype(np.float64)
    g = np.asarray(guides, np.float32).astype(np.float64)
    seen = g[..., 8:11]
    sets = []
    for hit, nrm, z in ((g[..., 3], g[..., 4:7], g[..., 7]), (g[..., 11], g[..., 12:15], g[..., 15])):
        zx, zy = np.abs(_clamped(z, 0, 1) - _clamped(z, 0, -1)), np.abs(_clamped(z, 1, 0) - _clamped(z, -1, 0))
        grad = (np.minimum(zx, zy) if variant == "gradient_min" else np.maximum(zx, zy)) / 2
        sets.append((hit, nrm, z, grad, np.all(nrm == 0, axis=-1), np.sqrt((nrm * nrm).sum(-1))))
    if variant == "wz2_with_hit1":
        sets[1] = (sets[0][0],) + sets[1][1:]
    if variant == "wz2_with_grad1":
        sets[1] = sets[1][:3] + (sets[0][3],) + sets[1][4:]
    floor = 0.0 if variant == "floor_0" else 0.02
    if demodulate:
        A = np.maximum(seen, floor)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = c / A
            var = (var[..., None] / A ** 2).mean(-1) if variant == "variance_per_channel" else var / ((A[..., 0] + A[..., 1] + A[..., 2]) / 3) ** 2
    wa_of = g[..., 0:3] if variant == "wa_first_albedo" else seen
    z_term = 0.0 if variant == "no_z_term" else 1e-3
    for k in range(iterations):
        step = 2 ** k
        gv = sum(BINOMIAL3[b + 1] * BINOMIAL3[a + 1] * _clamped(var, b, a) for b in (-1, 0, 1) for a in (-1, 0, 1))
        if variant == "gv_centre":
            gv = var
        y = (c[..., 0] + c[..., 1] + c[..., 2]) / 3
        lden = sigma_l * np.sqrt(np.maximum(gv, 0)) + 1e-6
        sw, sc, sv = np.zeros(y.shape), np.zeros(c.shape), np.zeros(y.shape)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = step * dy, step * dx
                cq, valid = _shift(c, oy, ox)
                vq, _ = _shift(var, oy, ox)
                yq = (cq[..., 0] + cq[..., 1] + cq[..., 2]) / 3
                wl = np.exp(-np.abs(y - yq) / lden)
                o = step * np.sqrt(dx * dx + dy * dy)
                wn = wz = None
                for hit, nrm, z, grad, nzero, nlen in sets:
                    hq, _ = _shift(hit, oy, ox)
                    nq, _ = _shift(nrm, oy, ox)
                    zq, _ = _shift(z, oy, ox)
                    nqzero = np.all(nq == 0, axis=-1)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        cos = (nrm * nq).sum(-1) / (nlen * np.sqrt((nq * nq).sum(-1)))
                        if variant == "cos_without_lengths":
                            cos = (nrm * nq).sum(-1)
                        wn_s = np.where(nzero & nqzero, 1.0, np.where(nzero | nqzero, 0.0, np.maximum(0.0, np.nan_to_num(cos)) ** sigma_n))
                        wz_s = np.exp(-np.abs(z - zq) / (sigma_z * (grad * o + z_term * z) + 1e-6))
                    wz_s = np.where(((hit < 1) | (hq < 1)) if variant == "hit_below_1" else ((hit == 0) | (hq == 0)), 1.0, wz_s)
                    wn = wn_s if wn is None else (wn if variant == "wn_set1_only" else np.minimum(wn, wn_s))
                    wz = wz_s if wz is None else (wz if variant == "wz_set1_only" else np.minimum(wz, wz_s))
                if demodulate:
                    wa = 1.0
                else:
                    aq, _ = _shift(wa_of, oy, ox)
                    wa = np.exp(-np.sqrt(((wa_of - aq) ** 2).sum(-1)) / sigma_a)
                w = np.where(valid, H5[dx + 2] * H5[dy + 2] * wl * wn * wz * wa, 0.0)
                sw += w
                sc += w[..., None] * cq
                sv += (w if variant == "variance_w" else w * w) * vq
        with np.errstate(invalid="ignore", divide="ignore"):
            c = sc / sw[..., None]
            var = sv / (sw * sw)
    return c * np.maximum(seen, floor) if demodulate else c


def _doubled(aov):
    """Guides whose second set is the first."""
    return np.concatenate([aov, aov], -1)


def _synthetic_guides(h=48, w=64, seed=5):
    """_synthetic with a second set that differs from the first inside a `mirror` rectangle: another albedo pattern, a tilted
    normal and a longer, sloped path; one column of it without end hits."""
    noisy, aov, se = _synthetic(h, w, seed)
    g = _doubled(aov)
    jj, ii = np.mgrid[0:h, 0:w]
    m = (ii >= w // 4) & (ii < w // 4 + max(1, w // 3)) & (jj >= h // 3)
    g[m, 8:11] = np.where(((ii + 2 * jj) % 7 < 3)[..., None], [0.7, 0.7, 0.2], [0.2, 0.3, 0.6])[m].astype(np.float32)
    g[m, 12:15] = np.float32([0.6, 0.0, 0.8])
    g[m, 15] = (6.0 + 0.03 * jj + 0.002 * ii * ii)[m].astype(np.float32)
    g[m & (ii == w // 4 + 1), 11:16] = 0
    return noisy, g, se


# ----------------------------------------------------------------------------------------------- the guide composition --
def compose_guides(be, mats, background, W, seed, ijs, follow, max_bounces, real):
    """include/rtk.h, rtk_render_guides, per (i, j, s) of ijs, from the four known-answer operations of backend `be`: get_ray
    (ijs) -> [n, 7]; hit(rays [n, 9], keys) -> [n, 12] = hit, t, p, normal, front_face, u, v, material; scatter(materials, rays
    [n, 7], records [n, 11], keys) -> [n, 11] = scattered, origin, direction, attenuation, time; texture(ids, uvp [n, 5]) ->
    [n, 3].  Returns the per-sample terms [n, 16] as `real` (k 3 / 11 are hit flags, k 7 / 15 the sample's length) and the first-hit
    material [n] (-1 on a miss)."""
    n = len(ijs)
    ijs64 = ijs.astype(np.int64)
    pixel, s = ijs64[:, 1] * W + ijs64[:, 0], ijs64[:, 2]
    rays = be.get_ray(ijs).copy()
    out = np.zeros((n, 16), real)
    first_mat = np.full(n, -1)
    T, length = np.ones((n, 3), real), np.zeros(n, real)
    miss = np.array([min(max(real(v), real(0)), real(1)) for v in background], real)
    live = np.arange(n)
    for b in range(max_bounces + 1):
        if live.size == 0:
            break
        m_ = live.size
        rays9 = np.concatenate([rays[live], np.full((m_, 1), 0.001), np.full((m_, 1), np.inf)], 1)
        keys = np.stack([np.full(m_, seed), pixel[live], 2 ** 31 + ((2 * b) << 20) + s[live]], 1).astype(np.uint32)
        rec = be.hit(rays9, keys)
        hit = rec[:, 0] != 0
        mat = np.where(hit, rec[:, 11], -1).astype(np.int64)
        kind = np.array([mats[k].kind if k >= 0 else 0 for k in mat])
        a, nrm = np.zeros((m_, 3), real), np.zeros((m_, 3), real)
        a[~hit] = miss
        tex_rows, tex_ids = [], []
        for r in np.flatnonzero(hit):
            m = mats[mat[r]]
            if m.kind in (MAT_LAMBERTIAN, MAT_ISOTROPIC, MAT_DIFFUSE_LIGHT) and m.texture >= 0:
                tex_rows.append(r)
                tex_ids.append(m.texture)
            elif m.kind == MAT_DIELECTRIC:
                a[r] = 1
            else:
                assert m.kind in (MAT_METAL, MAT_SPECULAR, MAT_LAMBERTIAN, MAT_DIFFUSE_LIGHT), m.kind
                a[r] = np.array([m.albedo.x, m.albedo.y, m.albedo.z]).astype(real)
        if tex_rows:
            a[tex_rows] = be.texture(np.array(tex_ids), rec[tex_rows][:, [9, 10, 2, 3, 4]]).astype(real)
        light = kind == MAT_DIFFUSE_LIGHT
        a[light] = np.minimum(a[light], real(1))
        keep_n = hit & (kind != MAT_ISOTROPIC)
        nrm[keep_n] = rec[keep_n, 5:8].astype(real)
        d = rays[live, 3:6].astype(real)
        seg = np.where(hit, rec[:, 1].astype(real) * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), real(0)).astype(real)
        length[live] = length[live] + seg
        if b == 0:
            out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = a, hit, nrm, seg
            first_mat = mat.copy()
        fuzz0 = np.array([k >= 0 and real(mats[k].param) == 0 for k in mat])
        followed = hit & (b < max_bounces) & ((bool(follow & MIRROR) & (kind == MAT_METAL) & fuzz0) | (bool(follow & DIELECTRIC) & (kind == MAT_DIELECTRIC)))
        cont = np.zeros(m_, bool)
        idx = np.flatnonzero(followed)
        if idx.size:
            keys2 = keys[idx].copy()
            keys2[:, 2] += np.uint32(1 << 20)
            sc = be.scatter(mat[idx], rays[live[idx]], rec[idx, 1:12], keys2)
            ok = sc[:, 0] != 0
            go = live[idx[ok]]
            T[go] = T[go] * sc[ok, 7:10].astype(real)
            rays[go, 0:6] = sc[ok, 1:7]
            cont[idx[ok]] = True
        end = ~cont
        e = live[end]
        out[e, 8:11] = T[e] * a[end]
        out[e, 11] = hit[end]
        out[e, 12:15] = nrm[end]
        out[e, 15] = np.where(hit[end], length[e], real(0))
        live = live[cont]
    assert live.size == 0
    return out, first_mat


def guides_of_samples(comp, real):
    """What rtk_render_guides writes for per-sample terms comp [pixels, n, 16]: each half by rtk_render_aovs' rule."""
    return np.concatenate([_aov_of_samples(comp[..., 0:8], real), _aov_of_samples(comp[..., 8:16], real)], 1)


class DeviceBackend:
    def __init__(self, renderer, cam, seed, real_mode):
        self.r, self.cam, self.seed, self.mode = renderer, cam, seed, real_mode

    def get_ray(self, ijs):
        return self.r.debug_get_ray(self.cam, self.seed, ijs, self.mode)[0]

    def hit(self, rays9, keys):
        return self.r.closest_hit(rays9, keys, self.mode)[0]

    def scatter(self, mat, rays, recs, keys):
        return self.r.debug_scatter(mat, rays, recs, keys, self.mode)[0][:, 0:11]

    def texture(self, ids, uvp):
        return self.r.debug_texture(ids, uvp, self.mode)[0]


class OracleBackend:
    def __init__(self, orc, desc_ptr, root, cam, seed):
        self.lib, self.desc, self.root, self.cam, self.seed = orc.lib(), desc_ptr, root, cam, seed

    def get_ray(self, ijs):
        out, res = np.zeros((len(ijs), 7)), (C.c_double * 7)()
        for k, (i, j, s) in enumerate(ijs.tolist()):
            self.lib.orc_kat_get_ray(C.addressof(self.cam), self.seed, i, j, s, C.addressof(res), None)
            out[k] = res[:]
        return out

    def hit(self, rays9, keys):
        out, rec = np.zeros((len(rays9), 12)), (C.c_double * 11)()
        for k, (row, key) in enumerate(zip(rays9, keys.tolist())):
            ray = (C.c_double * 7)(*row[0:7])
            if self.lib.orc_kat_node_hit(self.desc, self.root, C.addressof(ray), float(row[7]), float(row[8]), key[0], key[1], key[2], C.addressof(rec), None):
                out[k, 0] = 1
                out[k, 1:12] = rec[:]
            else:
                out[k, 11] = -1
        return out

    def scatter(self, mat, rays, recs, keys):
        out, res, em = np.zeros((len(mat), 11)), (C.c_double * 10)(), (C.c_double * 3)()
        for k in range(len(mat)):
            ray, rec = (C.c_double * 7)(*rays[k]), (C.c_double * 11)(*recs[k])
            key = keys[k].tolist()
            out[k, 0] = self.lib.orc_kat_scatter(self.desc, int(mat[k]), C.addressof(ray), C.addressof(rec), key[0], key[1], key[2], C.addressof(res),
                                                 C.addressof(em), None)
            out[k, 1:11] = res[:]
        return out

    def texture(self, ids, uvp):
        out, res = np.zeros((len(ids), 3)), (C.c_double * 3)()
        for k in range(len(ids)):
            p = (C.c_double * 3)(*uvp[k, 2:5])
            self.lib.orc_kat_texture(self.desc, int(ids[k]), float(uvp[k, 0]), float(uvp[k, 1]), C.addressof(p), C.addressof(res))
            out[k] = res[:]
        return out


def _materials(scene):
    desc = C.cast(C.c_void_p(scene.desc_ptr), C.POINTER(SceneDesc)).contents
    return [desc.materials[k] for k in range(desc.n_materials)], desc.root


def _all_samples(w, h, n):
    return np.array([[p % w, p // w, s] for p in range(w * h) for s in range(n)], np.int32)


# -------------------------------------------------------------------------------------------------------- the test room --
ROOM_MATERIALS = ("white", "red", "blue", "checker", "noise", "mirror", "glass", "light")


def build_test_room():
    """A room with a mirror wall, a Perlin-textured wall, a checker floor, a glass and a blue sphere under an area light."""
    rnd = random.Random(3)
    b = DescBuilder()
    white, red, blue = b.lambertian((.73, .73, .73)), b.lambertian((.65, .05, .05)), b.lambertian((.1, .2, .7))
    checker = b.textured(b.checker(0.5, b.solid((.2, .3, .1)), b.solid((.9, .9, .9))))
    noise = b.textured(b.noise(4.0, rnd))
    mirror, glass, light = b.metal((.9, .9, .9), 0.0), b.dielectric(1.5), b.light((6, 6, 6))
    assert (white, red, blue, checker, noise, mirror, glass, light) == tuple(range(8))
    nodes = [b.quad((0, 0, 0), (4, 0, 0), (0, 0, -4), checker), b.quad((0, 3, 0), (4, 0, 0), (0, 0, -4), white),
             b.quad((1, 2.99, -1), (2, 0, 0), (0, 0, -2), light), b.quad((0, 0, -4), (4, 0, 0), (0, 3, 0), noise),
             b.quad((0, 0, 0), (0, 0, -4), (0, 3, 0), mirror), b.quad((4, 0, 0), (0, 0, -4), (0, 3, 0), red),
             b.sphere((2.8, .6, -1.5), .6, glass), b.sphere((1.3, .5, -2.5), .5, blue)]
    return b.finish(b.list(nodes))


def room_camera(rt, width=160, spp=32):
    return rt.derive_camera(width, 1.0, spp=spp, max_depth=10, vfov=55, lookfrom=(2.6, 1.5, 3.0), lookat=(1.4, 1.1, -2.0))


def _regions(first_mat, names):
    """Pixels all of whose guide samples first hit material `name`: first_mat [H, W, n]."""
    return {name: np.all(first_mat == ROOM_MATERIALS.index(name), axis=-1) for name in names}


def _ratios(noisy, truth, outputs, regions):
    """MSE ratio output / noisy over the image ("all") and each region, per output."""
    err_noisy = ((noisy - truth) ** 2).sum(-1)
    res = {}
    for key, img in outputs.items():
        err = ((img - truth) ** 2).sum(-1)
        res[key] = {"all": float(err.mean() / err_noisy.mean())}
        res[key].update({name: float(err[m].mean() / err_noisy[m].mean()) for name, m in regions.items()})
    return res


def _se_from_chunk_means(chunk_rgb):
    """The progressive session's per-pixel standard error (tests/test_progressive.py) from K chunk means [K, H, W, 3]."""
    y = (chunk_rgb[..., 0] + chunk_rgb[..., 1] + chunk_rgb[..., 2]) / 3.0
    K = y.shape[0]
    m = y.sum(0) / K
    return np.sqrt(np.maximum(0.0, ((y * y).sum(0) - K * m * m) / (K - 1)) / K)


# Bounds = the ratios measured on the CPU restatement (printed by the test) + 15 %, the margin tests/test_denoise.py uses.
CPU_ROOM_BOUNDS = {("guided", "mirror"): 0.4952, ("demodulated", "noise"): 0.0936, ("demodulated", "all"): 0.3369, ("guided", "all"): 0.4839}


@pytest.fixture(scope="module")
def cpu_room(rt, orc):
    """The test room rendered by the oracle at 160x160: 32 spp of seed 1 with the se of its four 8-sample chunks (the chunk
    means from the differences of 8-, 16-, 24- and 32-spp frames: the same samples), the truth of 1024 spp of seed 1001, and the
    4-sample guides (follow = mirrors; first-hit material per sample for the region masks)."""
    scene = build_test_room()
    mats, root = _materials(scene)
    w = h = 160
    acc = [orc.render(scene.desc_ptr, room_camera(rt, w, n), 1)[0] * n for n in (8, 16, 24, 32)]
    chunks = np.stack([acc[0]] + [acc[k] - acc[k - 1] for k in (1, 2, 3)]) / 8.0
    noisy = acc[3] / 32.0
    se = _se_from_chunk_means(chunks).astype(np.float32)
    truth = orc.render(scene.desc_ptr, room_camera(rt, w, 1024), 1001)[0]
    cam = room_camera(rt, w, 32)
    be = OracleBackend(orc, scene.desc_ptr, root, cam, 1)
    bg = (cam.background.x, cam.background.y, cam.background.z)
    comp, first = compose_guides(be, mats, bg, w, 1, _all_samples(w, h, 4), MIRROR, 4, np.float64)
    guides = guides_of_samples(comp.reshape(w * h, 4, 16), np.float64).reshape(h, w, 16)
    return {"noisy": noisy, "se": se, "truth": truth, "guides": guides, "first": first.reshape(h, w, 4)}


# ---------------------------------------------------------------------------------------------------------------- CPU --
def test_header_declares_and_library_exports_the_guided_api(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, body), name
    assert re.search(r"typedef struct rtk_guide_opts\b", body)
    for name, value in (("RTK_GUIDE_FOLLOW_MIRROR", 1), ("RTK_GUIDE_FOLLOW_DIELECTRIC", 2), ("RTK_DENOISE_DEMODULATE", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), body), name
    assert "#define RTK_ABI_VERSION 2" in body
    lib = C.CDLL(rt.HIP_LIB_PATH)                          # loads without a GPU
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert C.sizeof(rt.GuideOpts) == 8
    assert (rt.GUIDE_FOLLOW_MIRROR, rt.GUIDE_FOLLOW_DIELECTRIC, rt.DENOISE_DEMODULATE) == (1, 2, 1)


def test_option_refusals_need_no_device(rt):
    """Options are checked before anything else: with no context at all, a bad option is what the error names."""
    lib = rt.hip_lib()
    err = lambda: lib.rtk_last_error().decode()  # noqa: E731
    cam = rt.derive_camera(16, 1.0)
    ro = rt.RenderOpts(1, 0, 0, 1, 0, 0, None)
    out = np.full((16, 16, 16), -7.0, np.float32)
    for gopts, n, word in ((rt.GuideOpts(4, 0), 4, "follow"), (rt.GuideOpts(-1, 0), 4, "follow"), (rt.GuideOpts(1, 9), 4, "max_bounces"),
                           (rt.GuideOpts(1, -1), 4, "max_bounces"), (rt.GuideOpts(0, 0), 0, "n_samples"), (rt.GuideOpts(3, 8), 2 ** 20 + 1, "n_samples"),
                           (rt.GuideOpts(3, 8), 2 ** 20, "null argument")):
        for f in (lib.rtk_render_guides, lib.rtk_render_guides_host):
            assert f(None, C.byref(cam), C.byref(ro), n, C.byref(gopts), out.ctypes.data) == -1
            assert word in err(), (word, err())
    assert np.all(out == -7.0)
    lin, noise = np.zeros((16, 16, 3)), np.zeros((16, 16), np.float32)
    o_lin = np.full((16, 16, 3), -3.0)
    ok = rt.DenoiseOpts(0, 0, 0, 0, 0, 0)
    for dn, flags, word in ((ok, 2, "flags"), (ok, -1, "flags"), (rt.DenoiseOpts(9, 0, 0, 0, 0, 0), 1, "iterations"), (ok, 1, "null context")):
        assert lib.rtk_denoise_guided_host(None, 16, 16, 0, lin.ctypes.data, out.ctypes.data, noise.ctypes.data, C.byref(dn), flags, o_lin.ctypes.data, None) == -1
        assert word in err(), (word, err())
        assert lib.rtk_denoise_guided(None, 16, 16, 0, lin.ctypes.data, out.ctypes.data, noise.ctypes.data, C.byref(dn), flags, o_lin.ctypes.data, None, None) == -1
        assert word in err(), (word, err())
    for g, dn, flags, word in ((rt.GuideOpts(8, 0), ok, 0, "follow"), (rt.GuideOpts(0, 12), ok, 0, "max_bounces"), (rt.GuideOpts(0, 0), ok, 4, "flags"),
                               (rt.GuideOpts(0, 0), rt.DenoiseOpts(0, -1, 0, 0, 0, 0), 0, "sigmas"), (rt.GuideOpts(0, 0), ok, 1, "null session")):
        assert lib.rtk_progressive_denoise_guided_host(None, 4, C.byref(g), C.byref(dn), flags, o_lin.ctypes.data, None) == -1
        assert word in err(), (word, err())
        assert lib.rtk_progressive_denoise_guided(None, 4, C.byref(g), C.byref(dn), flags, o_lin.ctypes.data, None) == -1
        assert word in err(), (word, err())
    assert np.all(o_lin == -3.0)


def test_guided_reference_with_equal_sets_is_the_first_hit_reference():
    noisy, aov, se = _synthetic()
    for opts in ({"iterations": 1}, {}, {"iterations": 8}, {"iterations": 3, "sigma_l": 2.0, "sigma_n": 32.0, "sigma_z": 0.5, "sigma_a": 0.3}):
        full = dict(DEFAULTS, **opts)
        assert np.array_equal(reference_denoise_guided(noisy, _doubled(aov), se, **full), reference_denoise(noisy, aov, se, **full))
    # the second set matters, and demodulation keeps an image that IS its albedo times a constant
    noisy, g, se = _synthetic_guides()
    assert not np.array_equal(reference_denoise_guided(noisy, g, se), reference_denoise(noisy, g[..., 0:8], se))
    flat = 0.375 * np.maximum(g[..., 8:11].astype(np.float64), 0.02)
    assert np.abs(reference_denoise_guided(flat, g, se, demodulate=True) - flat).max() < 1e-7  # (flat is rounded to float32 on the way in)


def test_guides_of_the_test_room_on_the_oracle(cpu_room):
    g, first = cpu_room["guides"], cpu_room["first"]
    regions = _regions(first, ROOM_MATERIALS)
    assert np.array_equal(g[~regions["mirror"] & ~regions["glass"] & np.all(first != 5, -1)][:, 8:16],
                          g[~regions["mirror"] & ~regions["glass"] & np.all(first != 5, -1)][:, 0:8])       # nothing followed: set 2 is set 1
    m = g[regions["mirror"]]
    assert len(m) > 0.2 * first.shape[0] * first.shape[1]
    assert np.all(m[:, 0:3] == np.float32(0.9)) and np.all(m[:, 15] > m[:, 7])       # one albedo at the first hit; the path goes on
    assert np.unique(m[:, 8:11], axis=0).shape[0] > 100                               # the mirror shows the room
    assert np.all(m[:, 8:11] <= np.float32(0.9))


def test_guided_filter_lowers_the_error_on_the_test_room(cpu_room):
    c = cpu_room
    regions = _regions(c["first"], ("mirror", "noise", "checker", "glass"))
    out = {"today": reference_denoise(c["noisy"], c["guides"][..., 0:8], c["se"]),
           "guided": reference_denoise_guided(c["noisy"], c["guides"], c["se"]),
           "demodulated": reference_denoise_guided(c["noisy"], c["guides"], c["se"], demodulate=True)}
    q = _ratios(c["noisy"], c["truth"], out, regions)
    print("test room, oracle:", json.dumps(q))
    assert q["guided"]["mirror"] < q["today"]["mirror"]
    assert q["demodulated"]["noise"] < q["today"]["noise"]
    assert q["demodulated"]["all"] < q["today"]["all"]
    for name in ("noise", "checker", "glass"):                   # first hit not followed: only taps that reach into the mirror differ
        assert abs(q["guided"][name] - q["today"][name]) <= 0.002, name
    for (key, name), measured in CPU_ROOM_BOUNDS.items():
        assert q[key][name] <= 1.15 * measured, (key, name, q[key][name])


# ---------------------------------------------------------------------------------------------------------------- GPU --
GUIDE_SCENES = [("book1_final", 40, 24, 6), ("book2_final", 32, 32, 6), ("material_zoo", 40, 24, 6), ("cornell_smoke", 32, 32, 6), ("mesh", 40, 24, 6),
                ("test_room", 40, 40, 6)]
# (follow, max_bounces): the cap at one followed hit, the default, glass as well, and the longest chain
GUIDE_OPTIONS = [(MIRROR, 1), (MIRROR, 4), (MIRROR | DIELECTRIC, 4), (MIRROR | DIELECTRIC, 8)]


@pytest.fixture(scope="module")
def scenes(rt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build_test_room() if name == "test_room" else rt.Scene.build(name, rt.SCENE_SEED, EARTH)
        return cache[name]
    return get


def _camera(rt, scene, name, w, h, spp, depth):
    if name == "test_room":
        assert w == h
        cam = room_camera(rt, w, spp)
        cam.max_depth = depth
        return cam
    return scene.camera(w, h, spp, depth)


def _composed(rt, renderer, scene, cam, seed, real_mode, ijs, follow, max_bounces):
    mats, _ = _materials(scene)
    real = np.float64 if real_mode == rt.RTK_REAL_F64 else np.float32
    bg = (cam.background.x, cam.background.y, cam.background.z)
    return compose_guides(DeviceBackend(renderer, cam, seed, real_mode), mats, bg, cam.image_width, seed, ijs, follow, max_bounces, real)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("order", ["reference", "fast"])
@pytest.mark.parametrize("case", GUIDE_SCENES, ids=[c[0] for c in GUIDE_SCENES])
def test_guides_equal_the_known_answer_composition(rt, renderer, scenes, case, order, real_mode):
    name, w, h, depth = case
    scene = scenes(name)
    cam = _camera(rt, scene, name, w, h, 8, depth)
    if order == "fast":
        renderer.upload_fast(scene, cam.center)
    else:
        renderer.upload(scene)
    seed = 7
    real = np.float64 if real_mode == 0 else np.float32
    aov = {n: renderer.aovs(cam, n, seed=seed, real_mode=real_mode) for n in (1, 4)}
    rng = np.random.default_rng(11)
    px = rng.choice(w * h, 75, replace=False)
    ijs = np.array([[p % w, p // w, s] for p in px for s in range(4)], np.int32)
    followed = 0
    for follow, max_bounces in GUIDE_OPTIONS:
        comp = _composed(rt, renderer, scene, cam, seed, real_mode, ijs, follow, max_bounces).reshape(len(px), 4, 16)
        for n in (1, 4):
            got = renderer.guides(cam, n, follow=follow, max_bounces=max_bounces, seed=seed, real_mode=real_mode)
            assert np.array_equal(got[..., 0:8], aov[n]), (follow, max_bounces, n)
            want = guides_of_samples(comp[:, 0:n], real)
            sel = got.reshape(-1, 16)[px]
            assert np.array_equal(sel, want), (follow, max_bounces, n, np.argwhere(sel != want)[:5])
            followed += int((got[..., 15] != got[..., 7]).sum())
    assert np.array_equal(renderer.guides(cam, 4, follow=0, max_bounces=0, seed=seed, real_mode=real_mode),
                          renderer.guides(cam, 4, follow=MIRROR, max_bounces=4, seed=seed, real_mode=real_mode))        # the defaults
    if name in ("book1_final", "test_room"):
        assert followed > 0


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["material_zoo", "cornell_smoke", "book2_final"])
def test_guides_at_ragged_and_degenerate_sizes(rt, renderer, scenes, name, real_mode):
    """Every pixel at image sizes whose last tile row and column are partial, for one sample and a count that is no power of two."""
    scene = scenes(name)
    renderer.upload(scene)
    real = np.float64 if real_mode == 0 else np.float32
    hits = 0
    for w, h in RAGGED:
        cam = scene.camera(w, h, 8, 6)
        for n in (1, 5):
            got = renderer.guides(cam, n, follow=MIRROR | DIELECTRIC, seed=7, real_mode=real_mode)
            comp = _composed(rt, renderer, scene, cam, 7, real_mode, _all_samples(w, h, n), MIRROR | DIELECTRIC, 4).reshape(w * h, n, 16)
            want = guides_of_samples(comp, real).reshape(h, w, 16)
            assert np.array_equal(got, want), (w, h, n, np.argwhere(got != want)[:5])
            assert np.array_equal(got[..., 0:8], renderer.aovs(cam, n, seed=7, real_mode=real_mode))
            hits += int((got[..., 11] > 0).sum())
    assert hits > 0


def _preview(rt, renderer, scenes, name, w, h, spp=32, real_mode=0, depth=10):
    scene = scenes(name)
    renderer.upload(scene)
    cam = _camera(rt, scene, name, w, h, spp, depth)
    p = renderer.progressive(cam, real_mode=real_mode)
    linear, _, noise = p.step(spp)
    p.close()
    return cam, linear, noise


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_nothing_to_follow_gives_the_first_hit_filter_bit_for_bit(rt, renderer, scenes, real_mode):
    cam, linear, noise = _preview(rt, renderer, scenes, "cornell_box", 72, 52, real_mode=real_mode)
    aov = renderer.aovs(cam, 4, real_mode=real_mode)
    for follow in (MIRROR, MIRROR | DIELECTRIC):
        g = renderer.guides(cam, 4, follow=follow, real_mode=real_mode)
        assert np.array_equal(g[..., 0:8], aov) and np.array_equal(g[..., 8:16], aov)
    for opts in ({}, {"iterations": 1}, {"iterations": 8, "sigma_a": 0.3}):
        want, want8 = renderer.denoise(linear, aov, noise, real_mode=real_mode, **opts)
        got, got8 = renderer.denoise_guided(linear, g, noise, real_mode=real_mode, **opts)
        assert np.array_equal(got, want) and np.array_equal(got8, want8), opts
    # and on guides that are only formally double: the synthetic image with its hard edges
    noisy, a, se = _synthetic(75, 100)
    want, want8 = renderer.denoise(noisy, a, se, real_mode=real_mode)
    got, got8 = renderer.denoise_guided(noisy, _doubled(a), se, real_mode=real_mode)
    assert np.array_equal(got, want) and np.array_equal(got8, want8)


@pytest.fixture(scope="module")
def room_preview(rt, renderer, scenes):
    cam, linear, noise = _preview(rt, renderer, scenes, "test_room", 160, 160)
    return linear, renderer.guides(cam, 4), noise


@pytest.mark.gpu
@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("source", ["synthetic", "room", "ragged"])
def test_guided_filter_matches_the_numpy_reference(rt, renderer, scenes, room_preview, source, iterations, demodulate):
    if source == "synthetic":
        cases = [_synthetic_guides()]
    elif source == "ragged":                                      # partial tiles; at 8 iterations the taps 128 apart overshoot both sides
        cases = [_synthetic_guides(h, w) for w, h in RAGGED + [(100, 75)]]
    else:
        cases = [room_preview]
    renderer.upload(scenes("cornell_box"))
    modes = [0] if source == "room" else [0, 1]
    for (linear, g, noise), real_mode in [(c, m) for c in cases for m in modes]:
        out, rgb8 = renderer.denoise_guided(linear, g, noise, demodulate=demodulate, real_mode=real_mode, iterations=iterations)
        ref = reference_denoise_guided(linear, g, noise, demodulate=demodulate, **dict(DEFAULTS, iterations=iterations))
        rel = (np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max()
        print(source, iterations, demodulate, real_mode, out.shape, "rel", rel)
        assert rel <= 1e-4, (real_mode, out.shape, rel)
        if real_mode == 1:
            assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
        assert np.array_equal(rgb8, _to_byte(out.astype(np.float32).astype(np.float64)))
        again, again8 = renderer.denoise_guided(linear, g, noise, demodulate=demodulate, real_mode=real_mode, iterations=iterations)
        assert np.array_equal(again, out) and np.array_equal(again8, rgb8)


@pytest.mark.gpu
@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
@pytest.mark.parametrize("opts", RICH_OPTIONS, ids=["it1", "defaults", "it8", "sigmas"])
@pytest.mark.parametrize("source", ["rich", "ragged"])
def test_guided_filter_matches_the_numpy_reference_on_rich_inputs(rt, renderer, scenes, source, opts, demodulate):
    """The same comparison on inputs that show every term of the rule (tests/rule_inputs.py, tests/test_rule_sensitivity.py): a
    second set with its own hit fractions, gradients, normals and seen albedo, albedos below the demodulation floor -- in both
    real modes.  Worst relative error on an MI355X: DESIGN.md, "What the post-processing tests can see"."""
    from tests.rule_inputs import rich_filter_case

    renderer.upload(scenes("cornell_box"))
    sizes = [(64, 48)] if source == "rich" else RAGGED + [(100, 75)]
    full = dict(DEFAULTS, **opts)
    for w, h in sizes:
        linear, g, noise = rich_filter_case(h, w)
        ref = reference_denoise_guided(linear, g, noise, demodulate=demodulate, **full)   # one reference for both modes
        for real_mode in (0, 1):
            out, rgb8 = renderer.denoise_guided(linear, g, noise, demodulate=demodulate, real_mode=real_mode, **opts)
            rel = (np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max()
            print("rich", opts, demodulate, real_mode, out.shape, "rel", rel)
            assert rel <= 1e-4, (real_mode, out.shape, rel)
            if real_mode == 1:
                assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
            assert np.array_equal(rgb8, _to_byte(out.astype(np.float32).astype(np.float64)))
            again, again8 = renderer.denoise_guided(linear, g, noise, demodulate=demodulate, real_mode=real_mode, **opts)
            assert np.array_equal(again, out) and np.array_equal(again8, rgb8)


def _first_materials(renderer, cam, seed, n):
    """Material of the first hit of samples 0 .. n-1 of every pixel (-1 on a miss): [H, W, n]."""
    w, h = cam.image_width, cam.image_height
    ijs = _all_samples(w, h, n)
    rays, _ = renderer.debug_get_ray(cam, seed, ijs)
    rays9 = np.concatenate([rays, np.full((len(ijs), 1), 0.001), np.full((len(ijs), 1), np.inf)], 1)
    ijs64 = ijs.astype(np.int64)
    keys = np.stack([np.full(len(ijs), seed), ijs64[:, 1] * w + ijs64[:, 0], ijs64[:, 2] + 2 ** 31], 1).astype(np.uint32)
    rec, _ = renderer.closest_hit(rays9, keys)
    return np.where(rec[:, 0] != 0, rec[:, 11], -1).astype(np.int64).reshape(h, w, n)


def device_quality(rt, renderer, scenes, name, w, h, seed, follows=(MIRROR,)):
    """MSE ratios against 1024 spp of another seed of a 32-spp session's denoised previews: today's filter, the guided one and
    the demodulating one per follow setting; regions by the first-hit material of all 4 guide samples."""
    scene = scenes(name)
    renderer.upload(scene)
    cam = _camera(rt, scene, name, w, h, 32, 10)
    p = renderer.progressive(cam, seed=seed)
    noisy, _, _ = p.step(32)
    out = {"today": p.denoised(4)[0]}
    for f in follows:
        tag = "" if f == MIRROR else "+glass"
        out["guided" + tag] = p.denoised_guided(4, follow=f)[0]
        out["demodulated" + tag] = p.denoised_guided(4, follow=f, demodulate=True)[0]
    p.close()
    truth, _, _ = renderer.render_host(_camera(rt, scene, name, w, h, 1024, 10), seed=seed + 1000)
    first = _first_materials(renderer, cam, seed, 4)
    mats, _ = _materials(scene)
    if name == "test_room":
        regions = _regions(first, ("mirror", "noise", "checker", "glass"))
    else:
        mirrors = [k for k, m in enumerate(mats) if m.kind == MAT_METAL and m.param == 0]
        regions = {"mirror": np.all(np.isin(first, mirrors), axis=-1)}
    q = _ratios(noisy, truth, out, regions)
    q["share"] = {k: float(m.mean()) for k, m in regions.items()}
    return q


# Bounds = the ratios measured on the device ("Denoiser") + 15 %.
ROOM_BOUNDS = {("guided", "mirror"): 0.4952, ("demodulated", "noise"): 0.0936, ("demodulated", "all"): 0.3369, ("guided", "all"): 0.4839}
BOOK1_BOUNDS = {("guided", "mirror"): 0.6028, ("guided", "all"): 0.5781}


@pytest.mark.gpu
def test_quality_on_the_test_room(rt, renderer, scenes):
    q = device_quality(rt, renderer, scenes, "test_room", 160, 160, 1, follows=(MIRROR, MIRROR | DIELECTRIC))
    print("test room, device:", json.dumps(q))
    assert q["guided"]["mirror"] < q["today"]["mirror"]
    assert q["demodulated"]["noise"] < q["today"]["noise"]
    assert q["demodulated"]["all"] < q["today"]["all"]
    for name in ("noise", "checker", "glass"):
        assert abs(q["guided"][name] - q["today"][name]) <= 0.002, name
    for (key, name), measured in ROOM_BOUNDS.items():
        assert q[key][name] <= 1.15 * measured, (key, name, q[key][name])
    # recorded, not gated: following glass by the render's lottery at 4 guide samples (q["guided+glass"]["glass"])


@pytest.mark.gpu
def test_quality_on_book1_final(rt, renderer, scenes):
    q = device_quality(rt, renderer, scenes, "book1_final", 480, 270, rt.RENDER_SEED)
    print("book1_final, device:", json.dumps(q))
    assert q["share"]["mirror"] > 0.1
    assert q["guided"]["mirror"] < q["today"]["mirror"]
    assert q["guided"]["all"] < q["today"]["all"]
    for (key, name), measured in BOOK1_BOUNDS.items():
        assert q[key][name] <= 1.15 * measured, (key, name, q[key][name])
    # recorded, not gated: demodulation loses on this scene (q["demodulated"]["all"] > q["guided"]["all"])


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_guided_previews_leave_the_session_alone(rt, renderer, scenes, real_mode):
    scene = scenes("test_room")
    renderer.upload(scene)
    cam = room_camera(rt, 64, 48)
    cam.max_depth = 8
    one, one8, _ = renderer.render_host(cam, real_mode=real_mode)
    a, b = renderer.progressive(cam, real_mode=real_mode), renderer.progressive(cam, real_mode=real_mode)
    a_lin, _, a_noise = a.step(16)
    b.step(16)
    option_sets = [dict(follow=MIRROR), dict(follow=MIRROR | DIELECTRIC), dict(follow=MIRROR | DIELECTRIC, max_bounces=1), dict(follow=MIRROR, demodulate=True)]
    results = []
    for o in option_sets + option_sets[::-1]:                      # kept per option set: the way back gives the same bits
        den, den8 = a.denoised_guided(4, **o)
        g = renderer.guides(cam, 4, follow=o["follow"], max_bounces=o.get("max_bounces", 0), real_mode=real_mode)
        want, want8 = renderer.denoise_guided(a_lin, g, a_noise, demodulate=o.get("demodulate", False), real_mode=real_mode)
        assert np.array_equal(den, want) and np.array_equal(den8, want8), o
        results.append(den)
    assert not np.array_equal(results[0], results[1]) and not np.array_equal(results[1], results[2]) and not np.array_equal(results[0], results[3])
    den2, _ = a.denoised_guided(2)
    assert not np.array_equal(den2, results[0])
    assert np.array_equal(a.denoised(4)[0], renderer.denoise(a_lin, renderer.aovs(cam, 4, real_mode=real_mode), a_noise, real_mode=real_mode)[0])
    a.step(16)
    b.step(16)
    a.denoised_guided()
    assert a.save() == b.save() and a.noise() == b.noise()
    fa, fa8, _ = a.step(16)
    fb, _, _ = b.step(16)
    assert a.save() == b.save()
    assert np.array_equal(fa, one) and np.array_equal(fa8, one8) and np.array_equal(fb, one)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_guided_previews_of_adaptive_and_partial_chunk_sessions(rt, renderer, scenes, real_mode):
    from tests.test_adaptive import _adaptive_cases, _median_rel_target, _uniform_metrics

    name, w, h, target, depth, min_samples, step = _adaptive_cases("ragged")[0]
    scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
    renderer.upload(scene)
    cam = scene.camera(w, h, target, depth)
    g = renderer.guides(cam, 4, real_mode=real_mode)
    rel_target = _median_rel_target(_uniform_metrics(renderer, cam, real_mode, step), min_samples, target)
    p = renderer.progressive(cam, real_mode=real_mode, rel_target=rel_target, min_samples=min_samples)
    mixed = 0
    while p.samples_done < target:
        linear, _, noise = p.step(step)
        spp = p.tile_samples()
        if not ((spp < p.samples_done).any() and (spp == p.samples_done).any()):
            continue
        mixed += 1
        before = p.save()
        den, den8 = p.denoised_guided(demodulate=bool(mixed & 1))
        want, want8 = renderer.denoise_guided(linear, g, noise, demodulate=bool(mixed & 1), real_mode=real_mode)
        assert np.array_equal(den, want) and np.array_equal(den8, want8), p.samples_done
        assert p.save() == before
    assert mixed >= 2
    p.close()
    cam = scene.camera(w, h, 36, depth)                           # 36 samples: 4 full chunks and 4 samples
    p = renderer.progressive(cam, real_mode=real_mode)
    for n in (8, 8, 8, 8, 4):
        linear, _, noise = p.step(n)
    assert p.samples_done == 36 and p.noise()["full_chunks"] == 4
    before = p.save()
    den, den8 = p.denoised_guided()
    want, want8 = renderer.denoise_guided(linear, g, noise, real_mode=real_mode)
    assert np.array_equal(den, want) and np.array_equal(den8, want8)
    assert p.save() == before
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_asynchronous_forms_on_a_caller_stream_and_refusals(rt, renderer, scenes, real_mode):
    import torch

    lib = rt.hip_lib()
    scene = scenes("test_room")
    renderer.upload(scene)
    w = h = 56
    cam = room_camera(rt, w, 32)
    dev = torch.device("cuda", renderer.device)
    dt = torch.float64 if real_mode == 0 else torch.float32
    stream = torch.cuda.Stream(device=dev)
    want_g = renderer.guides(cam, 4, follow=MIRROR | DIELECTRIC, max_bounces=3, real_mode=real_mode)
    go, dn = rt.GuideOpts(MIRROR | DIELECTRIC, 3), rt.DenoiseOpts(0, 0, 0, 0, 0, 0)
    ro = rt.RenderOpts(rt.RENDER_SEED, real_mode, 0, 1, 0, 0, stream.cuda_stream)
    d_g = torch.full((h, w, 16), -7.0, dtype=torch.float32, device=dev)
    lin, noise = torch.full((h, w, 3), -3.0, dtype=dt, device=dev), torch.full((h, w), -3.0, dtype=torch.float32, device=dev)
    out, out8 = torch.full((h, w, 3), -3.0, dtype=dt, device=dev), torch.full((h, w, 3), 77, dtype=torch.uint8, device=dev)
    own, own8 = torch.full((h, w, 3), -3.0, dtype=dt, device=dev), torch.full((h, w, 3), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    # refusals first: the sentinels stay
    bare = rt.Renderer(renderer.device)
    assert lib.rtk_render_guides(bare._ctx, C.byref(cam), C.byref(ro), 4, C.byref(go), d_g.data_ptr()) == -5
    bare.close()
    two_ranks = rt.RenderOpts(rt.RENDER_SEED, real_mode, 0, 2, 0, 0, stream.cuda_stream)
    assert lib.rtk_render_guides(renderer._ctx, C.byref(cam), C.byref(two_ranks), 4, C.byref(go), d_g.data_ptr()) == -1
    assert lib.rtk_render_guides(renderer._ctx, C.byref(cam), C.byref(ro), 4, C.byref(rt.GuideOpts(7, 0)), d_g.data_ptr()) == -1
    assert lib.rtk_render_guides(renderer._ctx, C.byref(cam), C.byref(ro), 0, C.byref(go), d_g.data_ptr()) == -1
    args = (renderer._ctx, w, h, real_mode, lin.data_ptr(), d_g.data_ptr(), noise.data_ptr())
    assert lib.rtk_denoise_guided(*args, C.byref(dn), 2, out.data_ptr(), out8.data_ptr(), stream.cuda_stream) == -1
    assert lib.rtk_denoise_guided(*args, C.byref(rt.DenoiseOpts(9, 0, 0, 0, 0, 0)), 0, out.data_ptr(), out8.data_ptr(), stream.cuda_stream) == -1
    assert lib.rtk_denoise_guided(renderer._ctx, w, h, real_mode, lin.data_ptr(), d_g.data_ptr(), None, C.byref(dn), 0, out.data_ptr(), out8.data_ptr(),
                                  stream.cuda_stream) == -1
    p = renderer.progressive(cam, real_mode=real_mode, stream=stream.cuda_stream)
    p.step_device(8, lin.data_ptr(), 0, noise.data_ptr(), 0)      # one chunk: no noise estimate yet
    assert lib.rtk_progressive_denoise_guided(p._h, 4, C.byref(go), C.byref(dn), 0, own.data_ptr(), own8.data_ptr()) == -1
    two = renderer.progressive(cam, real_mode=real_mode, n_ranks=2)
    two.step(16)
    assert lib.rtk_progressive_denoise_guided(two._h, 4, C.byref(go), C.byref(dn), 0, own.data_ptr(), own8.data_ptr()) == -1
    two.close()
    stream.synchronize()
    torch.cuda.synchronize(dev)
    assert bool((d_g == -7.0).all()) and bool((out == -3.0).all()) and bool((out8 == 77).all()) and bool((own == -3.0).all()) and bool((own8 == 77).all())
    # the chain on the stream: a step, the guides, the filter on them, the session's own
    p.step_device(24, lin.data_ptr(), 0, noise.data_ptr(), 0)
    assert lib.rtk_render_guides(renderer._ctx, C.byref(cam), C.byref(ro), 4, C.byref(go), d_g.data_ptr()) == 0
    assert lib.rtk_denoise_guided(*args, C.byref(dn), 1, out.data_ptr(), out8.data_ptr(), stream.cuda_stream) == 0
    assert lib.rtk_progressive_denoise_guided(p._h, 4, C.byref(go), C.byref(dn), 1, own.data_ptr(), own8.data_ptr()) == 0
    stream.synchronize()
    assert np.array_equal(d_g.cpu().numpy(), want_g)
    want, want8 = renderer.denoise_guided(lin.double().cpu().numpy(), want_g, noise.cpu().numpy(), demodulate=True, real_mode=real_mode)
    assert np.array_equal(out.double().cpu().numpy(), want) and np.array_equal(out8.cpu().numpy(), want8)
    assert torch.equal(own, out) and torch.equal(own8, out8)
    blocking, blocking8 = p.denoised_guided(4, follow=MIRROR | DIELECTRIC, max_bounces=3, demodulate=True)
    assert np.array_equal(blocking, want) and np.array_equal(blocking8, want8)
    p.close()


@pytest.mark.gpu
def test_camera_writes_the_guided_images(rt, tmp_path):
    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "guided_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "guided_camera_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])
    name, w, h, spp, depth = "book1_final", 96, 54, 32, 8
    text = subprocess.check_output([exe, str(tmp_path), name, EARTH, str(w), str(h), str(spp), str(depth)], timeout=300).decode()
    assert json.loads(text.strip().splitlines()[-1]) == {"rendered": 3}
    r = rt.Renderer(0)
    scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
    cam = scene.camera(w, h, spp, depth)
    info = r.upload_fast(scene, cam.center)                       # camera::auto_order: the fast order where it is proven exact
    if info["exactness"] != 2:
        r.upload(scene)
    p = r.progressive(cam)
    p.step(spp)
    today8, mirror8, demod8 = p.denoised(4)[1], p.denoised_guided(4)[1], p.denoised_guided(4, demodulate=True)[1]
    p.close()
    r.close()
    assert np.array_equal(_read_png(str(tmp_path / "first.png")), today8)      # denoise_follow left 0: today's image
    assert np.array_equal(_read_png(str(tmp_path / "mirror.png")), mirror8)
    assert np.array_equal(_read_png(str(tmp_path / "demod.png")), demod8)
    assert not np.array_equal(mirror8, today8) and not np.array_equal(demod8, mirror8)
