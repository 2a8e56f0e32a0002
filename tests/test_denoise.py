"""First-hit AOVs and the variance-guided a-trous denoiser (rtk_render_aovs, rtk_denoise, rtk_progressive_denoise).

CPU tests: the entry points are declared and exported; the numpy restatement of the filter below keeps a constant image
constant and gives the weights of a hand-computed 3x3 case.
GPU tests (-m gpu): AOVs equal the composition of the known-answer entry points bit for bit, at ragged sizes at every pixel; the
filter matches the numpy restatement; it lowers the error against a 1024-spp frame; nothing else changes (renders, sessions,
checkpoints); denoised previews of adaptive sessions are the step's own output denoised; one output, aliased outputs, a torch
stream and a reused workspace give the same bits; refusals write nothing; the C++ camera writes the same images."""
import ctypes as C
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests.conftest import EARTH, ROOT
from tests.desc_builder import MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC, MAT_LAMBERTIAN, MAT_METAL, MAT_SPECULAR, SceneDesc

ENTRY_POINTS = ("rtk_render_aovs", "rtk_render_aovs_host", "rtk_denoise", "rtk_denoise_host", "rtk_progressive_denoise",
                "rtk_progressive_denoise_host")
DEFAULTS = {"iterations": 5, "sigma_l": 4.0, "sigma_n": 128.0, "sigma_z": 1.0, "sigma_a": 0.1}
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
BINOMIAL3 = np.array([0.25, 0.5, 0.25])


# ------------------------------------------------------------------------------------------------------ numpy reference --
def _shift(x, oy, ox):
    """x[j + oy, i + ox] at every (j, i), and where that lies inside the image."""
    h, w = x.shape[:2]
    out = np.zeros_like(x)
    valid = np.zeros((h, w), bool)
    ys, ye, xs, xe = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = x[ys + oy:ye + oy, xs + ox:xe + ox]
        valid[ys:ye, xs:xe] = True
    return out, valid


def _clamped(x, oy, ox):
    h, w = x.shape[:2]
    jj = np.clip(np.arange(h) + oy, 0, h - 1)
    ii = np.clip(np.arange(w) + ox, 0, w - 1)
    return x[jj][:, ii]


def reference_denoise(linear, aov, noise, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, sigma_a=0.1, return_weights=False):
    """include/rtk.h "Denoising", in float64: the colour as the filter reads it (rounded to float), var = se^2."""
    c = np.asarray(linear, np.float32).astype(np.float64)
    se = np.asarray(noise, np.float32)
    var = (se * se).astype(np.float64)
    aov = np.asarray(aov, np.float32).astype(np.float64)
    alb, hit, nrm, z = aov[..., 0:3], aov[..., 3], aov[..., 4:7], aov[..., 7]
    grad = np.maximum(np.abs(_clamped(z, 0, 1) - _clamped(z, 0, -1)), np.abs(_clamped(z, 1, 0) - _clamped(z, -1, 0))) / 2
    nzero = np.all(nrm == 0, axis=-1)
    nlen = np.sqrt((nrm * nrm).sum(-1))
    weights = []
    for k in range(iterations):
        step = 2 ** k
        gv = sum(BINOMIAL3[b + 1] * BINOMIAL3[a + 1] * _clamped(var, b, a) for b in (-1, 0, 1) for a in (-1, 0, 1))
        y = (c[..., 0] + c[..., 1] + c[..., 2]) / 3
        lden = sigma_l * np.sqrt(np.maximum(gv, 0)) + 1e-6
        sw = np.zeros(y.shape)
        sc = np.zeros(c.shape)
        sv = np.zeros(y.shape)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = step * dy, step * dx
                cq, valid = _shift(c, oy, ox)
                vq, _ = _shift(var, oy, ox)
                aq, _ = _shift(alb, oy, ox)
                hq, _ = _shift(hit, oy, ox)
                nq, _ = _shift(nrm, oy, ox)
                zq, _ = _shift(z, oy, ox)
                yq = (cq[..., 0] + cq[..., 1] + cq[..., 2]) / 3
                wl = np.exp(-np.abs(y - yq) / lden)
                nqzero = np.all(nq == 0, axis=-1)
                with np.errstate(invalid="ignore", divide="ignore"):
                    cos = (nrm * nq).sum(-1) / (nlen * np.sqrt((nq * nq).sum(-1)))
                    wn = np.where(nzero & nqzero, 1.0, np.where(nzero | nqzero, 0.0, np.maximum(0.0, np.nan_to_num(cos)) ** sigma_n))
                o = step * np.sqrt(dx * dx + dy * dy)
                wz = np.where((hit == 0) | (hq == 0), 1.0, np.exp(-np.abs(z - zq) / (sigma_z * (grad * o + 1e-3 * z) + 1e-6)))
                wa = np.exp(-np.sqrt(((alb - aq) ** 2).sum(-1)) / sigma_a)
                w = np.where(valid, H5[dx + 2] * H5[dy + 2] * wl * wn * wz * wa, 0.0)
                weights.append(w)
                sw += w
                sc += w[..., None] * cq
                sv += w * w * vq
        c = sc / sw[..., None]
        var = sv / (sw * sw)
    return (c, weights) if return_weights else c


def _to_byte(x):
    g = np.sqrt(np.maximum(x, 0.0))
    return (255.999 * np.clip(g, 0.0, 0.999)).astype(np.int64).astype(np.uint8)


def _read_png(path):
    """RGB8 of a PNG written by the camera's encoder (8-bit RGB, filter 0 rows)."""
    data = open(path, "rb").read()
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
            assert body[8:10] == bytes([8, 2]), body
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * 3 + 1)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def _synthetic(h=48, w=64, seed=5):
    """Hard edges in colour, normal, depth and albedo, and noise on the colour."""
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:h, 0:w]
    aov = np.zeros((h, w, 8), np.float32)
    left = ii < w // 2
    aov[..., 0:3] = np.where(left[..., None], [0.8, 0.2, 0.1], [0.1, 0.5, 0.9])
    aov[..., 3] = np.where(jj < 6, 0.0, 1.0)                      # a band of background (no hits)
    aov[..., 4:7] = np.where((jj < h // 2)[..., None], [0.0, 0.0, 1.0], [0.0, 0.7071, 0.7071])
    aov[..., 7] = np.where(ii + jj < 50, 2.0, 5.0) + 0.01 * ii
    aov[jj < 6, 4:8] = 0
    aov[jj < 6, 0:3] = [0.3, 0.4, 0.5]
    clean = aov[..., 0:3].astype(np.float64) * np.where(jj < 24, 0.9, 0.3)[..., None]
    se = (0.05 + 0.1 * rng.random((h, w))).astype(np.float32)
    noisy = clean + rng.normal(0, 1, (h, w, 3)) * se[..., None]
    return noisy, aov, se


# ---------------------------------------------------------------------------------------------------------------- CPU --
def test_header_declares_and_library_exports_the_denoise_api(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, body), name
    assert re.search(r"typedef struct rtk_denoise_opts\b", body)
    assert "#define RTK_ABI_VERSION 2" in body
    lib = C.CDLL(rt.HIP_LIB_PATH)                          # loads without a GPU
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert C.sizeof(rt.DenoiseOpts) == 24


def test_reference_keeps_a_constant_image_constant():
    noisy, aov, se = _synthetic()
    const = np.full(noisy.shape, 0.375)
    for it in (1, 5, 8):
        out = reference_denoise(const, aov, se, iterations=it)
        assert np.abs(out - 0.375).max() < 1e-12


def test_reference_weights_equal_a_hand_computed_3x3_case():
    """One iteration on 3x3 pixels: equal normals, no hits (w_z = 1), equal albedo but for one pixel, var = 1/16 everywhere
    (so sigma_l sqrt(gv) = 1), a centre of luminance 1 among zeros."""
    lin = np.zeros((3, 3, 3))
    lin[1, 1] = 1.0
    aov = np.zeros((3, 3, 8), np.float32)
    aov[..., 0:3] = 0.5
    aov[0, 2, 0:3] = [0.5, 0.5, 0.6]                              # albedo distance 0.1 = sigma_a from the rest
    aov[..., 4:7] = [0.0, 1.0, 0.0]
    se = np.full((3, 3), 0.25, np.float32)
    out, w = reference_denoise(lin, aov, se, iterations=1, return_weights=True)
    e = np.exp(-1.0 / (1.0 + 1e-6))
    # taps of the centre: (dy, dx) in {-1, 0, 1}^2 -> w[(dy + 2) * 5 + dx + 2][1, 1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            want = H5[dx + 2] * H5[dy + 2] * (1.0 if dx == dy == 0 else e) * (np.exp(-1.0) if (dy, dx) == (-1, 1) else 1.0)
            assert abs(w[(dy + 2) * 5 + dx + 2][1, 1] - want) < 1e-6 * want, (dy, dx)  # (0.6f - 0.5f is 0.1 within 3e-7)
    for dy in (-2, 2):
        assert w[(dy + 2) * 5 + 2][1, 1] == 0.0                   # outside the image
    total = sum(H5[dx + 2] * H5[dy + 2] * (1.0 if dx == dy == 0 else e) * (np.exp(-1.0) if (dy, dx) == (-1, 1) else 1.0)
                for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert abs(out[1, 1, 0] - H5[2] ** 2 / total) < 1e-6
    # a corner (row 2, column 2): taps dx, dy in {-2, -1, 0} are inside; the centre is the only lit one and (0, 2) the other albedo
    wc = {(dy, dx): H5[dx + 2] * H5[dy + 2] * (e if (dy, dx) == (-1, -1) else 1.0) * (np.exp(-1.0) if (dy, dx) == (-2, 0) else 1.0)
          for dy in (-2, -1, 0) for dx in (-2, -1, 0)}
    assert abs(out[2, 2, 0] - wc[(-1, -1)] / sum(wc.values())) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- GPU --
AOV_SCENES = [("book1_final", 40, 24, 6), ("cornell_box", 32, 32, 6), ("mesh", 40, 24, 6), ("book2_final", 32, 32, 6), ("material_zoo", 40, 24, 6),
              ("cornell_smoke", 32, 32, 6)]


@pytest.fixture(scope="module")
def scenes(rt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
        return cache[name]
    return get


def _compose(rt, renderer, scene, cam, seed, real_mode, ijs):
    """Per (i, j, s): rtk_debug_get_ray, rtk_debug_closest_hit on [0.001, inf] with keys (seed, pixel, s + 2^31), then
    rtk_debug_texture / the material table -> albedo(3), hit, normal(3), depth as `real` values."""
    real = np.float64 if real_mode == rt.RTK_REAL_F64 else np.float32
    W = cam.image_width
    rays, _ = renderer.debug_get_ray(cam, seed, ijs, real_mode)
    n = len(ijs)
    rays9 = np.concatenate([rays, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], 1)
    ijs64 = ijs.astype(np.int64)
    keys = np.stack([np.full(n, seed), ijs64[:, 1] * W + ijs64[:, 0], ijs64[:, 2] + 2 ** 31], 1).astype(np.uint32)
    rec, _ = renderer.closest_hit(rays9, keys, real_mode)
    desc = C.cast(C.c_void_p(scene.desc_ptr), C.POINTER(SceneDesc)).contents
    mats = [desc.materials[k] for k in range(desc.n_materials)]
    bg = cam.background
    miss = np.array([min(max(real(v), real(0)), real(1)) for v in (bg.x, bg.y, bg.z)], real)
    out = np.zeros((n, 8), real)
    tex_rows, tex_ids, uvp = [], [], []
    for k in range(n):
        if rec[k, 0] == 0:
            out[k, 0:3] = miss
            continue
        m = mats[int(rec[k, 11])]
        out[k, 3] = 1
        if m.kind != MAT_ISOTROPIC:
            out[k, 4:7] = rec[k, 5:8].astype(real)
        d = rays[k, 3:6].astype(real)
        out[k, 7] = real(rec[k, 1]) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if m.kind in (MAT_LAMBERTIAN, MAT_ISOTROPIC, MAT_DIFFUSE_LIGHT) and m.texture >= 0:
            tex_rows.append(k)
            tex_ids.append(m.texture)
            uvp.append([rec[k, 9], rec[k, 10], rec[k, 2], rec[k, 3], rec[k, 4]])
        elif m.kind == MAT_DIELECTRIC:
            out[k, 0:3] = 1
        else:
            assert m.kind in (MAT_METAL, MAT_SPECULAR, MAT_LAMBERTIAN, MAT_DIFFUSE_LIGHT), m.kind
            out[k, 0:3] = np.array([m.albedo.x, m.albedo.y, m.albedo.z]).astype(real)
    if tex_rows:
        col, _ = renderer.debug_texture(np.array(tex_ids), np.array(uvp), real_mode)
        out[tex_rows, 0:3] = col.astype(real)
    light = np.array([rec[k, 0] != 0 and mats[int(rec[k, 11])].kind == MAT_DIFFUSE_LIGHT for k in range(n)])
    out[light, 0:3] = np.minimum(out[light, 0:3], real(1))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("order", ["reference", "fast"])
@pytest.mark.parametrize("case", AOV_SCENES, ids=[c[0] for c in AOV_SCENES])
def test_aovs_equal_the_known_answer_composition(rt, renderer, scenes, case, order, real_mode):
    name, w, h, depth = case
    scene = scenes(name)
    cam = scene.camera(w, h, 8, depth)
    if order == "fast":
        renderer.upload_fast(scene, cam.center)
    else:
        renderer.upload(scene)
    seed = 7
    real = np.float64 if real_mode == 0 else np.float32
    a1 = renderer.aovs(cam, 1, seed=seed, real_mode=real_mode)
    a4 = renderer.aovs(cam, 4, seed=seed, real_mode=real_mode)
    rng = np.random.default_rng(11)
    px = rng.choice(w * h, 75, replace=False)
    ijs = np.array([[p % w, p // w, s] for p in px for s in range(4)], np.int32)
    comp = _compose(rt, renderer, scene, cam, seed, real_mode, ijs).reshape(len(px), 4, 8)
    got1 = a1.reshape(-1, 8)[px]
    assert np.array_equal(got1, comp[:, 0].astype(np.float32)), np.argwhere(got1 != comp[:, 0].astype(np.float32))[:5]
    # four samples: in-order `real` sums, each divided by its count once
    want = _aov_of_samples(comp, real)
    got4 = a4.reshape(-1, 8)[px]
    assert np.array_equal(got4, want), np.argwhere(got4 != want)[:5]
    assert (a4[..., 3] > 0).any()


def _aov_of_samples(comp, real):
    """What rtk_render_aovs writes for per-sample compositions comp [pixels, n, 8]: in-order `real` sums, each divided by its
    count once (depth by the hits), rounded to float."""
    sums = np.zeros((comp.shape[0], 8), real)
    for s in range(comp.shape[1]):
        sums = sums + comp[:, s]
    hits = sums[:, 3]
    want = np.zeros_like(sums)
    want[:, 0:7] = sums[:, 0:7] / real(comp.shape[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        want[:, 7] = np.where(hits > 0, sums[:, 7] / np.where(hits > 0, hits, real(1)), real(0))
    return want.astype(np.float32)


def _check_every_pixel(rt, renderer, scene, cam, n, real_mode, seed=7):
    """rtk_render_aovs of n samples against the composition at every pixel of the image; returns the AOVs."""
    w, h = cam.image_width, cam.image_height
    got = renderer.aovs(cam, n, seed=seed, real_mode=real_mode)
    ijs = np.array([[p % w, p // w, s] for p in range(w * h) for s in range(n)], np.int32)
    comp = _compose(rt, renderer, scene, cam, seed, real_mode, ijs).reshape(w * h, n, 8)
    want = _aov_of_samples(comp, np.float64 if real_mode == 0 else np.float32).reshape(h, w, 8)
    assert np.array_equal(got, want), (w, h, n, np.argwhere(got != want)[:5])
    return got


# (width, height) with partial 8x8 tiles: a single pixel, 1-pixel columns and rows, both edges partial
RAGGED = [(1, 1), (1, 37), (37, 1), (13, 7), (65, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["material_zoo", "cornell_smoke", "book2_final"])
def test_aovs_at_ragged_and_degenerate_sizes(rt, renderer, scenes, name, real_mode):
    """Textures, media and motion blur at image sizes whose last tile row and column are partial, every pixel checked, for one
    sample and for a count that is not a power of two."""
    scene = scenes(name)
    renderer.upload(scene)
    hit = 0
    for w, h in RAGGED:
        for n in (1, 5):
            hit += int((_check_every_pixel(rt, renderer, scene, scene.camera(w, h, 8, 6), n, real_mode)[..., 3] > 0).sum())
    assert hit > 0


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_aov_background_is_clamped_per_channel(rt, renderer, scenes, real_mode):
    """Every library scene's background lies inside [0, 1]; a camera with one component above 1 and one below 0 checks the
    clamp of a miss channel by channel."""
    scene = scenes("book1_final")                                 # the sky fills the top of the frame
    renderer.upload(scene)
    misses = 0
    for w, h in ((65, 9), (13, 7)):
        cam = scene.camera(w, h, 8, 6)
        cam.background = rt.Vec3(1.75, -0.5, 0.25)
        for n in (1, 5):
            a = _check_every_pixel(rt, renderer, scene, cam, n, real_mode)
            sky = a[..., 3] == 0
            assert np.array_equal(a[sky][:, 0:3], np.broadcast_to(np.float32([1.0, 0.0, 0.25]), (int(sky.sum()), 3)))
            misses += int(sky.sum())
    assert misses > 0


def _c3_preview(rt, renderer, scenes, w=200, h=200, spp=32, real_mode=0):
    scene = scenes("cornell_box")
    renderer.upload(scene)
    cam = scene.camera(w, h, spp, 10)
    p = renderer.progressive(cam, real_mode=real_mode)
    linear, _, noise = p.step(spp)
    p.close()
    return linear, renderer.aovs(cam, 4, real_mode=real_mode), noise


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [{"iterations": 1}, {}, {"iterations": 8}, {"iterations": 3, "sigma_l": 2.0, "sigma_n": 32.0, "sigma_z": 0.5, "sigma_a": 0.3}],
                         ids=["it1", "defaults", "it8", "sigmas"])
@pytest.mark.parametrize("source", ["synthetic", "c3", "ragged"])
def test_filter_matches_the_numpy_reference(rt, renderer, scenes, source, opts):
    if source == "synthetic":
        renderer.upload(scenes("cornell_box"))
        cases = [_synthetic()]
    elif source == "ragged":                                      # partial tiles; at 8 iterations the taps 128 apart overshoot both sides
        cases = [_synthetic(h, w) for w, h in RAGGED + [(100, 75)]]
    else:
        cases = [_c3_preview(rt, renderer, scenes)]
    modes = [0] if source == "c3" else [0, 1]
    for (linear, aov, noise), real_mode in [(c, m) for c in cases for m in modes]:
        out, rgb8 = renderer.denoise(linear, aov, noise, real_mode=real_mode, **opts)
        full = dict(DEFAULTS, **opts)
        ref = reference_denoise(linear, aov, noise, **full)
        rel = (np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max()
        assert rel <= 1e-4, (real_mode, out.shape, rel)
        if real_mode == 1:
            assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
        # bytes: the resolve's conversion of the float colour
        assert np.array_equal(rgb8, _to_byte(out.astype(np.float32).astype(np.float64)))
        again, again8 = renderer.denoise(linear, aov, noise, real_mode=real_mode, **opts)
        assert np.array_equal(again, out) and np.array_equal(again8, rgb8)


RICH_OPTIONS = [{"iterations": 1}, {}, {"iterations": 8}, {"iterations": 3, "sigma_l": 2.0, "sigma_n": 32.0, "sigma_z": 0.5, "sigma_a": 0.3}]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", RICH_OPTIONS, ids=["it1", "defaults", "it8", "sigmas"])
@pytest.mark.parametrize("source", ["rich", "ragged"])
def test_filter_matches_the_numpy_reference_on_rich_inputs(rt, renderer, scenes, source, opts):
    """The same comparison on inputs that show every term of the rule (tests/rule_inputs.py, tests/test_rule_sensitivity.py):
    neighbours' cosines where cos^sigma_n is neither 0 nor 1, normals of length 0.3 .. 1, fractional hit fractions, albedo
    distances around sigma_a -- in both real modes.  Worst relative error on an MI355X: DESIGN.md, "What the post-processing
    tests can see"."""
    from tests.rule_inputs import rich_filter_case

    renderer.upload(scenes("cornell_box"))
    sizes = [(64, 48)] if source == "rich" else RAGGED + [(100, 75)]
    full = dict(DEFAULTS, **opts)
    for w, h in sizes:
        linear, g, noise = rich_filter_case(h, w)
        aov = np.ascontiguousarray(g[..., 0:8])
        ref = reference_denoise(linear, aov, noise, **full)      # one reference for both modes: the filter rounds its input to float
        for real_mode in (0, 1):
            out, rgb8 = renderer.denoise(linear, aov, noise, real_mode=real_mode, **opts)
            rel = (np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max()
            print("rich", opts, real_mode, out.shape, "rel", rel)
            assert rel <= 1e-4, (real_mode, out.shape, rel)
            if real_mode == 1:
                assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
            assert np.array_equal(rgb8, _to_byte(out.astype(np.float32).astype(np.float64)))
            again, again8 = renderer.denoise(linear, aov, noise, real_mode=real_mode, **opts)
            assert np.array_equal(again, out) and np.array_equal(again8, rgb8)


# (width, height, bound on the MSE ratio denoised / noisy over the image, the same over edge pixels).  The bounds are the
# measured ratios + 15 % ("Denoiser"): book1_final 0.603 / 1.291 -- at 480x270 its small spheres make a third of the
# pixels edges, where the filter is WORSE than the noisy preview -- and cornell_box 0.114 / 0.142.
QUALITY = {"book1_final": (480, 270, 0.69, 1.48), "cornell_box": (400, 400, 0.13, 0.16)}


def quality(rt, renderer, scenes, name):
    w, h = QUALITY[name][:2]
    scene = scenes(name)
    renderer.upload(scene)
    cam = scene.camera(w, h, 32, 10)
    p = renderer.progressive(cam)
    noisy, _, _ = p.step(32)
    den, _ = p.denoised(4)
    p.close()
    truth, _, _ = renderer.render_host(scene.camera(w, h, 1024, 10), seed=rt.RENDER_SEED + 1000)
    aov = renderer.aovs(cam, 4)
    z, n = aov[..., 7].astype(np.float64), aov[..., 4:7].astype(np.float64)
    zmax = np.max([_clamped(z, b, a) for b in (-1, 0, 1) for a in (-1, 0, 1)], 0)
    zmin = np.min([_clamped(z, b, a) for b in (-1, 0, 1) for a in (-1, 0, 1)], 0)
    nn = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-12)
    cmin = np.min([(nn * _clamped(nn, b, a)).sum(-1) for b in (-1, 0, 1) for a in (-1, 0, 1)], 0)
    edge = (zmax - zmin > 0.05 * z) | (cmin < 0.9)
    err_noisy = ((noisy - truth) ** 2).sum(-1)
    err_den = ((den - truth) ** 2).sum(-1)
    return {"mse_noisy": float(err_noisy.mean()), "mse_denoised": float(err_den.mean()), "ratio": float(err_den.mean() / err_noisy.mean()),
            "edge_fraction": float(edge.mean()), "edge_ratio": float(err_den[edge].mean() / err_noisy[edge].mean())}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(QUALITY))
def test_denoising_lowers_the_error_against_a_1024_spp_frame(rt, renderer, scenes, name):
    q = quality(rt, renderer, scenes, name)
    print(name, json.dumps(q))
    assert q["ratio"] <= QUALITY[name][2], q
    assert q["edge_ratio"] <= QUALITY[name][3], q


@pytest.mark.gpu
def test_aovs_and_denoise_change_no_render(rt, renderer, scenes):
    scene = scenes("book1_final")
    renderer.upload(scene)
    cam = scene.camera(240, 135, 32, 10)
    before_lin, before8, _ = renderer.render_host(cam)
    aov = renderer.aovs(cam, 4)
    p = renderer.progressive(cam)
    lin, _, noise = p.step(16)
    renderer.denoise(lin, aov, noise)
    p.denoised(2)
    p.close()
    after_lin, after8, _ = renderer.render_host(cam)
    assert np.array_equal(before8, after8) and np.array_equal(before_lin, after_lin)


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_denoised_previews_leave_the_session_alone(rt, renderer, scenes, real_mode):
    scene = scenes("cornell_box")
    renderer.upload(scene)
    cam = scene.camera(64, 48, 48, 8)
    one, one8, _ = renderer.render_host(cam, real_mode=real_mode)
    a, b = renderer.progressive(cam, real_mode=real_mode), renderer.progressive(cam, real_mode=real_mode)
    a_lin, _, a_noise = a.step(16)
    b.step(16)
    den1, den1_8 = a.denoised()
    # the preview it denoised is the step's own output, with the step's own se
    want, want8 = renderer.denoise(a_lin, renderer.aovs(cam, 4, real_mode=real_mode), a_noise, real_mode=real_mode)
    assert np.array_equal(den1, want) and np.array_equal(den1_8, want8)
    a.step(16)
    b.step(16)
    a.denoised()
    a.denoised(2)
    assert a.save() == b.save() and a.noise() == b.noise()
    fa, fa8, _ = a.step(16)
    fb, _, _ = b.step(16)
    assert a.save() == b.save()
    assert np.array_equal(fa, one) and np.array_equal(fa8, one8) and np.array_equal(fb, one)
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_denoised_previews_of_adaptive_and_partial_chunk_sessions(rt, renderer, scenes, real_mode):
    """rtk_preview_kernel rebuilds the step's preview from the sums: each tile scaled by its own count and se over its own K in an
    adaptive session (1 419 tiles, retired and active ones side by side), and a last step that ends inside a chunk."""
    from tests.test_adaptive import _adaptive_cases, _median_rel_target, _uniform_metrics

    name, w, h, target, depth, min_samples, step = _adaptive_cases("ragged")[0]
    scene = scenes(name)
    renderer.upload(scene)
    cam = scene.camera(w, h, target, depth)
    aov = renderer.aovs(cam, 4, real_mode=real_mode)
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
        den, den8 = p.denoised()
        want, want8 = renderer.denoise(linear, aov, noise, real_mode=real_mode)
        assert np.array_equal(den, want) and np.array_equal(den8, want8), p.samples_done
        assert p.save() == before
    assert mixed >= 2
    p.close()
    # a plain session whose last step ends at the target with a partial chunk: 36 samples are 4 full chunks and 4 samples
    cam = scene.camera(w, h, 36, depth)
    p = renderer.progressive(cam, real_mode=real_mode)
    for n in (8, 8, 8, 8, 4):
        linear, _, noise = p.step(n)
    assert p.samples_done == 36 and p.chunk_size == 8 and p.noise()["full_chunks"] == 4
    before = p.save()
    den, den8 = p.denoised()
    want, want8 = renderer.denoise(linear, aov, noise, real_mode=real_mode)
    assert np.array_equal(den, want) and np.array_equal(den8, want8)
    assert p.save() == before
    p.close()


@pytest.mark.gpu
def test_filter_matches_the_numpy_reference_on_a_c2_preview(rt, renderer):
    """C2's scene and camera (fast order) at 960x540 -- the float64 numpy reference takes about 20 s there, four times that at
    1920x1080: a 32-spp preview, 4-sample AOVs, the default options."""
    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    cam = scene.camera(960, 540, 100, 0)
    assert renderer.upload_fast(scene, cam.center)["exact"]
    p = renderer.progressive(cam)
    linear, _, noise = p.step(32)
    p.close()
    aov = renderer.aovs(cam, 4)
    out, rgb8 = renderer.denoise(linear, aov, noise)
    ref = reference_denoise(linear, aov, noise)
    rel = (np.abs(out - ref) / np.maximum(1.0, np.abs(ref))).max()
    assert rel <= 1e-4, rel
    assert np.array_equal(rgb8, _to_byte(out.astype(np.float32).astype(np.float64)))


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_denoise_entry_point_paths(rt, renderer, real_mode):
    """One output at a time; the device entry point on a torch stream with the colour written over d_linear and the bytes over
    d_noise (include/rtk.h: the outputs may alias d_linear or d_noise); the context's workspace grown and then reused."""
    import torch

    lib = rt.hip_lib()
    h, w = 75, 100
    linear, aov, noise = _synthetic(h, w)
    lin = np.ascontiguousarray(linear)
    both, both8 = renderer.denoise(linear, aov, noise, real_mode=real_mode)
    opts = rt.DenoiseOpts(0, 0, 0, 0, 0, 0)
    args = (renderer._ctx, w, h, real_mode, lin.ctypes.data, aov.ctypes.data, noise.ctypes.data, C.byref(opts))
    only = np.full((h, w, 3), -3.0)
    assert lib.rtk_denoise_host(*args, only.ctypes.data, None) == 0
    only8 = np.full((h, w, 3), 77, np.uint8)
    assert lib.rtk_denoise_host(*args, None, only8.ctypes.data) == 0
    assert np.array_equal(only, both) and np.array_equal(only8, both8)

    dev = torch.device("cuda", renderer.device)
    d_lin = torch.from_numpy(lin).to(dev, torch.float64 if real_mode == 0 else torch.float32)
    d_aov, d_noise = torch.from_numpy(aov).to(dev), torch.from_numpy(noise).to(dev)
    sep_lin, sep8 = torch.full_like(d_lin, -3.0), torch.full((h, w, 3), 77, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    ptrs = (d_lin.data_ptr(), d_aov.data_ptr(), d_noise.data_ptr())
    assert lib.rtk_denoise(renderer._ctx, w, h, real_mode, *ptrs, C.byref(opts), sep_lin.data_ptr(), sep8.data_ptr(), stream.cuda_stream) == 0
    assert lib.rtk_denoise(renderer._ctx, w, h, real_mode, *ptrs, C.byref(opts), d_lin.data_ptr(), d_noise.data_ptr(), stream.cuda_stream) == 0
    stream.synchronize()
    assert np.array_equal(sep_lin.double().cpu().numpy(), both) and np.array_equal(sep8.cpu().numpy(), both8)
    assert torch.equal(d_lin, sep_lin)
    assert torch.equal(d_noise.view(torch.uint8).flatten()[: h * w * 3].view(h, w, 3), sep8)

    one = rt.Renderer(renderer.device)                             # a context of its own: its workspace starts empty
    for w, h in ((13, 7), (340, 260), (13, 7)):
        inputs = _synthetic(h, w)
        got, got8 = one.denoise(*inputs, real_mode=real_mode)
        fresh = rt.Renderer(renderer.device)
        want, want8 = fresh.denoise(*inputs, real_mode=real_mode)
        fresh.close()
        assert np.array_equal(got, want) and np.array_equal(got8, want8), (w, h)
    one.close()


@pytest.mark.gpu
def test_refusals_write_nothing(rt, renderer, scenes):
    lib = rt.hip_lib()
    bare = rt.Renderer(0)                                         # no scene
    scene = scenes("cornell_box")
    renderer.upload(scene)
    cam = scene.camera(32, 24, 32, 6)
    h, w = 24, 32
    sentinel = np.full((h, w, 8), -7.0, np.float32)
    out = sentinel.copy()
    assert lib.rtk_render_aovs_host(bare._ctx, C.byref(cam), C.byref(rt.RenderOpts(1, 0, 0, 1, 0, 0, None)), 4, out.ctypes.data) == -5
    assert lib.rtk_render_aovs_host(renderer._ctx, C.byref(cam), C.byref(rt.RenderOpts(1, 0, 0, 2, 0, 0, None)), 4, out.ctypes.data) == -1
    assert lib.rtk_render_aovs_host(renderer._ctx, C.byref(cam), C.byref(rt.RenderOpts(1, 0, 0, 1, 0, 0, None)), 0, out.ctypes.data) == -1
    assert np.array_equal(out, sentinel)
    bare.close()

    linear, aov, noise = _synthetic(h, w)
    lin = np.ascontiguousarray(linear)
    o_lin, o8 = np.full((h, w, 3), -3.0), np.full((h, w, 3), 77, np.uint8)
    args = lambda noise_ptr, opts: (renderer._ctx, w, h, 0, lin.ctypes.data, aov.ctypes.data, noise_ptr, C.byref(opts), o_lin.ctypes.data, o8.ctypes.data)
    assert lib.rtk_denoise_host(*args(None, rt.DenoiseOpts(0, 0, 0, 0, 0, 0))) == -1             # d_noise required
    assert lib.rtk_denoise_host(*args(noise.ctypes.data, rt.DenoiseOpts(9, 0, 0, 0, 0, 0))) == -1  # iterations 1..8
    assert lib.rtk_denoise_host(*args(noise.ctypes.data, rt.DenoiseOpts(-1, 0, 0, 0, 0, 0))) == -1
    assert lib.rtk_denoise_host(*args(noise.ctypes.data, rt.DenoiseOpts(0, -1, 0, 0, 0, 0))) == -1
    assert np.array_equal(o_lin, np.full((h, w, 3), -3.0)) and np.array_equal(o8, np.full((h, w, 3), 77, np.uint8))

    p = renderer.progressive(cam)
    p.step(8)                                                     # one chunk: no noise estimate yet
    with pytest.raises(rt.RtkError) as e:
        p.denoised()
    assert e.value.code == -1
    p.step(8)
    p.denoised()                                                  # two chunks
    p.close()
    two = renderer.progressive(cam, n_ranks=2)
    two.step(16)
    d_lin = np.full((h, w, 3), -3.0)
    assert lib.rtk_progressive_denoise_host(two._h, 4, None, d_lin.ctypes.data, None) == -1
    assert np.array_equal(d_lin, np.full((h, w, 3), -3.0))
    two.close()


@pytest.mark.gpu
def test_camera_writes_the_one_shot_image_and_the_denoised_one(rt, tmp_path):
    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "denoise_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "denoise_camera_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])
    name, w, h, spp, depth = "cornell_box", 64, 64, 32, 8
    text = subprocess.check_output([exe, str(tmp_path), name, EARTH, str(w), str(h), str(spp), str(depth)], timeout=300).decode()
    v = json.loads(text.strip().splitlines()[-1])
    assert v == {"low_spp_failed": 1}, v
    assert (tmp_path / "two.png").read_bytes() == (tmp_path / "one.png").read_bytes()
    den = _read_png(str(tmp_path / "den.png"))

    r = rt.Renderer(0)
    scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
    cam = scene.camera(w, h, spp, depth)
    info = r.upload_fast(scene, cam.center)                       # camera::auto_order: the fast order where it is proven exact
    if info["exactness"] != 2:
        r.upload(scene)
    one_lin, one8, _ = r.render_host(cam)
    assert np.array_equal(_read_png(str(tmp_path / "one.png")), one8)
    p = r.progressive(cam)
    lin, _, noise = p.step(spp)
    p.close()
    _, want8 = r.denoise(lin, r.aovs(cam, 4), noise)
    assert np.array_equal(den, want8)
    r.close()
