"""Guided upsampling (rtk_upsample*): a frame rendered at 1/f of the width and height rebuilt at full size, steered by the guides
of both resolutions.

CPU tests: the entry points are declared and exported; rtk_upsample_camera puts every low pixel on the mean of its f x f full
pixels; the numpy restatement of the header's rule below keeps constants, gives the edge-renormalised bilinear interpolation
under uniform guides, brings a texture back at full resolution when demodulating, falls back to the bilinear value where the
guides reject every tap, and never raises the noise; option refusals need no device.
GPU tests (-m gpu): the device equals the restatement on every pixel; the entry-point forms, a caller stream, NULL outputs and
refusals; nothing else on the context moves; the low camera covers the full camera's pixels; the C++ camera; real frames."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import EARTH, ROOT
from tests.rule_inputs import rich_guides, shade, view_of
from tests.test_denoise import _read_png, _to_byte
from tests.test_temporal import _v, synthetic_camera, synthetic_guides

ENTRY_POINTS = ("rtk_upsample_camera", "rtk_upsample", "rtk_upsample_host")
DEFAULTS = {"sigma_n": 128.0, "sigma_z": 1.0, "sigma_a": 0.1}
OTHER = {"sigma_n": 32.0, "sigma_z": 2.5, "sigma_a": 0.3}
FACTORS = (2, 3, 4)
CPU_SIZES = [(64, 48), (37, 23), (8, 8), (1, 1), (2, 3), (5, 1)]
GPU_SIZES = [(64, 48), (37, 23), (8, 8), (1, 1)]


def low_size(w, h, f):
    return -(-w // f), -(-h // f)


# ------------------------------------------------------------------------------------------------------ numpy reference --
def _positions(n_full, f):
    """Step 1 of the rule along one axis: (x0 int64 [n], fx float32 [n])."""
    n = 2 * np.arange(n_full, dtype=np.int64) - (f - 1)
    x0 = n // (2 * f)                                             # floor, also below zero
    return x0, (n - 2 * f * x0).astype(np.float32) / np.float32(2 * f)


# Deliberate one-term deviations from the rule: what a subtly wrong kernel would compute.  tests/test_rule_sensitivity.py shows
# that the device comparison's inputs tell each of them from the rule; none is ever run against the device.
VARIANTS = ("cos_without_lengths", "no_z_term", "gradient_min", "hit_below_1", "wn_set1_only", "wz_set1_only", "wz2_with_hit1", "wz2_with_grad1",
            "wa_first_albedo", "o_is_1", "floor_0", "albedo_swapped", "support_omega")


def _depth_gradient(z, variant=None):
    """Half the larger central difference, edges clamped."""
    h, w = z.shape
    ii, jj = np.arange(w), np.arange(h)
    zx = np.abs(z[:, np.clip(ii + 1, 0, w - 1)] - z[:, np.clip(ii - 1, 0, w - 1)])
    zy = np.abs(z[np.clip(jj + 1, 0, h - 1), :] - z[np.clip(jj - 1, 0, h - 1), :])
    return (np.minimum(zx, zy) if variant == "gradient_min" else np.maximum(zx, zy)) / 2.0


def _normal_weight(n_p, n_q, sigma_n, variant=None):
    pz, qz = np.all(n_p == 0, -1), np.all(n_q == 0, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.nan_to_num((n_p * n_q).sum(-1) / (np.sqrt((n_p * n_p).sum(-1)) * np.sqrt((n_q * n_q).sum(-1))))
        if variant == "cos_without_lengths":
            cos = (n_p * n_q).sum(-1)
        w = np.where(cos > 0, np.power(np.maximum(cos, 0.0), sigma_n), 0.0)
    return np.where(pz | qz, (pz & qz).astype(np.float64), w)


def _depth_weight(hit_p, hit_q, z_p, z_q, grad, o, sigma_z, variant=None):
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        w = np.exp(-np.abs(z_p - z_q) / (sigma_z * (grad * o + (0.0 if variant == "no_z_term" else 1e-3) * z_p) + 1e-6))
    if variant == "hit_below_1":
        return np.where((hit_p < 1) | (hit_q < 1), 1.0, w)
    return np.where((hit_p == 0) | (hit_q == 0), 1.0, w)


def reference_upsample(w, h, f, low_linear, low_noise, low_guides, guides, demodulate=False, sigma_n=128.0, sigma_z=1.0, sigma_a=0.1, variant=None):
    """include/rtk.h, "Guided upsampling", in float64 (positions and bilinear weights in float32, as the rule says).
    Returns (out (H, W, 3), var_out (H, W), support (H, W), sum_beta (H, W)).  variant: one of VARIANTS, a deliberately wrong rule."""
    assert variant is None or variant in VARIANTS, variant
    f32 = lambda x: float(np.float32(x))  # noqa: E731  (the options are floats on the device)
    sigma_n, sigma_z, sigma_a = f32(sigma_n), f32(sigma_z), f32(sigma_a)
    lw, lh = low_size(w, h, f)
    c = np.asarray(low_linear, np.float32).astype(np.float64).reshape(lh, lw, 3)
    var = np.asarray(low_noise, np.float32).astype(np.float64).reshape(lh, lw) ** 2
    G = np.asarray(low_guides, np.float32).astype(np.float64).reshape(lh, lw, 16)
    g = np.asarray(guides, np.float32).astype(np.float64).reshape(h, w, 16)
    swapped = demodulate and variant == "albedo_swapped"
    if demodulate:
        A_q = np.maximum(G[..., 8:11], 0.02)
        if not swapped:
            c, var = c / A_q, var / A_q.mean(-1) ** 2
    x0, fx = _positions(w, f)
    y0, fy = _positions(h, f)
    grad1, grad2 = _depth_gradient(g[..., 7], variant), _depth_gradient(g[..., 15], variant)
    if variant == "wz2_with_grad1":
        grad2 = grad1
    hit2 = g[..., 3] if variant == "wz2_with_hit1" else g[..., 11]
    alb = slice(0, 3) if variant == "wa_first_albedo" else slice(8, 11)
    floor = 0.0 if variant == "floor_0" else 1e-3
    s_om, s_c, s_v, s_beta, s_acc = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    for b in (0, 1):
        for a in (0, 1):
            ti, tj = x0 + a, y0 + b
            inside = ((tj >= 0) & (tj < lh))[:, None] & ((ti >= 0) & (ti < lw))[None, :]
            ti, tj = np.clip(ti, 0, lw - 1), np.clip(tj, 0, lh - 1)
            bx, by = (fx if a else np.float32(1) - fx), (fy if b else np.float32(1) - fy)
            beta = (by[:, None] * bx[None, :]).astype(np.float64)                        # a float32 product
            q = G[tj[:, None], ti[None, :]]
            ox, oy = fx.astype(np.float64) - a, fy.astype(np.float64) - b
            o = f * np.sqrt(ox[None, :] ** 2 + oy[:, None] ** 2)
            if variant == "o_is_1":
                o = 1.0
            w_n = _normal_weight(g[..., 4:7], q[..., 4:7], sigma_n, variant)
            w_z = _depth_weight(g[..., 3], q[..., 3], g[..., 7], q[..., 7], grad1, o, sigma_z, variant)
            if variant != "wn_set1_only":
                w_n = np.minimum(w_n, _normal_weight(g[..., 12:15], q[..., 12:15], sigma_n, variant))
            if variant != "wz_set1_only":
                w_z = np.minimum(w_z, _depth_weight(hit2, q[..., 3] if variant == "wz2_with_hit1" else q[..., 11], g[..., 15], q[..., 15], grad2, o, sigma_z, variant))
            w_a = 1.0 if demodulate else np.exp(-np.sqrt(((g[..., alb] - q[..., alb]) ** 2).sum(-1)) / sigma_a)
            wt = w_n * w_z * w_a
            beta = np.where(inside, beta, 0.0)
            om = beta * (wt + floor)
            s_om += om
            cq, vq = c[tj[:, None], ti[None, :]], var[tj[:, None], ti[None, :]]
            if swapped:                                           # the tap divided by the full pixel's albedo, the blend multiplied by the tap's
                A_p = np.maximum(g[..., 8:11], 0.02)
                A_t = A_q[tj[:, None], ti[None, :]]
                cq, vq = cq / A_p * A_t, vq / A_p.mean(-1) ** 2 * A_t.mean(-1) ** 2
            s_c += om[..., None] * cq
            s_v += om * om * vq
            s_beta += beta
            s_acc += (om if variant == "support_omega" else beta * wt)
    with np.errstate(invalid="ignore", divide="ignore"):
        out, var_out = s_c / s_om[..., None], s_v / (s_om * s_om)
    if demodulate and not swapped:
        A_p = np.maximum(g[..., 8:11], 0.02)
        out, var_out = out * A_p, var_out * A_p.mean(-1) ** 2
    return out, var_out, s_acc / s_beta, s_beta


def bilinear(w, h, f, low):
    """The edge-renormalised bilinear interpolation of `low` (LH, LW[, 3]) at the rule's positions, written separably: a
    (W, LW) and an (H, LH) matrix of the one-dimensional weights, rows normalised."""
    lw, lh = low_size(w, h, f)

    def matrix(n_full, n_low):
        x0, fx = _positions(n_full, f)
        m = np.zeros((n_full, n_low))
        for a in (0, 1):
            t = x0 + a
            ok = (t >= 0) & (t < n_low)
            m[np.arange(n_full)[ok], t[ok]] += np.where(a, fx, np.float32(1) - fx).astype(np.float64)[ok]
        return m / m.sum(1, keepdims=True)

    low = np.asarray(low, np.float64).reshape(lh, lw, -1)
    return np.einsum("jJ,JIc,iI->jic", matrix(h, lh), low, matrix(w, lw))


def random_case(w, h, f, seed):
    """Random guides of both resolutions (surfaces and background, two distinct guide sets), colour and se of the low image."""
    rng = np.random.default_rng(seed)
    lw, lh = low_size(w, h, f)

    def guides(hh, ww):
        g = np.zeros((hh, ww, 16))
        for s in (0, 8):
            hit = rng.random((hh, ww)) < 0.8
            n = rng.normal(size=(hh, ww, 3))
            n /= np.sqrt((n * n).sum(-1, keepdims=True))
            g[..., s:s + 3] = rng.random((hh, ww, 3))
            g[..., s + 3] = np.where(hit, rng.choice([0.25, 0.5, 1.0], (hh, ww)), 0.0)
            g[..., s + 4:s + 7] = np.where(hit[..., None], n * rng.choice([0.5, 1.0], (hh, ww, 1)), 0.0)
            g[..., s + 7] = np.where(hit, rng.uniform(1.0, 20.0, (hh, ww)), 0.0)
        return g.astype(np.float32)

    return rng.uniform(0.0, 2.0, (lh, lw, 3)), rng.uniform(0.01, 0.3, (lh, lw)).astype(np.float32), guides(lh, lw), guides(h, w)


def uniform_guides(h, w):
    g = np.zeros((h, w, 16), np.float32)
    g[...] = np.array([0.5, 0.6, 0.7, 1.0, 0.0, 0.6, 0.8, 5.0] * 2, np.float32)
    return g


CPU_CASES = [(w, h, f) for (w, h) in CPU_SIZES for f in FACTORS]


# ---------------------------------------------------------------------------------------------------------------- CPU --
def test_header_declares_and_library_exports_the_upsample_api(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, body), name
    assert re.search(r"typedef struct rtk_upsample_opts\b", body) and re.search(r"#define RTK_UPSAMPLE_DEMODULATE 1\b", body)
    assert "#define RTK_ABI_VERSION 2" in body                    # new entry points only
    assert header.index("Temporal accumulation ---") < header.index("Guided upsampling ---")
    lib = C.CDLL(rt.HIP_LIB_PATH)                                 # loads without a GPU
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert C.sizeof(rt.UpsampleOpts) == 24 and rt.UPSAMPLE_DEMODULATE == 1
    assert callable(rt.upsample_camera) and hasattr(rt.Renderer, "upsample") and hasattr(rt.Renderer, "upsample_device")


@pytest.mark.parametrize("f", FACTORS)
def test_low_camera_pixels_are_the_means_of_their_full_pixels(rt, f):
    for w, h in ((37, 23), (201, 113), (64, 48), (1, 1), (5, 1)):
        full = rt.derive_camera(w, w / (h + 0.25), spp=24, max_depth=7, vfov=35.0, lookfrom=(3.0, 2.5, -7.0), lookat=(0.5, 1.0, 0.25), vup=(0.1, 1.0, 0.0),
                                focus_dist=4.0, defocus_angle=0.6)
        assert (full.image_width, full.image_height) == (w, h)
        low = rt.upsample_camera(full, f)
        lw, lh = low_size(w, h, f)
        assert (low.image_width, low.image_height) == (lw, lh)
        du, dv, p00 = _v(full.pixel_delta_u), _v(full.pixel_delta_v), _v(full.pixel00_loc)
        assert np.array_equal(_v(low.pixel_delta_u), f * du) and np.array_equal(_v(low.pixel_delta_v), f * dv)
        scale = np.abs(p00).max() + (w + f) * np.abs(du).max() + (h + f) * np.abs(dv).max()
        k = np.arange(f)
        for I, J in ((0, 0), (lw - 1, lh - 1), (lw // 2, lh // 3)):
            centre = _v(low.pixel00_loc) + I * _v(low.pixel_delta_u) + J * _v(low.pixel_delta_v)
            mean = (p00 + (f * I + k)[:, None, None] * du + (f * J + k)[None, :, None] * dv).reshape(-1, 3).mean(0)
            assert np.abs(centre - mean).max() <= 1e-12 * scale, (w, h, I, J)
        # every other field is copied
        same = rt.Camera.from_buffer_copy(bytes(low))
        same.image_width, same.image_height, same.pixel00_loc, same.pixel_delta_u, same.pixel_delta_v = w, h, full.pixel00_loc, full.pixel_delta_u, full.pixel_delta_v
        assert bytes(same) == bytes(full)
    assert rt.upsample_camera(full).image_width == low_size(5, 1, 2)[0]                  # factor defaults to 2


def test_low_camera_refusals_leave_the_output_untouched(rt):
    lib = rt.hip_lib()
    full = rt.derive_camera(40, 40 / 30.0)
    mark = rt.derive_camera(7, 1.0, spp=3)
    out = rt.Camera.from_buffer_copy(bytes(mark))
    empty = rt.Camera.from_buffer_copy(bytes(full))
    empty.image_height = 0
    for cam, f in ((full, 1), (full, 5), (full, 0), (full, -2), (empty, 2)):
        assert lib.rtk_upsample_camera(C.byref(cam), f, C.byref(out)) == -1 and bytes(out) == bytes(mark), f
        assert "rtk_upsample_camera" in lib.rtk_last_error().decode()
    assert lib.rtk_upsample_camera(None, 2, C.byref(out)) == -1 and bytes(out) == bytes(mark)
    assert lib.rtk_upsample_camera(C.byref(full), 2, None) == -1
    with pytest.raises(rt.RtkError):
        rt.upsample_camera(full, 5)


def test_option_refusals_need_no_device(rt):
    """Options are checked before anything else: with no context at all, a bad option is what the error names."""
    lib = rt.hip_lib()
    err = lambda: lib.rtk_last_error().decode()  # noqa: E731
    cam = rt.derive_camera(16, 1.0)
    low, low_se, low_g, g = np.zeros((8, 8, 3)), np.zeros((8, 8), np.float32), np.zeros((8, 8, 16), np.float32), np.zeros((16, 16, 16), np.float32)
    o_lin, o_se = np.full((16, 16, 3), -3.0), np.full((16, 16), -3.0, np.float32)
    U = rt.UpsampleOpts
    cases = ((U(0, 0, 0, 0, 2, 0), "flags"), (U(0, 0, 0, 0, -1, 0), "flags"), (U(0, 0, 0, 0, 0, 1), "reserved"), (U(1, 0, 0, 0, 0, 0), "factor"),
             (U(5, 0, 0, 0, 0, 0), "factor"), (U(-2, 0, 0, 0, 0, 0), "factor"), (U(0, -0.1, 0, 0, 0, 0), "sigmas"), (U(0, 0, float("nan"), 0, 0, 0), "sigmas"),
             (U(0, 0, 0, float("inf"), 0, 0), "sigmas"), (U(0, 0, 0, -1.0, 1, 0), "sigmas"), (U(4, 1.0, 1.0, 1.0, 1, 0), "null context"))
    for opts, word in cases:
        for fn, extra in ((lib.rtk_upsample, (None,)), (lib.rtk_upsample_host, ())):
            assert fn(None, C.byref(cam), 0, low.ctypes.data, low_se.ctypes.data, low_g.ctypes.data, g.ctypes.data, C.byref(opts), o_lin.ctypes.data,
                      o_se.ctypes.data, None, None, *extra) == -1
            assert word in err(), (word, err())
    assert lib.rtk_upsample(None, C.byref(cam), 0, low.ctypes.data, low_se.ctypes.data, low_g.ctypes.data, g.ctypes.data, None, o_lin.ctypes.data, None, None, None,
                            None) == -1 and "null context" in err()
    assert np.all(o_lin == -3.0) and np.all(o_se == -3.0)
    with pytest.raises(TypeError):
        rt.Renderer.upsample_device(None, cam, 0, 0, 0, 0, sigma=1.0)   # an unknown option never reaches the library
    with pytest.raises(TypeError):
        rt.Renderer.upsample(None, cam, low, low_se, low_g, g, sigma_l=1.0)


@pytest.mark.parametrize("case", CPU_CASES, ids=["%dx%d/%d" % c for c in CPU_CASES])
def test_restatement_has_the_rules_properties(case):
    w, h, f = case
    lw, lh = low_size(w, h, f)
    low, low_se, low_g, g = random_case(w, h, f, 100 * w + f)
    for opts in (DEFAULTS, OTHER):
        out, var, support, s_beta = reference_upsample(w, h, f, low, low_se, low_g, g, **opts)
        assert s_beta.min() >= 0.39 and s_beta.max() <= 1.0 + 1e-6                       # no pixel is without taps
        assert np.isfinite(out).all() and (support >= 0).all() and (support <= 1 + 1e-9).all()
        assert (np.sqrt(var) <= low_se.max() * (1 + 1e-9)).all()                        # out_noise <= max se
        assert (out.min() >= low.astype(np.float32).min() - 1e-6) and (out.max() <= low.astype(np.float32).max() + 1e-6)   # a convex combination
        # a constant colour stays constant
        const = np.broadcast_to(np.array([0.25, 1.5, 0.75]), (lh, lw, 3))
        assert np.abs(reference_upsample(w, h, f, const, low_se, low_g, g, **opts)[0] - const[0, 0]).max() <= 1e-6
        # demodulated: a colour that is a constant times the low albedo comes out as the constant times the FULL albedo
        E = np.array([0.9, 0.4, 1.3])
        textured = E * np.maximum(low_g[..., 8:11].astype(np.float64), 0.02)
        demod = reference_upsample(w, h, f, textured, low_se, low_g, g, demodulate=True, **opts)[0]
        want = E * np.maximum(g[..., 8:11].astype(np.float64), 0.02)
        assert (np.abs(demod - want) / want).max() <= 1e-6
    # uniform guides: every tap is accepted, the result is the bilinear interpolation
    out, var, support, _ = reference_upsample(w, h, f, low, low_se, uniform_guides(lh, lw), uniform_guides(h, w))
    assert np.abs(support - 1.0).max() <= 1e-12
    assert np.abs(out - bilinear(w, h, f, low.astype(np.float32))).max() <= 1e-6
    assert (np.sqrt(var) <= low_se.max() * (1 + 1e-9)).all()
    # a background pixel (all-zero normals) among surface taps: support 0, the bilinear value
    gb = uniform_guides(h, w)
    pj, pi = h // 2, w // 3
    gb[pj, pi] = 0.0
    out, _, support, _ = reference_upsample(w, h, f, low, low_se, uniform_guides(lh, lw), gb)
    assert support[pj, pi] == 0.0
    assert np.abs(out - bilinear(w, h, f, low.astype(np.float32))).max() <= 1e-6
    mask = np.ones((h, w), bool)
    mask[pj, pi] = False
    # (a neighbour's depth gradient sees the hole; its own taps are all alike, so its support stays 1)
    assert np.abs(support[mask] - 1.0).max(initial=0) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- GPU --
@pytest.fixture(scope="module")
def scenes(rt):
    from tests.test_guided_denoise import build_test_room

    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build_test_room() if name == "test_room" else rt.Scene.build(name, rt.SCENE_SEED, EARTH)
        return cache[name]
    return get


def synthetic_case(rt, w, h, f):
    """(full camera, low colour float64, low se, low guides, full guides): the analytic guides of tests/test_temporal.py seen by
    the full camera and by its low camera."""
    full = synthetic_camera(rt, w, h, (0.0, 2.0, 6.0))
    low = rt.upsample_camera(full, f)
    g, low_g = synthetic_guides(full), synthetic_guides(low)
    rng = np.random.default_rng(1000 * f + w)
    lw, lh = low_size(w, h, f)
    colour = 0.8 * low_g[..., 0:3].astype(np.float64) + rng.normal(0.0, 0.1, (lh, lw, 3))
    return full, colour, rng.uniform(0.05, 0.15, (lh, lw)).astype(np.float32), low_g, g


def rich_case(rt, w, h, f):
    """synthetic_case on the rich guides of tests/rule_inputs.py: two distinct guide sets, fractional hit fractions, short
    normals, textured albedo -- the same world seen by the full camera and by its low camera."""
    full = synthetic_camera(rt, w, h, (0.0, 2.0, 6.0))
    low = rt.upsample_camera(full, f)
    g, low_g = rich_guides(view_of(full)), rich_guides(view_of(low))
    rng = np.random.default_rng(3000 * f + w)
    lw, lh = low_size(w, h, f)
    se = rng.uniform(0.05, 0.15, (lh, lw)).astype(np.float32)
    return full, shade(low_g) + rng.normal(0.0, 1.0, (lh, lw, 3)) * se[..., None], se, low_g, g


def _rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("size", GPU_SIZES, ids=["%dx%d" % s for s in GPU_SIZES])
def test_device_equals_the_restatement(rt, renderer, size, f, demodulate, real_mode):
    w, h = size
    full, colour, se, low_g, g = synthetic_case(rt, w, h, f)
    if w >= 37:
        assert 0.3 < (g[..., 3] > 0).mean() < 1.0                 # surfaces and background in view
    for opts in (DEFAULTS, OTHER):
        out, out_se, rgb8, support = renderer.upsample(full, colour, se, low_g, g, factor=f, demodulate=demodulate, real_mode=real_mode, **opts)
        ref, ref_var, ref_support, _ = reference_upsample(w, h, f, colour, se, low_g, g, demodulate=demodulate, **opts)
        worst = (_rel(out, ref), _rel(out_se.astype(np.float64), np.sqrt(ref_var)), _rel(support.astype(np.float64), ref_support))
        print(size, f, demodulate, real_mode, opts["sigma_n"], "worst rel: colour %.3g se %.3g support %.3g" % worst,
              "support: mean %.3f min %.3f" % (float(support.mean()), float(support.min())))
        assert max(worst) <= 1e-4, worst                          # every pixel: the rule has no threshold
        assert np.array_equal(out, out.astype(np.float32).astype(np.float64))            # float32 colour arithmetic in both modes
        assert np.array_equal(rgb8, _to_byte(out))
        again = renderer.upsample(full, colour, se, low_g, g, factor=f, demodulate=demodulate, real_mode=real_mode, **opts)
        for x, y in zip(again, (out, out_se, rgb8, support)):
            assert np.array_equal(x, y)
        if w >= 37 and not demodulate:
            assert support.min() < 0.5 < support.mean()          # edges reject taps, surfaces accept them


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("size", GPU_SIZES, ids=["%dx%d" % s for s in GPU_SIZES])
def test_device_equals_the_restatement_on_rich_inputs(rt, renderer, size, f, demodulate, real_mode):
    """The same comparison on inputs that show every term of the rule (tests/test_rule_sensitivity.py): two distinct guide sets,
    fractional hit fractions, short normals whose cosines lie where cos^sigma_n is neither 0 nor 1, a textured seen albedo.
    Worst relative error on an MI355X over all cases: see DESIGN.md, "What the post-processing tests can see"."""
    w, h = size
    full, colour, se, low_g, g = rich_case(rt, w, h, f)
    for opts in (DEFAULTS, OTHER):
        out, out_se, rgb8, support = renderer.upsample(full, colour, se, low_g, g, factor=f, demodulate=demodulate, real_mode=real_mode, **opts)
        ref, ref_var, ref_support, _ = reference_upsample(w, h, f, colour, se, low_g, g, demodulate=demodulate, **opts)
        worst = (_rel(out, ref), _rel(out_se.astype(np.float64), np.sqrt(ref_var)), _rel(support.astype(np.float64), ref_support))
        partial = float(((support > 0.1) & (support < 0.9)).mean())
        print("rich", size, f, demodulate, real_mode, opts["sigma_n"], "worst rel: colour %.3g se %.3g support %.3g" % worst,
              "support: mean %.3f, share strictly between 0.1 and 0.9: %.3f" % (float(support.mean()), partial))
        assert max(worst) <= 1e-4, worst                          # every pixel: the rule has no threshold
        assert np.array_equal(out, out.astype(np.float32).astype(np.float64))            # float32 colour arithmetic in both modes
        assert np.array_equal(rgb8, _to_byte(out))
        again = renderer.upsample(full, colour, se, low_g, g, factor=f, demodulate=demodulate, real_mode=real_mode, **opts)
        for x, y in zip(again, (out, out_se, rgb8, support)):
            assert np.array_equal(x, y)
        if w >= 37:
            assert partial >= 0.1, partial                        # taps weighed, not only accepted or rejected


@pytest.fixture(scope="module")
def blocker(rt, scenes):
    from tests.test_streams import Blocker

    b = Blocker(rt, scenes("book1_final"))
    yield b
    b.r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_entry_point_forms_agree_and_run_on_the_callers_stream(rt, renderer, blocker, real_mode):
    """The device form on a caller stream behind a blocker (tests/test_streams.py's pattern): inputs made on the stream, no host
    wait; outputs equal the _host form's bit for bit, and an output given as NULL does not change the others."""
    import torch

    from tests.test_streams import _behind_blocker

    w, h, f = 37, 23, 3
    full, colour, se, low_g, g = synthetic_case(rt, w, h, f)
    dt, ndt = (torch.float64, np.float64) if real_mode == 0 else (torch.float32, np.float32)
    want = renderer.upsample(full, colour, se, low_g, g, factor=f, demodulate=True, real_mode=real_mode, **OTHER)
    base = [torch.from_numpy(x).to("cuda:0") for x in (colour.astype(ndt), se, low_g, g)]
    torch.cuda.synchronize()
    names = ("linear", "se", "rgb8", "support")

    def body(streams, keep):
        s = streams[0]
        with torch.cuda.stream(s):
            ins = [x + 0 for x in base]                           # the inputs are made on the stream
            result = {}
            for skip in (None, 0, 1, 2, 3):
                outs = [torch.full((h, w, 3), float("nan"), dtype=dt, device="cuda:0"), torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda:0"),
                        torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device="cuda:0"), torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda:0")]
                ptrs = [0 if k == skip else o.data_ptr() for k, o in enumerate(outs)]
                renderer.upsample_device(full, *[x.data_ptr() for x in ins], *ptrs, real_mode=real_mode, stream=s.cuda_stream, factor=f, demodulate=True, **OTHER)
                result.update({"%s without %s" % (n, "nothing" if skip is None else names[skip]): o for k, (n, o) in enumerate(zip(names, outs)) if k != skip})
            return result

    got = _behind_blocker("upsample f%d" % (64 if real_mode == 0 else 32), blocker, 1, body)
    assert len(got) == 4 + 4 * 3
    for key, value in got.items():
        ref = want[names.index(key.split(" without ")[0])]
        assert np.array_equal(value.astype(ref.dtype), ref), key
    assert (want[3] < 0.5).any() and (want[3] > 0.9).any()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_refusals_write_nothing(rt, renderer, real_mode):
    import torch

    lib = rt.hip_lib()
    w, h, f = 37, 23, 2
    full, colour, se, low_g, g = synthetic_case(rt, w, h, f)
    dt = torch.float64 if real_mode == 0 else torch.float32
    ins = [torch.from_numpy(colour).to("cuda:0", dtype=dt)] + [torch.from_numpy(x).to("cuda:0") for x in (se, low_g, g)]
    out, o_se = torch.full((h, w, 3), -3.0, dtype=dt, device="cuda:0"), torch.full((h, w), -3.0, dtype=torch.float32, device="cuda:0")
    o8, o_sup = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda:0"), torch.full((h, w), -3.0, dtype=torch.float32, device="cuda:0")
    outs = (out.data_ptr(), o_se.data_ptr(), o8.data_ptr(), o_sup.data_ptr())
    p = [x.data_ptr() for x in ins]
    ok, U = rt.UpsampleOpts(2, 0, 0, 0, 0, 0), rt.UpsampleOpts
    empty = rt.Camera.from_buffer_copy(bytes(full))
    empty.image_width = 0
    ctx = renderer._ctx
    cases = [(ctx, full, real_mode, p, U(5, 0, 0, 0, 0, 0), outs), (ctx, full, real_mode, p, U(2, 0, 0, 0, 4, 0), outs), (ctx, full, real_mode, p, U(2, 0, 0, 0, 0, 7), outs),
             (ctx, full, real_mode, p, U(2, -1.0, 0, 0, 0, 0), outs), (ctx, full, real_mode, p, U(2, 0, float("nan"), 0, 0, 0), outs),
             (ctx, full, real_mode, p, U(2, 0, 0, float("inf"), 0, 0), outs), (None, full, real_mode, p, ok, outs), (ctx, empty, real_mode, p, ok, outs),
             (ctx, full, 2, p, ok, outs)]
    cases += [(ctx, full, real_mode, [None if k == m else x for k, x in enumerate(p)], ok, outs) for m in range(4)]
    for c, cam, mode, inputs, opts, o in cases:
        assert lib.rtk_upsample(c, C.byref(cam), mode, *inputs, C.byref(opts), *o, None) == -1, lib.rtk_last_error()
        assert "rtk_upsample:" in lib.rtk_last_error().decode()
    assert lib.rtk_upsample(ctx, None, real_mode, *p, C.byref(ok), *outs, None) == -1
    assert lib.rtk_upsample(ctx, C.byref(full), real_mode, *p, C.byref(ok), None, None, None, None, None) == -1 and "no output" in lib.rtk_last_error().decode()
    h_out = np.full((h, w, 3), -3.0)
    host = (colour.ctypes.data, se.ctypes.data, low_g.ctypes.data, g.ctypes.data)
    assert lib.rtk_upsample_host(ctx, C.byref(full), real_mode, *host, C.byref(U(1, 0, 0, 0, 0, 0)), h_out.ctypes.data, None, None, None) == -1
    assert lib.rtk_upsample_host(ctx, C.byref(full), real_mode, host[0], None, host[2], host[3], C.byref(ok), h_out.ctypes.data, None, None, None) == -1
    assert lib.rtk_upsample_host(ctx, C.byref(full), real_mode, *host, C.byref(ok), None, None, None, None) == -1
    assert lib.rtk_upsample_host(ctx, C.byref(empty), real_mode, *host, C.byref(ok), h_out.ctypes.data, None, None, None) == -1
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((o_se == -3.0).all()) and bool((o8 == 77).all()) and bool((o_sup == -3.0).all()) and np.all(h_out == -3.0)
    with pytest.raises(ValueError):
        renderer.upsample(full, colour[:-1], se, low_g, g)
    # and the same arguments, accepted
    assert lib.rtk_upsample(ctx, C.byref(full), real_mode, *p, C.byref(ok), *outs, None) == 0
    torch.cuda.synchronize()
    assert bool((o_sup >= 0).all()) and bool(torch.isfinite(out).all())


def _frame(renderer, cam, seed, real_mode=0):
    p = renderer.progressive(cam, seed=seed, real_mode=real_mode)
    linear, _, noise = p.step(cam.samples_per_pixel)
    p.close()
    return linear, noise


@pytest.mark.gpu
def test_upsampling_changes_no_render_guide_denoise_or_temporal_step(rt, renderer, scenes):
    scene = scenes("book1_final")
    renderer.upload(scene)
    w, h = 160, 90
    cam = scene.camera(w, h, 16, 10)
    low = rt.upsample_camera(cam, 2)

    def everything():
        lin, rgb8, _ = renderer.render_host(cam)
        g = renderer.guides(cam, 4)
        linear, noise = _frame(renderer, cam, 5)
        t = renderer.temporal(w, h)
        t.accumulate(cam, linear, g, noise)
        acc = t.accumulate(cam, lin, g, noise)
        t.close()
        return (lin, rgb8, g, linear, noise, renderer.denoise_guided(linear, g, noise)[0]) + acc

    before = everything()
    low_linear, low_noise = _frame(renderer, low, 6)
    low_g = renderer.guides(low, 4)
    first = renderer.upsample(cam, low_linear, low_noise, low_g, before[2])
    for demodulate in (False, True):
        renderer.upsample(cam, low_linear, low_noise, low_g, before[2], demodulate=demodulate, real_mode=1)
    during = everything()
    second = renderer.upsample(cam, low_linear, low_noise, low_g, before[2])
    for x, y in zip(before, during):
        assert np.array_equal(x, y)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_low_camera_sees_the_box_average_of_the_full_frame(rt, renderer, scenes):
    """The low camera's pixel integrates exactly its f x f full pixels: its frame and the box average of a full frame differ by
    noise only.  Bound: the mean |difference| of two unbiased estimates with standard errors se_a, se_b is about
    0.8 sqrt(se_a^2 + se_b^2); 4 x the combined mean se is a loose bound for that (measured: 0.88 x)."""
    scene = scenes("cornell_box")
    renderer.upload(scene)
    f, w = 2, 96
    cam = scene.camera(w, w, 64, 10)
    low = rt.upsample_camera(cam, f)
    assert (low.image_width, low.image_height, low.samples_per_pixel) == (48, 48, 64)
    low_linear, low_se = _frame(renderer, low, 41)
    assert np.array_equal(renderer.render_host(low, seed=41)[0], low_linear)
    linear, se = _frame(renderer, cam, 42)
    box = linear.reshape(48, f, 48, f, 3).mean((1, 3))
    box_se = np.sqrt((se.astype(np.float64) ** 2).reshape(48, f, 48, f).sum((1, 3))) / (f * f)
    combined = np.sqrt(low_se.astype(np.float64) ** 2 + box_se ** 2)
    diff = np.abs(low_linear.mean(-1) - box.mean(-1))
    print("cornell_box 96x96 / 2, 64 spp: mean |low - box| %.5f, combined mean se %.5f" % (diff.mean(), combined.mean()))
    assert combined.mean() > 0
    assert diff.mean() <= 4.0 * combined.mean()


@pytest.mark.gpu
def test_camera_renders_at_reduced_resolution(rt, tmp_path):
    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "upsample_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "upsample_camera_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])
    name, w, h, spp, depth, dx = "cornell_box", 64, 64, 16, 8, 6.0
    text = subprocess.check_output([exe, str(tmp_path), name, EARTH, str(w), str(h), str(spp), str(depth), str(dx)], timeout=300).decode()
    v = json.loads(text.strip().splitlines()[-1])
    assert v == {"upsampled": [1, 1, 0, 0, 1, 1], "frames": [0, 0, 0, 0, 1, 2]}, v

    r = rt.Renderer(0)
    scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
    view = lambda k, n: rt.derive_camera(w, 1.0, spp=n, max_depth=depth, vfov=40.0, lookfrom=(278.0 + dx * k, 278.0, -800.0), lookat=(278.0, 278.0, 0.0))  # noqa: E731
    assert bytes(view(0, spp)) == bytes(scene.camera(w, h, spp, depth))

    def upload(cam):
        info = r.upload_fast(scene, cam.center)                   # camera::auto_order: the fast order where it is proven exact
        if info["exactness"] != 2:
            r.upload(scene)

    def upsampled(cam, seed, demodulate=False):
        low = rt.upsample_camera(cam, 2)
        low_linear, low_noise = _frame(r, low, seed)
        g = r.guides(cam, 4, seed=seed)
        return r.upsample(cam, low_linear, low_noise, r.guides(low, 4, seed=seed), g, demodulate=demodulate), g

    cam = view(0, spp)
    upload(cam)
    (out, out_se, rgb8, _), g = upsampled(cam, rt.RENDER_SEED)
    assert np.array_equal(_read_png(str(tmp_path / "up.png")), rgb8)
    (out, out_se, rgb8, _), g = upsampled(cam, rt.RENDER_SEED, demodulate=True)
    assert np.array_equal(_read_png(str(tmp_path / "updemod.png")), rgb8)
    assert np.array_equal(_read_png(str(tmp_path / "den.png")), r.denoise_guided(out, g, out_se)[1])
    one8 = r.render_host(cam)[1]
    assert np.array_equal(_read_png(str(tmp_path / "plain.png")), one8)                  # render_scale = 1: the one-shot image
    assert not np.array_equal(_read_png(str(tmp_path / "up.png")), one8)
    assert np.array_equal(_read_png(str(tmp_path / "low.png")), r.render_host(view(0, 8))[1])   # too few samples: rendered at full resolution
    t = r.temporal(w, h)
    for k in range(2):
        cam = view(k, spp)
        upload(cam)
        (out, out_se, _, _), g = upsampled(cam, rt.RENDER_SEED + k)   # camera::seed + frames accumulated so far
        acc = t.accumulate(cam, out, g, out_se, max_history=8)
        assert np.array_equal(_read_png(str(tmp_path / ("ut%d.png" % k))), acc[2]), k
    assert (acc[3] > 1).mean() > 0.5
    t.close()
    r.close()


# MSE ratios against a 16-spp full-resolution frame (A) at equal sample budget, measured on an MI355X ("Guided
# upsampling"): B = a 64-spp half-resolution frame upsampled, C = the same demodulated; "filtered" = after rtk_denoise_guided on
# both sides.  The test allows each measured ratio + 15 %, the margin of tests/test_temporal.py.  Ratios above 1 are findings, not
# targets: at equal budget the demodulated frame loses to the plain one (light bleeds across the borders of emitters, where no
# albedo weight holds it back) and the guided filter does less for an upsampled frame, whose noise is correlated between
# neighbours, than for a full-resolution one (DESIGN.md has the split by region).
REAL_RATIOS_MEASURED = {
    "test_room": {"B/A": 0.7571, "C/A": 1.0426, "filtered B/A": 1.8100, "filtered C/A": 2.0592},
    "cornell_box": {"B/A": 0.4724, "C/A": 1.6845, "filtered B/A": 2.1391, "filtered C/A": 8.8381},
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("test_room", 160), ("cornell_box", 200)], ids=["test_room", "cornell_box"])
def test_real_frames_at_equal_sample_budget(rt, renderer, scenes, case):
    from tests.test_guided_denoise import room_camera

    name, w = case
    scene = scenes(name)
    renderer.upload(scene)
    camera = (lambda spp: room_camera(rt, w, spp)) if name == "test_room" else (lambda spp: scene.camera(w, w, spp, 10))
    cam = camera(16)
    low = rt.upsample_camera(camera(64), 2)
    a, a_se = _frame(renderer, cam, 31)
    low_linear, low_se = _frame(renderer, low, 32)
    g, low_g = renderer.guides(cam, 4), renderer.guides(low, 4)
    b, b_se, _, b_support = renderer.upsample(cam, low_linear, low_se, low_g, g)
    c, c_se, _, _ = renderer.upsample(cam, low_linear, low_se, low_g, g, demodulate=True)
    d = np.repeat(np.repeat(low_linear, 2, 0), 2, 1)[:w, :w]
    truth, _, _ = renderer.render_host(camera(1024), seed=1031)
    mse = lambda img: float(((img - truth) ** 2).sum(-1).mean())  # noqa: E731
    fa, fb, fc = (renderer.denoise_guided(x, g, s)[0] for x, s in ((a, a_se), (b, b_se), (c, c_se)))
    m = {"A": mse(a), "B": mse(b), "C": mse(c), "D": mse(d), "filtered A": mse(fa), "filtered B": mse(fb), "filtered C": mse(fc)}
    ratios = {"B/A": m["B"] / m["A"], "C/A": m["C"] / m["A"], "filtered B/A": m["filtered B"] / m["filtered A"], "filtered C/A": m["filtered C"] / m["filtered A"]}
    print(name, "%dx%d, 16 spp full against 64 spp at half resolution:" % (w, w), json.dumps({"mse": m, "ratios": ratios, "mean support": float(b_support.mean())}))
    if name == "test_room":
        assert m["C"] < m["D"], m                                 # demodulated upsampling beats replicated pixels where there are textures
    else:
        assert m["B"] < m["D"], m                                 # plain upsampling beats replicated pixels
    for key, measured in REAL_RATIOS_MEASURED[name].items():
        assert measured is not None, "the measured ratio %s of %s has not been recorded" % (key, name)
        assert ratios[key] <= 1.15 * measured, (key, ratios[key], measured)
