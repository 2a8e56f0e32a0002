"""Temporal accumulation (rtk_temporal_*): the frames of a moving camera reprojected, checked against the surface and blended.

CPU tests: the entry points are declared and exported; rtk_temporal_reproject_matrix maps a point back to its pixel; the numpy
restatement of the rule below averages a static camera's frames exactly and, on the synthetic camera paths, leaves out only a
handful of pixels as too close to a threshold ("fragile"); option refusals need no device.
GPU tests (-m gpu): the device equals the restatement step by step (the restatement takes the previous frame's DEVICE outputs
as its history, so one flipped threshold does not propagate); real frames under a static and a moving camera; the entry-point
forms, aliasing, a caller stream and refusals; nothing else on the context moves; the C++ camera."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import EARTH, ROOT
from tests.rule_inputs import rich_guides, shade, view_of
from tests.test_denoise import _read_png, _to_byte

ENTRY_POINTS = ("rtk_temporal_create", "rtk_temporal_accumulate", "rtk_temporal_accumulate_host", "rtk_temporal_reset", "rtk_temporal_frames",
                "rtk_temporal_destroy", "rtk_temporal_reproject_matrix")
DEFAULTS = {"max_history": 32, "depth_tol": 0.02, "normal_cos": 0.9, "albedo_tol": 0.25, "check_albedo": False}
OTHER = {"max_history": 3, "depth_tol": 0.05, "normal_cos": 0.5, "check_albedo": True}     # the issue's non-default set
FRAGILE = 1e-3


# ------------------------------------------------------------------------------------------------------ numpy reference --
def _v(v):
    return np.array([v.x, v.y, v.z], np.float64)


# Deliberate one-term deviations from the rule: what a subtly wrong kernel would compute.  tests/test_rule_sensitivity.py shows
# that the device comparison's inputs tell each of them from the rule; none is ever run against the device.
VARIANTS = ("cos_without_lengths", "hit_below_1", "tap_hit_nonzero", "depth_test_relative_to_tap", "albedo_check_first", "history_first_albedo",
            "history_end_hit", "variance_omega", "no_history_cap")


def reference_temporal(cam, linear, guides, noise, prev=None, max_history=32, depth_tol=0.02, normal_cos=0.9, albedo_tol=0.25, check_albedo=False, variant=None):
    """include/rtk.h, "Temporal accumulation", in float64.  prev = None (start of a history) or a dict of the previous frame:
    "color" (H, W, 3), "var" (H, W), "n" (H, W), "guides" (H, W, 16), "matrix" = rtk_temporal_reproject_matrix of its camera.
    Returns (out, var_out, n_out, has_history, margin): margin = how far the pixel's nearest decision is from its threshold
    (the minimum over taps in the image with g'[3] > 0 and omega > 1e-6 of ||dz| - lim| / lim and |cos - normal_cos|, and
    |Omega - 1e-3| / 1e-3).  variant: one of VARIANTS, a deliberately wrong rule (the margin stays the rule's)."""
    assert variant is None or variant in VARIANTS, variant
    f32 = lambda x: float(np.float32(x))  # noqa: E731  (the options are floats on the device)
    depth_tol, normal_cos, albedo_tol = f32(depth_tol), f32(normal_cos), f32(albedo_tol)
    c = np.asarray(linear, np.float32).astype(np.float64)
    se = np.asarray(noise, np.float32).astype(np.float64)
    var = se * se
    g = np.asarray(guides, np.float32).astype(np.float64)
    h, w = se.shape
    out, var_out, n_out = c.copy(), var.copy(), np.ones((h, w))
    has, margin = np.zeros((h, w), bool), np.full((h, w), np.inf)
    if prev is None:
        return out, var_out, n_out, has, margin
    pc = np.asarray(prev["color"], np.float32).astype(np.float64)
    pv = np.asarray(prev["var"], np.float32).astype(np.float64)
    pn = np.asarray(prev["n"], np.float32).astype(np.float64)
    pg = np.asarray(prev["guides"], np.float32).astype(np.float64)
    minv, pcen = np.asarray(prev["matrix"][0:9], np.float64).reshape(3, 3), np.asarray(prev["matrix"][9:12], np.float64)
    jj, ii = np.mgrid[0:h, 0:w]
    cen = _v(cam.center)
    d = _v(cam.pixel00_loc) + ii[..., None] * _v(cam.pixel_delta_u) + jj[..., None] * _v(cam.pixel_delta_v) - cen
    with np.errstate(invalid="ignore", divide="ignore"):
        q = cen + g[..., 7:8] * d / np.sqrt((d * d).sum(-1, keepdims=True)) - pcen
        uvw = q @ minv.T
        x, y = uvw[..., 0] / uvw[..., 2], uvw[..., 1] / uvw[..., 2]
    z_exp = np.sqrt((q * q).sum(-1))
    cand = ((g[..., 3] >= 1) if variant == "hit_below_1" else (g[..., 3] != 0)) & (uvw[..., 2] > 0) & np.isfinite(x) & np.isfinite(y) & (np.abs(np.nan_to_num(x)) < 1e9) & (np.abs(np.nan_to_num(y)) < 1e9)
    x, y = np.where(cand, x, 0.0), np.where(cand, y, 0.0)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    nrm = g[..., 4:7]
    nzero, nlen = np.all(nrm == 0, -1), np.sqrt((nrm * nrm).sum(-1))
    lim = depth_tol * z_exp
    om_sum, c_sum, v_sum, n_sum = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    for b in (0, 1):
        for a in (0, 1):
            ti, tj = (x0 + a).astype(np.int64), (y0 + b).astype(np.int64)
            inside = cand & (ti >= 0) & (ti < w) & (tj >= 0) & (tj < h)
            ti, tj = np.clip(ti, 0, w - 1), np.clip(tj, 0, h - 1)
            om = ((fx if a else 1.0 - fx) * (fy if b else 1.0 - fy)).astype(np.float32).astype(np.float64)
            gq = pg[tj, ti]
            hit_q = gq[..., 3] > 0
            if variant == "tap_hit_nonzero":
                hit_q = gq[..., 3] != 0
            if variant == "history_end_hit":
                hit_q = gq[..., 11] > 0
            dz = np.abs(gq[..., 7] - z_exp)
            ok_z = dz <= (depth_tol * gq[..., 7] if variant == "depth_test_relative_to_tap" else lim)
            nq = gq[..., 4:7]
            nqzero = np.all(nq == 0, -1)
            with np.errstate(invalid="ignore", divide="ignore"):
                cos = np.nan_to_num((nrm * nq).sum(-1) / (nlen * np.sqrt((nq * nq).sum(-1))))
                m_z = np.abs(dz - lim) / lim
            ok_n = np.where(nzero | nqzero, nzero & nqzero, ((nrm * nq).sum(-1) if variant == "cos_without_lengths" else cos) >= normal_cos)
            a_p, a_q = g[..., 8:11], gq[..., 8:11]
            if variant == "albedo_check_first":
                a_p, a_q = g[..., 0:3], gq[..., 0:3]
            if variant == "history_first_albedo":
                a_q = gq[..., 0:3]
            ok_a = np.abs(a_p - a_q).max(-1) <= albedo_tol if check_albedo else True
            valid = inside & hit_q & ok_z & ok_n & ok_a
            weighed = inside & (gq[..., 3] > 0) & (om > 1e-6)
            margin = np.where(weighed, np.minimum(margin, np.nan_to_num(m_z, nan=0.0)), margin)
            margin = np.where(weighed & ~nzero & ~nqzero, np.minimum(margin, np.abs(cos - normal_cos)), margin)
            o = np.where(valid, om, 0.0)
            om_sum += o
            c_sum += o[..., None] * pc[tj, ti]
            v_sum += (o if variant == "variance_omega" else o * o) * pv[tj, ti]
            n_sum += o * pn[tj, ti]
    margin = np.where(cand, np.minimum(margin, np.abs(om_sum - 1e-3) / 1e-3), margin)
    has = cand & (om_sum >= 1e-3)
    safe = np.where(has, om_sum, 1.0)
    n_new = n_sum / safe + 1.0 if variant == "no_history_cap" else np.minimum(n_sum / safe + 1.0, float(max_history))
    alpha = 1.0 / n_new
    out = np.where(has[..., None], (1 - alpha)[..., None] * (c_sum / safe[..., None]) + alpha[..., None] * c, c)
    var_out = np.where(has, (1 - alpha) ** 2 * (v_sum / (safe * safe)) + alpha ** 2 * var, var)
    n_out = np.where(has, n_new, 1.0)
    return out, var_out, n_out, has, margin


# ----------------------------------------------------------------------------------------------------- synthetic inputs --
SIZES = [(64, 48), (37, 23), (8, 8), (1, 1)]
PATHS = ("static", "orbit", "dolly")
ALBEDO = {"ground": (0.5, 0.5, 0.5), "wall": (0.8, 0.3, 0.2), "sphere": (0.2, 0.4, 0.8)}
N_FRAMES = 6


def path_lookfrom(path, k):
    if path == "static":
        return (0.0, 2.0, 6.0)
    if path == "orbit":
        a = math.radians(2.0 * k)
        return (6.0 * math.sin(a), 2.0 + 0.1 * k, 6.0 * math.cos(a))
    return (0.2 * k, 2.0, 6.0 - 0.3 * k)


def synthetic_camera(rt, w, h, lookfrom):
    cam = rt.derive_camera(w, w / (h + 0.25), vfov=40.0, focus_dist=10.0, lookfrom=lookfrom, lookat=(0.0, 1.0, 0.0))   # int(w / aspect) == h
    assert (cam.image_width, cam.image_height) == (w, h)
    return cam


def synthetic_guides(cam):
    """Guides of the analytic scene per pixel centre: ground y = 0 (|x|, |z| < 8), wall x = -3 (0 < y < 3, |z| < 4), unit sphere
    at (0, 1, 0).  Hit fraction 0 / 1, depth = distance, unit normals, flat albedos, set 2 = set 1."""
    h, w = cam.image_height, cam.image_width
    jj, ii = np.mgrid[0:h, 0:w]
    o = _v(cam.center)
    d = _v(cam.pixel00_loc) + ii[..., None] * _v(cam.pixel_delta_u) + jj[..., None] * _v(cam.pixel_delta_v) - o
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    best = np.full((h, w), np.inf)
    g = np.zeros((h, w, 8))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = -o[1] / d[..., 1]
        p = o + t[..., None] * d
        ok = (t > 0) & (np.abs(p[..., 0]) < 8) & (np.abs(p[..., 2]) < 8)
        best = np.where(ok, t, best)
        g[ok] = np.concatenate([ALBEDO["ground"], [1.0], [0.0, 1.0, 0.0], [0.0]])
        t = (-3.0 - o[0]) / d[..., 0]
        p = o + t[..., None] * d
        ok = (t > 0) & (t < best) & (p[..., 1] > 0) & (p[..., 1] < 3) & (np.abs(p[..., 2]) < 4)
        best = np.where(ok, t, best)
        g[ok] = np.concatenate([ALBEDO["wall"], [1.0], [1.0, 0.0, 0.0], [0.0]])
        oc = o - np.array([0.0, 1.0, 0.0])
        bq = (d * oc).sum(-1)
        disc = bq * bq - ((oc * oc).sum() - 1.0)
        t = -bq - np.sqrt(disc)
        ok = (disc > 0) & (t > 0) & (t < best)
        best = np.where(ok, t, best)
        nrm = o + np.where(ok, t, 0.0)[..., None] * d - np.array([0.0, 1.0, 0.0])
        g[ok, 0:3] = ALBEDO["sphere"]
        g[ok, 3] = 1.0
        g[ok, 4:7] = nrm[ok]
    g[..., 7] = np.where(np.isfinite(best), best, 0.0)
    g[g[..., 3] == 0] = 0.0
    g32 = g.astype(np.float32)
    return np.concatenate([g32, g32], -1)


def synthetic_frames(rt, path, w, h):
    """[(camera, colour float64 (H, W, 3), guides float32 (H, W, 16), se float32 (H, W))] of the path's six frames."""
    rng = np.random.default_rng(1000 * PATHS.index(path) + w)
    frames = []
    for k in range(N_FRAMES):
        cam = synthetic_camera(rt, w, h, path_lookfrom(path, k))
        g = synthetic_guides(cam)
        colour = 0.8 * g[..., 0:3].astype(np.float64) + rng.normal(0.0, 0.1, (h, w, 3))
        frames.append((cam, colour, g, np.full((h, w), 0.1, np.float32)))
    return frames


def rich_frames(rt, path, w, h):
    """synthetic_frames on the rich guides of tests/rule_inputs.py: the same cameras, every guide channel a function of the world
    point, a shaded colour and an se that varies per pixel."""
    rng = np.random.default_rng(2000 * PATHS.index(path) + w)
    frames = []
    for k in range(N_FRAMES):
        cam = synthetic_camera(rt, w, h, path_lookfrom(path, k))
        g = rich_guides(view_of(cam))
        se = (0.05 + 0.1 * rng.random((h, w))).astype(np.float32)
        frames.append((cam, shade(g) + rng.normal(0.0, 1.0, (h, w, 3)) * se[..., None], g, se))
    return frames


def fragile_cap(w, h):
    """Most pixels of a frame the comparison may leave out: 2 %, one pixel at 8x8, none at 1x1."""
    return 0 if w * h == 1 else (1 if w * h <= 64 else int(0.02 * w * h))


def _history(rt, cam, out, var, n, guides):
    return {"color": out, "var": var, "n": n, "guides": guides, "matrix": rt.temporal_reproject_matrix(cam)}


# ---------------------------------------------------------------------------------------------------------------- CPU --
def test_header_declares_and_library_exports_the_temporal_api(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, body), name
    assert re.search(r"typedef struct rtk_temporal_opts\b", body) and re.search(r"typedef struct rtk_temporal rtk_temporal;", body)
    assert re.search(r"#define RTK_TEMPORAL_CHECK_ALBEDO 1\b", body)
    assert "#define RTK_ABI_VERSION 2" in body                    # new entry points only
    lib = C.CDLL(rt.HIP_LIB_PATH)                                 # loads without a GPU
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert C.sizeof(rt.TemporalOpts) == 24 and rt.TEMPORAL_CHECK_ALBEDO == 1
    for name in ("temporal", ):
        assert hasattr(rt.Renderer, name)
    for name in ("accumulate", "accumulate_device", "reset", "frames", "close"):
        assert hasattr(rt.Temporal, name), name


def test_reproject_matrix_returns_a_point_to_its_pixel(rt):
    cam = rt.derive_camera(200, 200 / 113.0, vfov=35.0, lookfrom=(3.0, 2.5, -7.0), lookat=(0.5, 1.0, 0.25), vup=(0.1, 1.0, 0.0), focus_dist=4.0)
    m = rt.temporal_reproject_matrix(cam)
    assert m.shape == (12,) and np.array_equal(m[9:12], _v(cam.center))
    cols = np.stack([_v(cam.pixel_delta_u), _v(cam.pixel_delta_v), _v(cam.pixel00_loc) - _v(cam.center)], 1)
    assert np.abs(m[0:9].reshape(3, 3) @ cols - np.eye(3)).max() < 1e-9
    rng = np.random.default_rng(2)
    i, j = rng.uniform(-20, 220, 200), rng.uniform(-20, 133, 200)
    depth = 10.0 ** rng.uniform(-2, 4, 200)
    d = _v(cam.pixel00_loc) + i[:, None] * _v(cam.pixel_delta_u) + j[:, None] * _v(cam.pixel_delta_v) - _v(cam.center)
    p = _v(cam.center) + depth[:, None] * d / np.sqrt((d * d).sum(-1, keepdims=True))
    q = p - m[9:12]
    uvw = q @ m[0:9].reshape(3, 3).T
    assert (uvw[:, 2] > 0).all()
    assert np.abs(uvw[:, 0] / uvw[:, 2] - i).max() <= 1e-9 and np.abs(uvw[:, 1] / uvw[:, 2] - j).max() <= 1e-9
    assert (np.abs(np.sqrt((q * q).sum(-1)) - depth) / depth).max() <= 1e-12
    flat = rt.derive_camera(200, 200 / 113.0)
    flat.pixel_delta_u = rt.Vec3(0.0, 0.0, 0.0)
    with pytest.raises(rt.RtkError) as e:
        rt.temporal_reproject_matrix(flat)
    assert e.value.code == -1 and "singular" in str(e.value)
    out = (C.c_double * 12)(*([-7.0] * 12))
    assert rt.hip_lib().rtk_temporal_reproject_matrix(C.byref(flat), out) == -1 and list(out) == [-7.0] * 12
    assert rt.hip_lib().rtk_temporal_reproject_matrix(None, out) == -1


def _chain_reference(rt, frames, opts):
    """The restatement run on its own outputs (rounded to float32, as the device keeps them): per frame (out, var, n, has, margin)."""
    prev, results = None, []
    for cam, colour, g, se in frames:
        out, var, n, has, margin = reference_temporal(cam, colour, g, se, prev, **opts)
        results.append((out, var, n, has, margin))
        prev = _history(rt, cam, out.astype(np.float32), var.astype(np.float32), n.astype(np.float32), g)
    return results


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_restatement_averages_a_static_camera(rt, size):
    w, h = size
    frames = synthetic_frames(rt, "static", w, h)
    hit = frames[0][2][..., 3] > 0
    if w >= 37:
        assert 0.3 < hit.mean() < 1.0                              # surfaces and background in view
    results = _chain_reference(rt, frames, DEFAULTS)
    shown = np.stack([f[1].astype(np.float32).astype(np.float64) for f in frames])
    # the static camera reprojects every pixel onto itself
    m = rt.temporal_reproject_matrix(frames[0][0])
    jj, ii = np.mgrid[0:h, 0:w]
    cam = frames[0][0]
    d = _v(cam.pixel00_loc) + ii[..., None] * _v(cam.pixel_delta_u) + jj[..., None] * _v(cam.pixel_delta_v) - _v(cam.center)
    uvw = (7.5 * d / np.sqrt((d * d).sum(-1, keepdims=True))) @ m[0:9].reshape(3, 3).T
    assert np.abs(uvw[..., 0] / uvw[..., 2] - ii).max() <= 1e-12 * max(w, 8) and np.abs(uvw[..., 1] / uvw[..., 2] - jj).max() <= 1e-12 * max(h, 8)
    for k, (out, var, n, has, _) in enumerate(results, 1):
        assert np.array_equal(has, hit if k > 1 else np.zeros_like(hit))
        assert np.abs(n[hit] - k).max(initial=0) <= 1e-9 and (n[~hit] == 1).all()
        assert np.abs(out[hit] - shown[:k].mean(0)[hit]).max(initial=0) <= 1e-6
        assert (np.abs(var[hit] - 0.01 / k) / (0.01 / k)).max(initial=0) <= 1e-6
        assert np.array_equal(out[~hit], shown[k - 1][~hit])
    capped = _chain_reference(rt, frames, dict(DEFAULTS, max_history=3))
    assert np.abs(capped[-1][2][hit] - 3).max(initial=0) <= 1e-9 and (capped[-1][1][hit] > 0.01 / 5).all()    # v = (2/3)^2 v + 0.01 / 9 settles at 0.01 / 5, from above


@pytest.mark.parametrize("opts", [DEFAULTS, OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("path", ["orbit", "dolly"])
def test_restatement_leaves_few_pixels_out(rt, path, opts):
    found = []
    for w, h in SIZES:
        frames = synthetic_frames(rt, path, w, h)
        for k, (out, var, n, has, margin) in enumerate(_chain_reference(rt, frames, opts)):
            fragile = int((margin < FRAGILE).sum())
            assert fragile <= fragile_cap(w, h), (path, w, h, k, fragile)
            assert np.isfinite(out).all() and (var >= 0).all() and (n >= 1).all() and (n <= opts["max_history"]).all()
            if k > 0 and w >= 37:
                found.append(has.mean())
                assert (n[has] > 1).all() and (n[~has] == 1).all()
    print(path, "share of pixels with history: %.3f .. %.3f" % (min(found), max(found)))
    assert 0.3 < min(found) and max(found) < 0.9


@pytest.mark.parametrize("opts", [DEFAULTS, OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("path", ["orbit", "dolly"])
def test_restatement_leaves_few_pixels_out_of_the_rich_frames(rt, path, opts):
    """test_restatement_leaves_few_pixels_out on rich_frames: the same margin rule and the same cap."""
    found = []
    for w, h in SIZES:
        frames = rich_frames(rt, path, w, h)
        for k, (out, var, n, has, margin) in enumerate(_chain_reference(rt, frames, opts)):
            fragile = int((margin < FRAGILE).sum())
            assert fragile <= fragile_cap(w, h), (path, w, h, k, fragile)
            assert np.isfinite(out).all() and (var >= 0).all() and (n >= 1).all() and (n <= opts["max_history"]).all()
            if k > 0 and w >= 37:
                found.append(has.mean())
                assert (n[has] > 1).all() and (n[~has] == 1).all()
    print(path, "share of pixels with history: %.3f .. %.3f" % (min(found), max(found)))
    assert 0.3 < min(found) and max(found) < 0.9


def test_option_refusals_need_no_device(rt):
    """Options are checked before anything else: with no object at all, a bad option is what the error names."""
    lib = rt.hip_lib()
    err = lambda: lib.rtk_last_error().decode()  # noqa: E731
    cam = rt.derive_camera(16, 1.0)
    lin, g, noise = np.zeros((16, 16, 3)), np.zeros((16, 16, 16), np.float32), np.zeros((16, 16), np.float32)
    o_lin, o_noise = np.full((16, 16, 3), -3.0), np.full((16, 16), -3.0, np.float32)
    T = rt.TemporalOpts
    cases = ((T(0, 0, 0, 0, 2, 0), "flags"), (T(0, 0, 0, 0, -1, 0), "flags"), (T(0, 0, 0, 0, 0, 1), "reserved"), (T(-1, 0, 0, 0, 0, 0), "max_history"),
             (T(1025, 0, 0, 0, 0, 0), "max_history"), (T(0, -0.1, 0, 0, 0, 0), "tolerances"), (T(0, float("nan"), 0, 0, 0, 0), "tolerances"),
             (T(0, 0, 0, float("inf"), 0, 0), "tolerances"), (T(0, 0, -0.5, 0, 0, 0), "tolerances"), (T(0, 0, 1.5, 0, 0, 0), "normal_cos"),
             (T(0, 0, 0, -1.0, 1, 0), "tolerances"), (T(1024, 1.0, 1.0, 1.0, 1, 0), "null object"))
    for opts, word in cases:
        for f in (lib.rtk_temporal_accumulate, lib.rtk_temporal_accumulate_host):
            assert f(None, C.byref(cam), lin.ctypes.data, g.ctypes.data, noise.ctypes.data, C.byref(opts), o_lin.ctypes.data, o_noise.ctypes.data, None, None) == -1
            assert word in err(), (word, err())
    assert lib.rtk_temporal_accumulate(None, C.byref(cam), lin.ctypes.data, g.ctypes.data, noise.ctypes.data, None, o_lin.ctypes.data, None, None, None) == -1
    assert "null object" in err()
    assert np.all(o_lin == -3.0) and np.all(o_noise == -3.0)
    h = C.c_void_p()
    assert lib.rtk_temporal_create(None, 16, 16, 0, None, C.byref(h)) == -1 and not h.value
    assert lib.rtk_temporal_reset(None) == -1 and lib.rtk_temporal_frames(None) == -1 and lib.rtk_temporal_destroy(None) == 0
    with pytest.raises(TypeError):
        rt.Temporal.accumulate_device(None, cam, 0, 0, 0, sigma=1.0)  # an unknown option never reaches the library


# ---------------------------------------------------------------------------------------------------------------- GPU --
@pytest.fixture(scope="module")
def scenes(rt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
        return cache[name]
    return get


def _close(got, ref):
    return np.abs(got - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))


def _device_against_restatement(rt, renderer, frames, path, size, opts, real_mode):
    """The device, frame by frame, against the restatement run on the DEVICE's previous outputs; returns the worst relative
    errors (colour, se, n) over the chain."""
    w, h = size
    a, b = renderer.temporal(w, h, real_mode), renderer.temporal(w, h, real_mode)
    prev, compared, with_history, overall = None, 0, 0, [0.0, 0.0, 0.0]
    for k, (cam, colour, g, se) in enumerate(frames):
        out, out_se, rgb8, n = a.accumulate(cam, colour, g, se, **opts)
        ref, ref_var, ref_n, has, margin = reference_temporal(cam, colour, g, se, prev, **opts)
        keep = margin >= FRAGILE
        assert int((~keep).sum()) <= fragile_cap(w, h), (k, int((~keep).sum()))
        worst = [float((np.abs(x - y) / np.maximum(1.0, np.abs(y)))[m].max(initial=0)) for x, y, m in
                 ((out, ref, keep), (out_se.astype(np.float64), np.sqrt(ref_var), keep), (n.astype(np.float64), ref_n, keep))]
        overall = [max(x, y) for x, y in zip(overall, worst)]
        print(path, size, real_mode, "frame", k, "left out", int((~keep).sum()), "history", round(float(has.mean()), 3), "worst rel", worst)
        assert _close(out, ref)[keep].all(), (k, worst)
        assert _close(out_se.astype(np.float64), np.sqrt(ref_var))[keep].all(), (k, worst)
        assert (np.abs(n.astype(np.float64) - ref_n) <= 1e-4)[keep].all(), (k, worst)
        assert np.array_equal(out, out.astype(np.float32).astype(np.float64))        # float32 colour arithmetic in both modes
        assert np.array_equal(rgb8, _to_byte(out))
        if k == 0 or path == "static":
            assert np.array_equal(n > 1, has)
        again = b.accumulate(cam, colour, g, se, **opts)
        for x, y in zip(again, (out, out_se, rgb8, n)):
            assert np.array_equal(x, y)
        assert a.frames == k + 1
        prev = _history(rt, cam, out, out_se.astype(np.float64) ** 2, n, g)
        compared += int(keep.sum())
        with_history += int((has & keep).sum())
    assert compared >= N_FRAMES * (w * h - fragile_cap(w, h))
    if w >= 37:
        assert with_history > 0.3 * (N_FRAMES - 1) * w * h
    a.close()
    b.close()
    return overall


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("opts", [DEFAULTS, OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("path", PATHS)
def test_device_equals_the_restatement(rt, renderer, path, size, opts, real_mode):
    _device_against_restatement(rt, renderer, synthetic_frames(rt, path, *size), path, size, opts, real_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("opts", [DEFAULTS, OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("path", PATHS)
def test_device_equals_the_restatement_on_rich_frames(rt, renderer, path, size, opts, real_mode):
    """The same comparison on inputs that show every term of the rule (tests/test_rule_sensitivity.py): a seen albedo that is not
    the first one and crosses albedo_tol between frames, fractional hit fractions, short normals.  Worst relative error on an
    MI355X over all cases: see DESIGN.md, "What the post-processing tests can see"."""
    worst = _device_against_restatement(rt, renderer, rich_frames(rt, path, *size), path, size, opts, real_mode)
    print("rich", path, size, real_mode, "worst rel over the chain: colour %.3g se %.3g n %.3g" % tuple(worst))


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_first_frame_bytes_follow_the_reference_rule_and_linear_is_a_copy(rt, renderer, real_mode):
    """A first frame returns out = c: chosen colours reach to_byte directly.  Every byte threshold with its neighbours one
    and two float32 units in the last place away, the clamp's edge, zeros, negatives, infinities and NaN (tests/test_output_stage.py)
    must give that file's bytes, and the linear output the float input bit for bit."""
    from tests.test_output_stage import known_values, to_byte

    values = known_values(np.float32)
    w, h = 37, 23
    assert w * h * 3 >= len(values)
    colour = values[np.arange(h * w * 3) % len(values)].reshape(h, w, 3)
    cam, _, g, se = rich_frames(rt, "static", w, h)[0]
    t = renderer.temporal(w, h, real_mode)
    out, out_se, rgb8, n = t.accumulate(cam, colour.astype(np.float64), g, se)
    t.close()
    assert np.array_equal(out.astype(np.float32).view(np.uint32), colour.view(np.uint32))    # a copy, -0.0 and NaN included
    want = to_byte(colour.astype(np.float64))
    bad = np.argwhere(rgb8 != want)
    assert len(bad) == 0, [(float(colour[tuple(k)]).hex(), int(rgb8[tuple(k)]), int(want[tuple(k)])) for k in bad[:8]]
    assert len(set(rgb8.reshape(-1).tolist())) == 256 and (n == 1).all()


def _frame(renderer, cam, seed, real_mode):
    p = renderer.progressive(cam, seed=seed, real_mode=real_mode)
    linear, _, noise = p.step(cam.samples_per_pixel)
    p.close()
    return linear, noise


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("case", [("cornell_box", 200, 200), ("book1_final", 160, 90)], ids=["cornell_box", "book1_final"])
def test_real_frames_under_a_static_camera_are_averaged(rt, renderer, scenes, case, real_mode):
    name, w, h = case
    scene = scenes(name)
    renderer.upload(scene)
    cam = scene.camera(w, h, 16, 10)
    g = renderer.guides(cam, 4, real_mode=real_mode)
    hit = g[..., 3] > 0
    assert hit.mean() > 0.5
    t = renderer.temporal(w, h, real_mode)
    shown, variances = [], []
    for k in range(4):
        linear, noise = _frame(renderer, cam, 11 + k, real_mode)
        shown.append(linear.astype(np.float32).astype(np.float64))
        variances.append(noise.astype(np.float64) ** 2)
        out, out_se, rgb8, n = t.accumulate(cam, linear, g, noise)
    mean = np.stack(shown).mean(0)
    print(name, real_mode, "worst |colour - mean|", float(np.abs(out - mean)[hit].max()), "largest colour", float(mean[hit].max()))
    assert (n[hit] == 4).all() and (n[~hit] == 1).all()
    assert np.abs(out - mean)[hit].max() <= 1e-5
    assert np.array_equal(out[~hit], shown[3][~hit]) and np.array_equal(out_se[~hit], noise[~hit])
    want_se = np.sqrt(np.sum(variances, 0)) / 4.0                # four equal weights: var = sum se_k^2 / 16
    assert _close(out_se.astype(np.float64), want_se)[hit].all() and (want_se[hit] > 0).mean() > 0.5
    assert t.frames == 4
    t.reset()
    assert t.frames == 0
    out, out_se, rgb8, n = t.accumulate(cam, linear, g, noise)
    assert np.array_equal(out, shown[3]) and np.array_equal(out_se, noise) and (n == 1).all() and t.frames == 1
    assert np.array_equal(rgb8, _to_byte(out))
    t.close()


CORNELL_CENTRE = (278.0, 278.0, 278.0)


def cornell_orbit(rt, w, spp, k, depth=10):
    """The cornell_box view turned k degrees around the room's centre (k = 0: the scene's own eye point)."""
    a = math.radians(k)
    eye = (CORNELL_CENTRE[0] + 1078.0 * math.sin(a), 278.0, CORNELL_CENTRE[2] - 1078.0 * math.cos(a))
    return rt.derive_camera(w, 1.0, spp=spp, max_depth=depth, vfov=40.0, lookfrom=eye, lookat=CORNELL_CENTRE)


# MSE(accumulated) / MSE(the last 16-spp frame) at the last camera, measured on an MI355X ("Temporal accumulation");
# the test allows the measured ratio + 15 %.
MOVING_RATIO_MEASURED = 0.1625


@pytest.mark.gpu
def test_real_frames_under_a_moving_camera(rt, renderer, scenes):
    scene = scenes("cornell_box")
    renderer.upload(scene)
    w = h = 200
    t = renderer.temporal(w, h)
    prev = None
    for k in range(8):
        cam = cornell_orbit(rt, w, 16, k)
        linear, noise = _frame(renderer, cam, 21 + k, 0)
        g = renderer.guides(cam, 4)
        out, out_se, _, n = t.accumulate(cam, linear, g, noise)
        _, _, _, has, margin = reference_temporal(cam, linear, g, noise, prev)
        start = ~has & (margin >= FRAGILE)
        assert np.array_equal(out[start], linear.astype(np.float32).astype(np.float64)[start]) and (n[start] == 1).all(), k
        if k:
            assert has.mean() > 0.6 and start.sum() > 0, (k, has.mean(), start.sum())   # most of the room is carried along; some is uncovered
        prev = _history(rt, cam, out, out_se.astype(np.float64) ** 2, n, g)
    t.close()
    truth, _, _ = renderer.render_host(cornell_orbit(rt, w, 1024, 7), seed=1021)
    mse = lambda img: float(((img - truth) ** 2).sum(-1).mean())  # noqa: E731
    ratio = mse(out) / mse(linear)
    den_acc, _ = renderer.denoise_guided(out, g, out_se)
    den_one, _ = renderer.denoise_guided(linear, g, noise)
    ratio_filtered = mse(den_acc) / mse(den_one)
    print("cornell_box 200x200, 8 frames of 16 spp, 1 degree per frame:", json.dumps(
        {"mse_frame": mse(linear), "mse_accumulated": mse(out), "ratio": ratio, "mse_filtered_frame": mse(den_one), "mse_filtered_accumulated": mse(den_acc),
         "ratio_filtered": ratio_filtered, "mean_history": float(n.mean())}))
    assert ratio < 1.0
    assert MOVING_RATIO_MEASURED is not None, "the measured ratio has not been recorded"
    assert ratio <= 1.15 * MOVING_RATIO_MEASURED, ratio
    assert ratio_filtered < 1.0


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
    wait, three frames in flight; outputs equal the _host form's bit for bit, aliased or not."""
    import torch

    from tests.test_streams import _behind_blocker

    w, h = 37, 23
    frames = synthetic_frames(rt, "orbit", w, h)[:3]
    dt, ndt = (torch.float64, np.float64) if real_mode == 0 else (torch.float32, np.float32)
    host = renderer.temporal(w, h, real_mode)
    want = [host.accumulate(cam, colour, g, se, **OTHER) for cam, colour, g, se in frames]
    host.close()
    base = [(torch.from_numpy(colour.astype(ndt)).to("cuda:0"), torch.from_numpy(g).to("cuda:0"), torch.from_numpy(se).to("cuda:0")) for _, colour, g, se in frames]
    torch.cuda.synchronize()

    def body(streams, keep):
        s = streams[0]
        with torch.cuda.stream(s):
            plain, alias = renderer.temporal(w, h, real_mode, stream=s.cuda_stream), renderer.temporal(w, h, real_mode, stream=s.cuda_stream)
            keep.extend([plain, alias])                           # closed after the host was seen to be ahead: destroy waits for the stream
            result = {}
            for k, (cam, _, _, _) in enumerate(frames):
                lin, d_g, d_se = base[k][0] + 0, base[k][1] + 0, base[k][2] + 0      # the inputs are made on the stream
                out, o_se = torch.full((h, w, 3), float("nan"), dtype=dt, device="cuda:0"), torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda:0")
                o8, o_n = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device="cuda:0"), torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda:0")
                plain.accumulate_device(cam, lin.data_ptr(), d_g.data_ptr(), d_se.data_ptr(), out.data_ptr(), o_se.data_ptr(), o8.data_ptr(), o_n.data_ptr(), **OTHER)
                a_lin, a_se = lin.clone(), d_se.clone()
                alias.accumulate_device(cam, a_lin.data_ptr(), d_g.data_ptr(), a_se.data_ptr(), a_lin.data_ptr(), a_se.data_ptr(), 0, 0, **OTHER)
                result.update({"linear %d" % k: out.clone(), "se %d" % k: o_se.clone(), "rgb8 %d" % k: o8.clone(), "n %d" % k: o_n.clone(),
                               "aliased linear %d" % k: a_lin.clone(), "aliased se %d" % k: a_se.clone()})
            assert plain.frames == 3 and alias.frames == 3
            return result

    got = _behind_blocker("temporal f%d" % (64 if real_mode == 0 else 32), blocker, 1, body)
    for k, (out, out_se, rgb8, n) in enumerate(want):
        assert np.array_equal(got["linear %d" % k].astype(np.float64), out) and np.array_equal(got["se %d" % k], out_se)
        assert np.array_equal(got["rgb8 %d" % k], rgb8) and np.array_equal(got["n %d" % k], n)
        assert np.array_equal(got["aliased linear %d" % k], got["linear %d" % k]) and np.array_equal(got["aliased se %d" % k], got["se %d" % k])
    assert (want[2][3] > 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_refusals_write_nothing_and_keep_the_history(rt, renderer, real_mode):
    import torch

    lib = rt.hip_lib()
    w, h = 37, 23
    frames = synthetic_frames(rt, "dolly", w, h)
    dt = torch.float64 if real_mode == 0 else torch.float32
    t, twin = renderer.temporal(w, h, real_mode), renderer.temporal(w, h, real_mode)
    cam, colour, g, se = frames[0]
    t.accumulate(cam, colour, g, se)
    twin.accumulate(cam, colour, g, se)
    lin, d_g, d_se = torch.from_numpy(colour).to("cuda:0", dtype=dt), torch.from_numpy(g).to("cuda:0"), torch.from_numpy(se).to("cuda:0")
    out, o_se = torch.full((h, w, 3), -3.0, dtype=dt, device="cuda:0"), torch.full((h, w), -3.0, dtype=torch.float32, device="cuda:0")
    o8, o_n = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda:0"), torch.full((h, w), -3.0, dtype=torch.float32, device="cuda:0")
    outs = (out.data_ptr(), o_se.data_ptr(), o8.data_ptr(), o_n.data_ptr())
    ok = rt.TemporalOpts(0, 0, 0, 0, 0, 0)
    other_size = synthetic_camera(rt, 64, 48, (0.0, 2.0, 6.0))
    flat = synthetic_camera(rt, w, h, (0.0, 2.0, 6.0))
    flat.pixel_delta_v = rt.Vec3(0.0, 0.0, 0.0)
    moved = frames[1][0]
    for args, opts in (((other_size, lin.data_ptr(), d_g.data_ptr(), d_se.data_ptr()), ok), ((flat, lin.data_ptr(), d_g.data_ptr(), d_se.data_ptr()), ok),
                       ((moved, lin.data_ptr(), d_g.data_ptr(), d_se.data_ptr()), rt.TemporalOpts(0, 0, 0, 0, 4, 0)),
                       ((moved, lin.data_ptr(), d_g.data_ptr(), d_se.data_ptr()), rt.TemporalOpts(0, 0, 2.0, 0, 0, 0)),
                       ((moved, None, d_g.data_ptr(), d_se.data_ptr()), ok), ((moved, lin.data_ptr(), None, d_se.data_ptr()), ok),
                       ((moved, lin.data_ptr(), d_g.data_ptr(), None), ok)):
        assert lib.rtk_temporal_accumulate(t._h, C.byref(args[0]), *args[1:], C.byref(opts), *outs) == -1, lib.rtk_last_error()
        assert t.frames == 1
    assert lib.rtk_temporal_accumulate(t._h, None, lin.data_ptr(), d_g.data_ptr(), d_se.data_ptr(), C.byref(ok), *outs) == -1
    h_out = np.full((h, w, 3), -3.0)
    assert lib.rtk_temporal_accumulate_host(t._h, C.byref(other_size), colour.ctypes.data, g.ctypes.data, se.ctypes.data, C.byref(ok), h_out.ctypes.data, None, None, None) == -1
    assert lib.rtk_temporal_accumulate_host(t._h, C.byref(moved), colour.ctypes.data, None, se.ctypes.data, C.byref(ok), h_out.ctypes.data, None, None, None) == -1
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((o_se == -3.0).all()) and bool((o8 == 77).all()) and bool((o_n == -3.0).all()) and np.all(h_out == -3.0)
    assert t.frames == 1
    with pytest.raises(rt.RtkError):
        renderer.temporal(0, 5)
    with pytest.raises(rt.RtkError):
        renderer.temporal(8, 8, real_mode=2)
    # the history is what it was: the next frame equals the twin's, which saw no refusal
    cam, colour, g, se = frames[1]
    for x, y in zip(t.accumulate(cam, colour, g, se), twin.accumulate(cam, colour, g, se)):
        assert np.array_equal(x, y)
    assert (t.accumulate(*frames[2])[3] > 2).any()
    t.close()
    twin.close()


@pytest.mark.gpu
def test_temporal_objects_change_no_render_aov_or_denoise(rt, renderer, scenes):
    scene = scenes("book1_final")
    renderer.upload(scene)
    w, h = 160, 90
    cam = scene.camera(w, h, 16, 10)

    def everything():
        lin, rgb8, _ = renderer.render_host(cam)
        g = renderer.guides(cam, 4)
        linear, noise = _frame(renderer, cam, 5, 0)
        return lin, rgb8, renderer.aovs(cam, 4), g, linear, noise, renderer.denoise_guided(linear, g, noise)[0]

    before = everything()
    t = renderer.temporal(w, h)
    for k in range(3):
        linear, noise = _frame(renderer, cam, 30 + k, 0)
        t.accumulate(cam, linear, before[3], noise)
    during = everything()
    t.close()
    after = everything()
    for x, y, z in zip(before, during, after):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.gpu
def test_camera_keeps_a_history_between_render_calls(rt, tmp_path):
    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "temporal_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "temporal_camera_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])
    name, w, h, spp, depth, dx = "cornell_box", 64, 64, 16, 8, 6.0
    text = subprocess.check_output([exe, str(tmp_path), name, EARTH, str(w), str(h), str(spp), str(depth), str(dx)], timeout=300).decode()
    v = json.loads(text.strip().splitlines()[-1])
    assert v == {"frames": [1, 2, 3], "plain_frames": 0, "low_frames": 0}, v

    r = rt.Renderer(0)
    scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
    view = lambda k, n: rt.derive_camera(w, 1.0, spp=n, max_depth=depth, vfov=40.0, lookfrom=(278.0 + dx * k, 278.0, -800.0), lookat=(278.0, 278.0, 0.0))  # noqa: E731
    assert bytes(view(0, spp)) == bytes(scene.camera(w, h, spp, depth))

    def upload(cam):
        info = r.upload_fast(scene, cam.center)                   # camera::auto_order: the fast order where it is proven exact
        if info["exactness"] != 2:
            r.upload(scene)

    t = r.temporal(w, h)
    for k in range(3):
        cam = view(k, spp)
        upload(cam)
        linear, noise = _frame(r, cam, rt.RENDER_SEED + k, 0)     # camera::seed + frames accumulated so far
        g = r.guides(cam, 4, seed=rt.RENDER_SEED + k)
        out, out_se, rgb8, n = t.accumulate(cam, linear, g, noise, max_history=8)
        assert np.array_equal(_read_png(str(tmp_path / ("t%d.png" % k))), rgb8), k
    assert (n > 2).mean() > 0.5
    assert np.array_equal(_read_png(str(tmp_path / "d2.png")), r.denoise_guided(out, g, out_se)[1])
    t.close()
    cam = view(0, spp)
    upload(cam)
    one8 = r.render_host(cam)[1]
    assert np.array_equal(_read_png(str(tmp_path / "plain.png")), one8)                  # temporal_history = 0: the one-shot image
    assert not np.array_equal(_read_png(str(tmp_path / "t2.png")), r.render_host(view(2, spp))[1])
    assert np.array_equal(_read_png(str(tmp_path / "low.png")), r.render_host(view(0, 8))[1])   # too few samples: rendered without history
    r.close()
