"""ctypes binding of oracle/liboracle.so (the CPU restatement, rt_oracle.cpp).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py -- never by the package.  It is the checker, not a
rendering path of the product.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_DIR, "liboracle.so")
REF_DRIVER = os.path.join(_DIR, "_ref", "ref_driver")
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (make -C oracle)")
        l = C.CDLL(LIB_PATH)
        l.orc_render.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.orc_rng_stream.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        l.orc_kat_aabb.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double]
        l.orc_kat_node_hit.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        l.orc_kat_scatter.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_kat_texture.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        l.orc_kat_get_ray.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.orc_ray_hit.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_ray_color.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        l.orc_ray_hits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_ray_hits.restype = None
        l.orc_ray_colors.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        l.orc_ray_colors.restype = None
        _lib = l
    return _lib


def render(desc_ptr: int, cam, seed: int = 1, threads: int = 0):
    """Oracle render of the whole image: (linear f64 HxWx3, rgb8 HxWx3, counters dict)."""
    h, w = cam.image_height, cam.image_width
    linear = np.zeros((h, w, 3), np.float64)
    rgb8 = np.zeros((h, w, 3), np.uint8)
    cnt = (C.c_uint64 * 12)()
    rc = lib().orc_render(desc_ptr, C.addressof(cam), seed, threads, linear.ctypes.data, rgb8.ctypes.data, C.addressof(cnt))
    if rc != 0:
        raise RuntimeError(f"orc_render failed ({rc})")
    names = ("samples", "segments", "box_tests", "sphere_tests", "quad_tests", "triangle_tests", "xform_enters", "medium_tests",
             "surface_hits", "noise_calls", "texel_fetches", "rng_draws")
    return linear, rgb8, {n: int(v) for n, v in zip(names, cnt)}


def rng_stream(seed: int, pixel: int, sample: int, n: int) -> np.ndarray:
    out = np.zeros(n, np.float64)
    lib().orc_rng_stream(seed, pixel, sample, n, out.ctypes.data)
    return out


# ---- a caller's rays: arrays of rtk_ray records (88 bytes each; the package's ray_dtype()) -----------------------------
HIT_FIELDS = [("t", "<f8"), ("p", "<f8", (3,)), ("normal", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"), ("hit", "<i4"), ("front_face", "<i4"), ("material", "<i4"),
              ("prim_kind", "<i4"), ("draws", "<i8")]


def _ray_records(rays) -> np.ndarray:
    rays = np.ascontiguousarray(rays)
    if rays.ndim != 1 or rays.dtype.itemsize != 88:
        raise ValueError("rays: a one-dimensional array of 88-byte rtk_ray records")
    return rays


def hits(desc_ptr: int, rays, seed: int = 1) -> np.ndarray:
    """world.hit(r, interval(tmin, tmax), rec) of every ray, its stream keyed (seed, pixel, sample) and advanced by skip: records
    with the fields of rtk_ray_hit but prim_index (the oracle does not know the tables' indices); all 0 and material -1 on a
    miss; u, v of a constant medium's hit are whatever the record held before (constant_medium.h:45-50)."""
    rays = _ray_records(rays)
    n = len(rays)
    rec, hit, kind, draws = np.zeros((n, 11)), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)
    lib().orc_ray_hits(desc_ptr, n, rays.ctypes.data, seed, rec.ctypes.data, hit.ctypes.data, kind.ctypes.data, draws.ctypes.data)
    out = np.zeros(n, np.dtype(HIT_FIELDS))
    out["t"], out["p"], out["normal"], out["u"], out["v"] = rec[:, 0], rec[:, 1:4], rec[:, 4:7], rec[:, 8], rec[:, 9]
    out["hit"], out["front_face"], out["material"], out["prim_kind"], out["draws"] = hit, rec[:, 7].astype(np.int32), rec[:, 10].astype(np.int32), kind, draws
    return out


def ray_color(desc_ptr: int, rays, *, max_depth: int, background=(0.0, 0.0, 0.0), samples: int = 1, seed: int = 1):
    """(radiance [n][3], draws [n]) of ray_color for every ray: sample s = 0 .. samples-1 draws from (seed, pixel, sample + s)
    advanced by skip; the samples are summed in sample order and divided once; draws are summed, skip not counted."""
    rays = _ray_records(rays)
    n = len(rays)
    bg = np.array([float(background.x), float(background.y), float(background.z)] if hasattr(background, "x") else background, np.float64)
    total, total_draws = None, np.zeros(n, np.uint64)
    for s in range(max(1, samples)):
        rgb, draws = np.zeros((n, 3)), np.zeros(n, np.uint64)
        lib().orc_ray_colors(desc_ptr, n, rays.ctypes.data, bg.ctypes.data, max_depth, seed, s, rgb.ctypes.data, draws.ctypes.data)
        total = rgb if total is None else total + rgb
        total_draws += draws
    return (total / float(samples) if samples > 1 else total), total_draws
