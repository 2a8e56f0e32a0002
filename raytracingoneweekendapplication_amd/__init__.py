"""MI355X-native path tracer: Python plumbing over the C ABI of include/rtk.h.

The product is ``librtk_hip.so`` (hand-written HIP for gfx950, csrc/) driven through
the C ABI; this module only loads it with ctypes, mirrors the ABI structs and wraps
handles in small classes so that tests and ``bench.py`` can pass torch device
pointers and streams.  Scenes come from ``librtk_host.so`` -- the reference's scene
API re-implemented in C++ (host/), which flattens a ``hittable`` graph into the
``rtk_scene_desc`` the ABI takes.

There is no CPU rendering path here.  If ``librtk_hip.so`` is missing or no gfx950
device is usable, ``Renderer`` raises; nothing falls back to the oracle.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys
from typing import Optional

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_PKG_DIR)
DEFAULT_HIP_LIB_PATH = os.path.join(_PKG_DIR, "librtk_hip.so")
# RTK_HIP_LIB substitutes a diagnostic build (tools/: A/B libraries, the -DRTK_PROFILE build) and is honoured only together
# with RTK_DEV_TOOLS=1: a stray RTK_HIP_LIB in the environment of a test or bench run is an error, never a silent swap.
if os.environ.get("RTK_HIP_LIB") and os.environ.get("RTK_DEV_TOOLS") != "1":
    raise ImportError("RTK_HIP_LIB is set without RTK_DEV_TOOLS=1: refusing to load a substitute kernel library "
                      f"({os.environ['RTK_HIP_LIB']}) in place of {DEFAULT_HIP_LIB_PATH}")
HIP_LIB_PATH = os.environ.get("RTK_HIP_LIB") or DEFAULT_HIP_LIB_PATH
HOST_LIB_PATH = os.path.join(_PKG_DIR, "librtk_host.so")

RTK_ABI_VERSION = 2
RTK_REAL_F64 = 0
RTK_REAL_F32 = 1
TILE_PIXELS = 64

SCENE_SEED = 0x5EED2025  # construction RNG seed of the BASELINE scenes
RENDER_SEED = 1

# BASELINE.json configs -> scene_library.h names
CONFIG_SCENES = {
    "c1": "three_spheres",
    "c2": "book1_final",
    "c3": "cornell_box",
    "c4": "mesh",
    "c5": "book2_final",
}


class RtkError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"rtk error {code}: {message}")
        self.code = code


# ----------------------------------------------------------------------------- ABI structs
class Vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class Camera(C.Structure):
    """rtk_camera (include/rtk.h): the values camera::initialize() derives."""

    _fields_ = [
        ("image_width", C.c_int32), ("image_height", C.c_int32),
        ("samples_per_pixel", C.c_int32), ("max_depth", C.c_int32),
        ("background", Vec3), ("center", Vec3), ("pixel00_loc", Vec3),
        ("pixel_delta_u", Vec3), ("pixel_delta_v", Vec3),
        ("defocus_disk_u", Vec3), ("defocus_disk_v", Vec3),
        ("defocus_angle", C.c_double), ("pixel_samples_scale", C.c_double),
    ]


class RenderOpts(C.Structure):
    _fields_ = [
        ("seed", C.c_uint32), ("real_mode", C.c_int32), ("rank", C.c_int32), ("n_ranks", C.c_int32),
        ("count_work", C.c_int32), ("variant", C.c_int32), ("stream", C.c_void_p),
    ]


def _whole_image_opts(seed: int, real_mode: int, stream: int = 0) -> RenderOpts:
    """rtk_render_opts of a pass over the whole image: rank 0 of 1, no work counters, variant 0."""
    return RenderOpts(seed, real_mode, 0, 1, 0, 0, stream or None)


class OptimizeOpts(C.Structure):
    """rtk_optimize_opts (include/rtk.h)."""

    _fields_ = [("has_eye", C.c_int32), ("max_leaf", C.c_int32), ("eye", Vec3), ("prim_cost_scale", C.c_double),
                ("free_media_order", C.c_int32), ("_pad", C.c_int32)]


class OptimizeInfo(C.Structure):
    _fields_ = [("exact", C.c_int32), ("has_media", C.c_int32), ("has_triangles", C.c_int32),
                ("n_bvh_nodes_in", C.c_int32), ("n_bvh_nodes_out", C.c_int32), ("n_ordered_items", C.c_int32),
                ("expected_cost", C.c_double), ("box_margin", C.c_double)]


def _optimize_opts(eye, max_leaf, prim_cost_scale, free_media_order) -> OptimizeOpts:
    return OptimizeOpts(1 if eye is not None else 0, max_leaf, eye if eye is not None else Vec3(0, 0, 0), prim_cost_scale, 1 if free_media_order else 0, 0)


def _optimize_info(info: OptimizeInfo) -> dict:
    # exact: rtk_optimize_info.exact != 0 (bit-identical to the reference order); proven: == 2 (no triangles -- with them it is
    # identical in every measurement but not provable, include/rtk.h)
    return {"exact": bool(info.exact), "proven": info.exact == 2, "exactness": int(info.exact),
            "has_media": bool(info.has_media), "has_triangles": bool(info.has_triangles),
            "n_bvh_nodes_in": info.n_bvh_nodes_in, "n_bvh_nodes_out": info.n_bvh_nodes_out, "n_ordered_items": info.n_ordered_items,
            "expected_cost": info.expected_cost, "box_margin": info.box_margin}


PROGRESS_FN = C.CFUNCTYPE(None, C.c_int64, C.c_int64, C.c_void_p)  # rtk_progress_fn
GATHER_AUTO, GATHER_PEER, GATHER_RCCL = 0, 1, 2                     # rtk_gather_mode

COUNTER_FIELDS = (
    "samples", "segments", "box_tests", "sphere_tests", "quad_tests", "triangle_tests",
    "xform_enters", "medium_tests", "surface_hits", "noise_calls", "texel_fetches", "rng_draws",
)


class WorkCounters(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in COUNTER_FIELDS]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in COUNTER_FIELDS}


def algorithmic_bytes_per_sample(counters: dict, spp: int, real_mode: int, f32_boxes: bool = False) -> float:
    """SURVEY.md 8(d) byte model: bytes the sample loop must touch per sample.

    fp32 record sizes: BVH node 32, sphere 32, quad 68, triangle 76, instance
    transform 24, medium 12, material 32, perlin::noise 120, texel 4, framebuffer
    12 B/pixel.  In f64 mode the real-valued fields double (the 4-byte indices and
    the u8 texel do not).  ``f32_boxes``: the launched kernel reads the MIXED program's
    32-byte f32 culling-box records (F_F32_BOX) whatever the arithmetic type of the primitives.
    """
    n = max(1, counters["samples"])
    f64 = real_mode == RTK_REAL_F64
    node = 56 if (f64 and not f32_boxes) else 32        # 6 reals + 2 u32
    sphere = 60 if f64 else 32      # 7 reals + material
    quad = 132 if f64 else 68       # 16 reals + material
    tri = 124 if f64 else 76        # 12 reals + 6 float uv + material
    xform = 44 if f64 else 24       # 5 reals + child
    medium = 16 if f64 else 12
    material = 48 if f64 else 32
    noise = 216 if f64 else 120     # 8 gradients of 3 reals + 6 perm ints
    fb = 24 if f64 else 12
    total = (node * counters["box_tests"] + sphere * counters["sphere_tests"] + quad * counters["quad_tests"]
             + tri * counters["triangle_tests"] + xform * counters["xform_enters"] + medium * counters["medium_tests"]
             + material * counters["surface_hits"] + noise * counters["noise_calls"] + 4 * counters["texel_fetches"])
    return total / n + fb / max(1, spp)


class NoiseStats(C.Structure):
    """rtk_noise_stats: frame noise statistics of a progressive session (batch means over sample chunks)."""

    _fields_ = [("samples_done", C.c_int64), ("full_chunks", C.c_int32), ("valid", C.c_int32),
                ("mean_se", C.c_double), ("max_se", C.c_double), ("mean_rel_se", C.c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class CheckpointInfo(C.Structure):
    """rtk_checkpoint_info: the header of a progressive session's checkpoint."""

    _fields_ = [(name, C.c_int32) for name in ("version", "width", "height", "rank", "n_ranks", "real_mode", "target_spp", "chunk_size",
                                                 "samples_done")] + [("seed", C.c_uint32), ("scene_digest", C.c_uint64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class AdaptiveOpts(C.Structure):
    """rtk_adaptive_opts: the retire rule of a tile-adaptive progressive session."""

    _fields_ = [("rel_target", C.c_double), ("min_samples", C.c_int32), ("reserved", C.c_int32)]


class AdaptiveState(C.Structure):
    """rtk_adaptive_state: active / retired tiles and the samples rendered so far of one rank."""

    _fields_ = [("active_tiles", C.c_int32), ("retired_tiles", C.c_int32), ("pixel_samples", C.c_int64), ("mean_spp", C.c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


# ----------------------------------------------------------------------------- libraries
_host_lib = None
_hip_lib = None


class DenoiseOpts(C.Structure):
    """rtk_denoise_opts (include/rtk.h): a field left 0 takes its default (iterations 5, sigma_l 4, sigma_n 128, sigma_z 1,
    sigma_a 0.1)."""

    _fields_ = [("iterations", C.c_int32), ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float),
                ("sigma_a", C.c_float), ("reserved", C.c_int32)]


def _denoise_opts(iterations: int = 0, sigma_l: float = 0.0, sigma_n: float = 0.0, sigma_z: float = 0.0, sigma_a: float = 0.0) -> DenoiseOpts:
    return DenoiseOpts(int(iterations), float(sigma_l), float(sigma_n), float(sigma_z), float(sigma_a), 0)


class GuideOpts(C.Structure):
    """rtk_guide_opts (include/rtk.h): follow = GUIDE_FOLLOW_* bits (0 = mirrors), max_bounces 1..8 (0 = 4)."""

    _fields_ = [("follow", C.c_int32), ("max_bounces", C.c_int32)]


GUIDE_FOLLOW_MIRROR = 1
GUIDE_FOLLOW_DIELECTRIC = 2
DENOISE_DEMODULATE = 1
TEMPORAL_CHECK_ALBEDO = 1
UPSAMPLE_DEMODULATE = 1


class TemporalOpts(C.Structure):
    """rtk_temporal_opts (include/rtk.h): a field left 0 takes its default (max_history 32, depth_tol 0.02, normal_cos 0.9,
    albedo_tol 0.25); flags = TEMPORAL_CHECK_ALBEDO or 0."""

    _fields_ = [("max_history", C.c_int32), ("depth_tol", C.c_float), ("normal_cos", C.c_float), ("albedo_tol", C.c_float),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


def _temporal_opts(max_history: int = 0, depth_tol: float = 0.0, normal_cos: float = 0.0, albedo_tol: float = 0.0, check_albedo: bool = False) -> TemporalOpts:
    return TemporalOpts(int(max_history), float(depth_tol), float(normal_cos), float(albedo_tol), TEMPORAL_CHECK_ALBEDO if check_albedo else 0, 0)


class UpsampleOpts(C.Structure):
    """rtk_upsample_opts (include/rtk.h): a field left 0 takes its default (factor 2, sigma_n 128, sigma_z 1, sigma_a 0.1);
    flags = UPSAMPLE_DEMODULATE or 0."""

    _fields_ = [("factor", C.c_int32), ("sigma_n", C.c_float), ("sigma_z", C.c_float), ("sigma_a", C.c_float), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


def _upsample_opts(factor: int = 2, demodulate: bool = False, sigma_n: float = 0.0, sigma_z: float = 0.0, sigma_a: float = 0.0) -> UpsampleOpts:
    return UpsampleOpts(int(factor), float(sigma_n), float(sigma_z), float(sigma_a), UPSAMPLE_DEMODULATE if demodulate else 0, 0)


DISPLAY_CLAMP, DISPLAY_REINHARD, DISPLAY_ACES = 0, 1, 2
DISPLAY_GAMMA2, DISPLAY_SRGB = 0, 1
DISPLAY_BINS = 320


class TileSelectOpts(C.Structure):
    """rtk_tile_select_opts (include/rtk.h, "Tile lists"): a pixel is raw-flagged when !(below_map >= below) or !(above_map <= above);
    a tile is flagged when a raw-flagged pixel lies within ``dilate`` (0..8, Chebyshev) of one of its pixels."""
    _fields_ = [("below", C.c_float), ("above", C.c_float), ("dilate", C.c_int32), ("reserved", C.c_int32)]


def tile_flags_from_mask(mask):
    """Tile flags (int32, one per 8x8 tile, row-major over the tiles) of an (H, W) bool array: a tile is flagged when the mask is
    set at one of its pixels -- a region of interest for ``Renderer.render_tiles``."""
    import numpy as np

    m = np.asarray(mask, dtype=bool)
    if m.ndim != 2 or m.size == 0:
        raise ValueError(f"tile_flags_from_mask: an (H, W) array is needed, not shape {m.shape}")
    h, w = m.shape
    ty, tx = -(-h // 8), -(-w // 8)
    padded = np.zeros((ty * 8, tx * 8), bool)
    padded[:h, :w] = m
    return padded.reshape(ty, 8, tx, 8).any(axis=(1, 3)).reshape(-1).astype(np.int32)


class DisplayOpts(C.Structure):
    """rtk_display_opts (include/rtk.h): a field left 0 takes its default (exposure metered, key 0.18, meter_low 0.10, meter_high
    0.90, min_exposure 2^-10, max_exposure 2^10, adapt 1, curve CLAMP, white 4, encode GAMMA2, bloom off, bloom_threshold 1,
    bloom_levels 4)."""

    _fields_ = [("exposure", C.c_float), ("key", C.c_float), ("meter_low", C.c_float), ("meter_high", C.c_float), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("adapt", C.c_float), ("curve", C.c_int32), ("white", C.c_float), ("encode", C.c_int32), ("bloom", C.c_float),
                ("bloom_threshold", C.c_float), ("bloom_levels", C.c_int32), ("reserved", C.c_int32)]


def _display_opts(exposure: float = 0.0, key: float = 0.0, meter_low: float = 0.0, meter_high: float = 0.0, min_exposure: float = 0.0, max_exposure: float = 0.0,
                  adapt: float = 0.0, curve: int = DISPLAY_CLAMP, white: float = 0.0, encode: int = DISPLAY_GAMMA2, bloom: float = 0.0,
                  bloom_threshold: float = 0.0, bloom_levels: int = 0) -> DisplayOpts:
    return DisplayOpts(float(exposure), float(key), float(meter_low), float(meter_high), float(min_exposure), float(max_exposure), float(adapt), int(curve),
                       float(white), int(encode), float(bloom), float(bloom_threshold), int(bloom_levels), 0)


class Ray(C.Structure):
    """rtk_ray (include/rtk.h): a caller's ray and the keys of its random stream."""

    _fields_ = [("origin", C.c_double * 3), ("direction", C.c_double * 3), ("time", C.c_double), ("tmin", C.c_double), ("tmax", C.c_double),
                ("pixel", C.c_uint32), ("sample", C.c_uint32), ("skip", C.c_uint32), ("reserved", C.c_uint32)]


class RayHit(C.Structure):
    """rtk_ray_hit (include/rtk.h): the hit record of rtk_query_hits."""

    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("normal", C.c_double * 3), ("u", C.c_double), ("v", C.c_double),
                ("hit", C.c_int32), ("front_face", C.c_int32), ("material", C.c_int32), ("prim_kind", C.c_int32), ("prim_index", C.c_int32),
                ("draws", C.c_int32)]


class QueryOpts(C.Structure):
    """rtk_query_opts (include/rtk.h)."""

    _fields_ = [("seed", C.c_uint32), ("real_mode", C.c_int32), ("max_depth", C.c_int32), ("samples", C.c_int32), ("background", Vec3),
                ("stream", C.c_void_p), ("reserved", C.c_int32 * 2)]


# numpy structured dtypes with the layout of Ray and RayHit (field lists; numpy is imported where they are used)
RAY_FIELDS = [("origin", "<f8", (3,)), ("direction", "<f8", (3,)), ("time", "<f8"), ("tmin", "<f8"), ("tmax", "<f8"),
              ("pixel", "<u4"), ("sample", "<u4"), ("skip", "<u4"), ("reserved", "<u4")]
RAY_HIT_FIELDS = [("t", "<f8"), ("p", "<f8", (3,)), ("normal", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"),
                  ("hit", "<i4"), ("front_face", "<i4"), ("material", "<i4"), ("prim_kind", "<i4"), ("prim_index", "<i4"), ("draws", "<i4")]
NODE_SPHERE, NODE_QUAD, NODE_TRIANGLE, NODE_MEDIUM = 1, 2, 3, 8   # rtk_node_kind values of rtk_ray_hit.prim_kind


def ray_dtype():
    import numpy as np

    return np.dtype(RAY_FIELDS)


def ray_hit_dtype():
    import numpy as np

    return np.dtype(RAY_HIT_FIELDS)


def make_rays(origin, direction, *, time=0.0, tmin=0.001, tmax=float("inf"), pixel=0, sample=0, skip=0):
    """Ray records (``ray_dtype``) from arrays that broadcast to n rays: origin and direction (3,) or (n, 3), the rest scalars
    or (n,)."""
    import numpy as np

    origin, direction = np.atleast_2d(np.asarray(origin, np.float64)), np.atleast_2d(np.asarray(direction, np.float64))
    n = max([origin.shape[0], direction.shape[0]] + [np.size(v) for v in (time, tmin, tmax, pixel, sample, skip)])
    rays = np.zeros(n, ray_dtype())
    rays["origin"], rays["direction"] = origin, direction
    rays["time"], rays["tmin"], rays["tmax"] = time, tmin, tmax
    rays["pixel"], rays["sample"], rays["skip"] = pixel, sample, skip
    return rays


def _query_opts(seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, max_depth: int = 0, samples: int = 0, background=(0.0, 0.0, 0.0),
                stream: int = 0) -> QueryOpts:
    bg = background if isinstance(background, Vec3) else Vec3(*(float(c) for c in background))
    return QueryOpts(int(seed), int(real_mode), int(max_depth), int(samples), bg, stream or None, (C.c_int32 * 2)(0, 0))


class ProbeOpts(C.Structure):
    """rtk_probe_opts (include/rtk.h "Light probes")."""

    _fields_ = [("seed", C.c_uint32), ("real_mode", C.c_int32), ("max_depth", C.c_int32), ("samples", C.c_int32), ("rays", C.c_int32),
                ("first_key", C.c_uint32), ("background", Vec3), ("time", C.c_double), ("stream", C.c_void_p), ("reserved", C.c_int32 * 2)]


class ProbeGrid(C.Structure):
    """rtk_probe_grid (include/rtk.h): probe (ix, iy, iz) at origin + (ix, iy, iz) * spacing, index (iz * ny + iy) * nx + ix."""

    _fields_ = [("origin", Vec3), ("spacing", Vec3), ("counts", C.c_int32 * 3), ("reserved", C.c_int32)]


PROBE_COEFFS = 9


def _probe_opts(seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, max_depth: int = 0, samples: int = 0, rays: int = 0, first_key: int = 0,
                background=(0.0, 0.0, 0.0), time: float = 0.0, stream: int = 0) -> ProbeOpts:
    bg = background if isinstance(background, Vec3) else Vec3(*(float(c) for c in background))
    return ProbeOpts(int(seed), int(real_mode), int(max_depth), int(samples), int(rays), int(first_key) & 0xFFFFFFFF, bg, float(time), stream or None,
                     (C.c_int32 * 2)(0, 0))


def probe_grid(origin, spacing, counts) -> ProbeGrid:
    """A ``ProbeGrid`` from three (3,) sequences (a ``ProbeGrid`` is passed through)."""
    if isinstance(origin, ProbeGrid):
        return origin
    return ProbeGrid(Vec3(*(float(c) for c in origin)), Vec3(*(float(c) for c in spacing)), (C.c_int32 * 3)(*(int(c) for c in counts)), 0)


def probe_grid_positions(origin, spacing, counts):
    """The probe positions of a grid, float64 (nx * ny * nz, 3), in the grid's index order: x fastest, then y, then z."""
    import numpy as np

    origin, spacing = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    nx, ny, nz = (int(c) for c in counts)
    if origin.shape != (3,) or spacing.shape != (3,) or min(nx, ny, nz) < 1:
        raise ValueError(f"probe_grid_positions: origin {origin.shape}, spacing {spacing.shape}, counts {(nx, ny, nz)} do not describe a grid")
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return origin + np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1).astype(np.float64) * spacing


class GatherOpts(C.Structure):
    """rtk_gather_opts (include/rtk.h "Surface gathers")."""

    _fields_ = [("seed", C.c_uint32), ("real_mode", C.c_int32), ("max_depth", C.c_int32), ("samples", C.c_int32), ("rays", C.c_int32),
                ("first_key", C.c_uint32), ("rotate", C.c_int32), ("batch_points", C.c_int32), ("background", Vec3), ("time", C.c_double),
                ("max_distance", C.c_double), ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


def _gather_opts(seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, max_depth: int = 0, samples: int = 0, rays: int = 0, first_key: int = 0,
                 rotate: int = 0, batch_points: int = 0, background=(0.0, 0.0, 0.0), time: float = 0.0, max_distance: float = 0.0, stream: int = 0) -> GatherOpts:
    bg = background if isinstance(background, Vec3) else Vec3(*(float(c) for c in background))
    return GatherOpts(int(seed), int(real_mode), int(max_depth), int(samples), int(rays), int(first_key) & 0xFFFFFFFF, int(rotate), int(batch_points), bg,
                      float(time), float(max_distance), stream or None, (C.c_int32 * 4)(0, 0, 0, 0))


def quad_texels(Q, u, v, nu: int, nv: int):
    """The texel centres of a quad Q, u, v (quad.h) on an nu x nv grid and the quad's normal: (points, normals), float64
    (nu * nv, 3) each, texel (i, j) at index j * nu + i, point Q + ((i + .5) / nu) u + ((j + .5) / nv) v, every normal
    unit_vector(cross(u, v)) as the reference's quad computes it."""
    import numpy as np

    Q, u, v = (np.asarray(a, np.float64) for a in (Q, u, v))
    nu, nv = int(nu), int(nv)
    if Q.shape != (3,) or u.shape != (3,) or v.shape != (3,) or nu < 1 or nv < 1:
        raise ValueError(f"quad_texels: Q {Q.shape}, u {u.shape}, v {v.shape}, {nu} x {nv} texels do not describe a quad's grid")
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    n = (1.0 / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])) * n   # unit_vector: (1 / length) * v
    j, i = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    points = Q + ((i.ravel() + 0.5) / nu)[:, None] * u + ((j.ravel() + 0.5) / nv)[:, None] * v
    return points, np.tile(n, (nu * nv, 1))


LENS_PERSPECTIVE, LENS_EQUIRECT, LENS_FISHEYE, LENS_ORTHOGRAPHIC = 0, 1, 2, 3   # RTK_LENS_*


class Lens(C.Structure):
    """rtk_lens (include/rtk.h "Lens models"): a camera record, a projection and its frame and extents."""

    _fields_ = [("cam", Camera), ("model", C.c_int32), ("reserved", C.c_int32), ("u", Vec3), ("v", Vec3), ("w", Vec3),
                ("fov_h", C.c_double), ("fov_v", C.c_double), ("ortho_width", C.c_double), ("ortho_height", C.c_double)]


def derive_lens(model: int = LENS_PERSPECTIVE, image_width: int = 0, image_height: int = 0, *, cam: Optional[Camera] = None, spp: int = 1, max_depth: int = 10,
                lookfrom=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0), background=(0.0, 0.0, 0.0), fov_h: float = 0.0, fov_v: float = 0.0,
                ortho_width: float = 0.0, ortho_height: float = 0.0) -> Lens:
    """An rtk_lens.  LENS_PERSPECTIVE takes a whole camera: ``derive_lens(cam=...)`` (get_ray itself).  The other models take
    the image size, ``spp`` (pixel_samples_scale = 1 / spp), ``max_depth``, ``background``, the frame of ``lookfrom`` /
    ``lookat`` / ``vup`` (rtk_lens_look_at) and their extents: ``fov_h`` / ``fov_v`` in radians (0 = the model's default),
    ``ortho_width`` / ``ortho_height`` in world units."""
    lens = Lens()
    if cam is not None:
        if model != LENS_PERSPECTIVE:
            raise ValueError("derive_lens: cam= is the perspective lens; the other models take a size and a frame")
        C.memmove(C.byref(lens.cam), C.byref(cam), C.sizeof(Camera))
        return lens
    if model == LENS_PERSPECTIVE:
        raise ValueError("derive_lens: the perspective lens needs cam=")
    lens.cam.image_width, lens.cam.image_height = int(image_width), int(image_height)
    lens.cam.samples_per_pixel, lens.cam.max_depth = int(spp), int(max_depth)
    lens.cam.background = background if isinstance(background, Vec3) else Vec3(*(float(c) for c in background))
    lens.cam.pixel_samples_scale = 1.0 / spp if spp > 0 else 0.0
    lens.model = int(model)
    lens.fov_h, lens.fov_v, lens.ortho_width, lens.ortho_height = float(fov_h), float(fov_v), float(ortho_width), float(ortho_height)
    v3 = lambda v: v if isinstance(v, Vec3) else Vec3(*(float(c) for c in v))  # noqa: E731
    if hip_lib().rtk_lens_look_at(C.byref(lens), v3(lookfrom), v3(lookat), v3(vup)) != 0:
        raise ValueError("rtk_lens_look_at failed")
    return lens


def host_lib() -> C.CDLL:
    """librtk_host.so: scene construction + flattening (no GPU needed)."""
    global _host_lib
    if _host_lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"{HOST_LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(HOST_LIB_PATH)
        lib.rtkh_scene_build.restype = C.c_void_p
        lib.rtkh_scene_build.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
        lib.rtkh_scene_load.restype = C.c_void_p
        lib.rtkh_scene_load.argtypes = [C.c_char_p]
        lib.rtkh_scene_free.argtypes = [C.c_void_p]
        lib.rtkh_scene_desc.restype = C.c_void_p
        lib.rtkh_scene_desc.argtypes = [C.c_void_p]
        lib.rtkh_scene_save.argtypes = [C.c_void_p, C.c_char_p]
        lib.rtkh_scene_rng_draws.restype = C.c_uint64
        lib.rtkh_scene_rng_draws.argtypes = [C.c_void_p]
        lib.rtkh_scene_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Camera)]
        lib.rtkh_camera_derive.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(Camera)]
        lib.rtkh_image_texels.restype = C.c_int64
        lib.rtkh_image_texels.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int64]
        _host_lib = lib
    return _host_lib


def _one_hip_runtime() -> None:
    """One HIP runtime per process.  librtk_hip.so links /opt/rocm's libamdhip64; a PyTorch-ROCm wheel carries its own copy, and
    whichever runtime touches the devices FIRST owns them -- a process that rendered before it imported torch finds torch.cuda
    without devices ("No HIP GPUs are available").  With torch loaded first the library's HIP calls bind to torch's runtime (its
    libraries sit in the global symbol scope), which is also what makes torch streams and data_ptr()s valid arguments of the C
    ABI.  So where torch is installed it is imported before a HIP library of this package is loaded."""
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
        try:
            import torch  # noqa: F401
        except Exception:   # a broken torch install must not take the renderer down with it
            pass


def hip_lib() -> C.CDLL:
    """librtk_hip.so: the kernels + C ABI.  Raises if it was not built."""
    global _hip_lib
    if _hip_lib is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise RuntimeError(f"{HIP_LIB_PATH} not built: the HIP extension is required, there is no CPU path")
        _one_hip_runtime()
        lib = C.CDLL(HIP_LIB_PATH)
        lib.rtk_abi_version.restype = C.c_int
        lib.rtk_last_error.restype = C.c_char_p
        lib.rtk_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.rtk_destroy.argtypes = [C.c_void_p]
        lib.rtk_scene_upload.argtypes = [C.c_void_p, C.c_void_p]
        lib.rtk_tiles_per_rank.restype = C.c_int64
        lib.rtk_tiles_per_rank.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.rtk_render_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rtk_tiles_unpermute.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rtk_render_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rtk_scene_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.rtk_debug_closest_hit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        try:
            lib.rtk_frame_launches.argtypes = [C.POINTER(Camera), C.POINTER(RenderOpts)]
            lib.rtk_debug_scatter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_debug_texture.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_debug_get_ray.argtypes = [C.c_void_p, C.c_int, C.POINTER(Camera), C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_render_multi_enqueue.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_void_p]
            lib.rtk_multi_wait.argtypes = [C.c_void_p]
            lib.rtk_multi_frame_plan.argtypes = [C.c_int64, C.POINTER(C.c_int32)]
        except AttributeError:
            if HIP_LIB_PATH == DEFAULT_HIP_LIB_PATH:   # an A/B library of an older round (tools/, RTK_DEV_TOOLS=1) may lack the newer entry points
                raise
        lib.rtk_scene_optimize.argtypes = [C.c_void_p, C.POINTER(OptimizeOpts), C.POINTER(C.c_void_p), C.POINTER(OptimizeInfo)]
        lib.rtk_scene_upload_fast.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(OptimizeOpts), C.POINTER(OptimizeInfo)]
        lib.rtk_scene_optimized_free.restype = None
        lib.rtk_scene_optimized_free.argtypes = [C.c_void_p]
        lib.rtk_kernel_name.restype = C.c_char_p
        lib.rtk_kernel_name.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.rtk_render_views.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Camera), C.POINTER(C.c_uint32), C.POINTER(RenderOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rtk_render_views_host.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Camera), C.POINTER(C.c_uint32), C.POINTER(RenderOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rtk_view_kernel_name.restype = C.c_char_p
        lib.rtk_view_kernel_name.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.rtk_scene_upload_optimized.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(OptimizeOpts)]
        lib.rtk_init_multi.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        lib.rtk_multi_destroy.argtypes = [C.c_void_p]
        lib.rtk_multi_device_count.argtypes = [C.c_void_p]
        lib.rtk_multi_uses_rccl.argtypes = [C.c_void_p]
        lib.rtk_multi_ctx.restype = C.c_void_p
        lib.rtk_multi_ctx.argtypes = [C.c_void_p, C.c_int]
        lib.rtk_multi_scene_upload.argtypes = [C.c_void_p, C.c_void_p]
        lib.rtk_multi_scene_upload_fast.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(OptimizeOpts), C.POINTER(OptimizeInfo)]
        lib.rtk_render_multi_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_void_p]
        lib.rtk_render_multi.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_void_p]
        lib.rtk_set_progress_callback.argtypes = [C.c_void_p, PROGRESS_FN, C.c_void_p, C.c_int]
        try:
            lib.rtk_progressive_create.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(C.c_void_p)]
            lib.rtk_progressive_step.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_progressive_step_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_progressive_samples_done.argtypes = [C.c_void_p]
            lib.rtk_progressive_chunk_size.argtypes = [C.c_void_p]
            lib.rtk_progressive_noise.argtypes = [C.c_void_p, C.POINTER(NoiseStats)]
            lib.rtk_progressive_checkpoint_bytes.restype = C.c_int64
            lib.rtk_progressive_checkpoint_bytes.argtypes = [C.c_void_p]
            lib.rtk_progressive_save.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
            lib.rtk_progressive_resume.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
            lib.rtk_checkpoint_read_info.argtypes = [C.c_void_p, C.c_int64, C.POINTER(CheckpointInfo)]
            lib.rtk_progressive_destroy.argtypes = [C.c_void_p]
            lib.rtk_progressive_set_adaptive.argtypes = [C.c_void_p, C.POINTER(AdaptiveOpts)]
            lib.rtk_adaptive_status.argtypes = [C.c_void_p, C.POINTER(AdaptiveState)]
            lib.rtk_adaptive_tile_samples.argtypes = [C.c_void_p, C.c_void_p]
            lib.rtk_checkpoint_read_adaptive.argtypes = [C.c_void_p, C.c_int64, C.POINTER(AdaptiveOpts), C.c_void_p]
            lib.rtk_render_aovs.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_int32, C.c_void_p]
            lib.rtk_render_aovs_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_int32, C.c_void_p]
            lib.rtk_denoise.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenoiseOpts),
                                        C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_denoise_host.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenoiseOpts),
                                             C.c_void_p, C.c_void_p]
            lib.rtk_progressive_denoise.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DenoiseOpts), C.c_void_p, C.c_void_p]
            lib.rtk_progressive_denoise_host.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DenoiseOpts), C.c_void_p, C.c_void_p]
            lib.rtk_render_guides.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_int32, C.POINTER(GuideOpts), C.c_void_p]
            lib.rtk_render_guides_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_int32, C.POINTER(GuideOpts), C.c_void_p]
            lib.rtk_denoise_guided.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenoiseOpts),
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_denoise_guided_host.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(DenoiseOpts), C.c_int32, C.c_void_p, C.c_void_p]
            lib.rtk_progressive_denoise_guided.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GuideOpts), C.POINTER(DenoiseOpts), C.c_int32, C.c_void_p,
                                                           C.c_void_p]
            lib.rtk_progressive_denoise_guided_host.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GuideOpts), C.POINTER(DenoiseOpts), C.c_int32, C.c_void_p,
                                                                C.c_void_p]
            lib.rtk_temporal_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
            lib.rtk_temporal_accumulate.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalOpts), C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_temporal_accumulate_host.argtypes = lib.rtk_temporal_accumulate.argtypes
            lib.rtk_temporal_reset.argtypes = [C.c_void_p]
            lib.rtk_temporal_frames.argtypes = [C.c_void_p]
            lib.rtk_temporal_destroy.argtypes = [C.c_void_p]
            lib.rtk_temporal_reproject_matrix.argtypes = [C.POINTER(Camera), C.POINTER(C.c_double)]
            lib.rtk_upsample_camera.argtypes = [C.POINTER(Camera), C.c_int32, C.POINTER(Camera)]
            lib.rtk_upsample.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(UpsampleOpts),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_upsample_host.argtypes = lib.rtk_upsample.argtypes[:-1]
            lib.rtk_display_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
            lib.rtk_display_apply.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DisplayOpts), C.c_void_p, C.c_void_p]
            lib.rtk_display_apply_host.argtypes = lib.rtk_display_apply.argtypes
            lib.rtk_display_exposure.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
            lib.rtk_display_histogram.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
            lib.rtk_display_reset.argtypes = [C.c_void_p]
            lib.rtk_display_frames.argtypes = [C.c_void_p]
            lib.rtk_display_destroy.argtypes = [C.c_void_p]
            query = [C.c_void_p, C.POINTER(QueryOpts), C.c_int64, C.c_void_p, C.c_void_p]
            for name in ("rtk_query_hits", "rtk_query_occluded", "rtk_query_hits_host", "rtk_query_occluded_host"):
                getattr(lib, name).argtypes = query
            lib.rtk_query_radiance.argtypes = lib.rtk_query_radiance_host.argtypes = query + [C.c_void_p]
            for name in ("rtk_probe_rays", "rtk_probe_bake", "rtk_probe_rays_host", "rtk_probe_bake_host"):
                getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(ProbeOpts), C.c_int64, C.c_void_p, C.c_void_p]
            lib.rtk_probe_irradiance_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(ProbeGrid), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.rtk_probe_irradiance.argtypes = lib.rtk_probe_irradiance_host.argtypes + [C.c_void_p]
            gather = [C.c_void_p, C.POINTER(GatherOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            for name in ("rtk_gather_rays", "rtk_gather_irradiance", "rtk_gather_rays_host", "rtk_gather_irradiance_host"):
                getattr(lib, name).argtypes = gather
            lib.rtk_gather_occlusion.argtypes = lib.rtk_gather_occlusion_host.argtypes = gather + [C.c_void_p]
            lens = [C.c_void_p, C.POINTER(Lens), C.POINTER(RenderOpts)]
            lib.rtk_lens_look_at.argtypes = [C.POINTER(Lens), Vec3, Vec3, Vec3]
            lib.rtk_lens_rays.argtypes = lib.rtk_lens_rays_host.argtypes = lens + [C.c_int32, C.c_int32, C.c_void_p]
            lib.rtk_lens_render.argtypes = lib.rtk_lens_render_host.argtypes = lens + [C.c_int32, C.c_void_p, C.c_void_p]
            lib.rtk_lens_aovs.argtypes = lib.rtk_lens_aovs_host.argtypes = lens + [C.c_int32, C.c_void_p]
            lib.rtk_lens_guides.argtypes = lib.rtk_lens_guides_host.argtypes = lens + [C.c_int32, C.POINTER(GuideOpts), C.c_void_p]
            lib.rtk_tiles_select_host.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(TileSelectOpts), C.c_void_p]
            lib.rtk_tiles_select.argtypes = lib.rtk_tiles_select_host.argtypes + [C.c_void_p]
            lib.rtk_render_tiles.argtypes = lib.rtk_render_tiles_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_int32,
                                                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        except AttributeError:
            if HIP_LIB_PATH == DEFAULT_HIP_LIB_PATH:   # (an A/B library of an older round lacks the progressive entry points)
                raise
        if lib.rtk_abi_version() != RTK_ABI_VERSION and HIP_LIB_PATH == DEFAULT_HIP_LIB_PATH:
            raise RuntimeError("librtk_hip.so ABI version mismatch")
        _hip_lib = lib
    return _hip_lib


MICROBENCH_LIB_PATH = os.path.join(_PKG_DIR, "librtk_microbench.so")


def microbench(device: int = 0) -> dict:
    """Measured ceilings of the box (csrc/rtk_microbench.hip): HBM stream copy, LDS read rates, VALU issue rates per class.
    A measurement tool for bench.py's roofline object; raises when the library or a device is missing."""
    if not os.path.exists(MICROBENCH_LIB_PATH):
        raise RuntimeError(f"{MICROBENCH_LIB_PATH} not built (run __graft_entry__.build())")
    _one_hip_runtime()
    lib = C.CDLL(MICROBENCH_LIB_PATH)
    lib.rtk_microbench_names.restype = C.c_char_p
    lib.rtk_microbench_last_error.restype = C.c_char_p
    names = lib.rtk_microbench_names().decode().split(",")
    out = (C.c_double * len(names))()
    rc = lib.rtk_microbench_run(device, out, len(names))
    if rc != 0:
        raise RuntimeError(f"rtk_microbench_run failed ({rc}): {lib.rtk_microbench_last_error().decode()}")
    return dict(zip(names, [float(v) for v in out]))


def tiles_per_rank(width: int, height: int, n_ranks: int) -> int:
    """Same arithmetic as rtk_tiles_per_rank (usable without the HIP library)."""
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    return (tiles + n_ranks - 1) // n_ranks


# ----------------------------------------------------------------------------- scenes
class Scene:
    """A flattened scene (rtk_scene_desc) owned by librtk_host.so."""

    def __init__(self, handle: int, name: str):
        if not handle:
            raise ValueError(f"could not build/load scene {name!r}")
        self._h = handle
        self.name = name

    @classmethod
    def build(cls, name: str, scene_seed: int = SCENE_SEED, image_file: Optional[str] = None) -> "Scene":
        h = host_lib().rtkh_scene_build(name.encode(), scene_seed, (image_file or "").encode())
        return cls(h, name)

    @classmethod
    def load(cls, path: str) -> "Scene":
        return cls(host_lib().rtkh_scene_load(path.encode()), os.path.basename(path))

    @property
    def desc_ptr(self) -> int:
        return host_lib().rtkh_scene_desc(self._h)

    def save(self, path: str) -> None:
        if host_lib().rtkh_scene_save(self._h, path.encode()) != 0:
            raise IOError(f"cannot write {path}")

    def camera(self, width: int = 0, height: int = 0, spp: int = 0, depth: int = 0) -> Camera:
        cam = Camera()
        rc = host_lib().rtkh_scene_camera(self._h, width, height, spp, depth, C.byref(cam))
        if rc != 0:
            raise ValueError(f"cannot derive a {width}x{height} camera for {self.name} (rc={rc})")
        return cam

    def fast_order(self, eye: Optional[Vec3] = None, max_leaf: int = 0, prim_cost_scale: float = 0.0, free_media_order: bool = False) -> "FastOrderScene":
        """The same primitives re-grouped by rtk_scene_optimize (host-only pass of librtk_hip.so)."""
        return FastOrderScene(self, eye, max_leaf, prim_cost_scale, free_media_order)

    def close(self) -> None:
        if self._h:
            host_lib().rtkh_scene_free(self._h)
            self._h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastOrderScene:
    """rtk_scene_optimize output: a description that borrows the tables of `base` (kept alive here).

    ``exact`` says whether rendering it gives bit-identical images to the reference order (always, unless media were
    re-grouped too: ``free_media_order``); ``proven`` whether that is a proof (scenes without triangles) or a
    measurement (``rtk_optimize_info.exact`` 2 vs 1).
    """

    def __init__(self, base: Scene, eye: Optional[Vec3] = None, max_leaf: int = 0, prim_cost_scale: float = 0.0, free_media_order: bool = False):
        self.base = base
        self.name = base.name + "+fast_order"
        self.opts = opts = _optimize_opts(eye, max_leaf, prim_cost_scale, free_media_order)
        out, info = C.c_void_p(), OptimizeInfo()
        rc = hip_lib().rtk_scene_optimize(base.desc_ptr, C.byref(opts), C.byref(out), C.byref(info))
        if rc != 0 or not out.value:
            raise RtkError(rc, "rtk_scene_optimize failed")
        self._h = out.value
        self.exact = bool(info.exact)
        self.proven = info.exact == 2
        self.info = _optimize_info(info)

    @property
    def desc_ptr(self) -> int:
        return self._h

    def camera(self, *args, **kwargs) -> Camera:
        return self.base.camera(*args, **kwargs)

    def close(self) -> None:
        if getattr(self, "_h", None):
            hip_lib().rtk_scene_optimized_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def derive_camera(image_width: int, aspect_ratio: float, *, spp: int = 10, max_depth: int = 10, vfov: float = 90.0, lookfrom=(0.0, 0.0, 0.0),
                  lookat=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0), defocus_angle: float = 0.0, focus_dist: float = 10.0) -> Camera:
    """camera::derive() of the drop-in camera (host/rtk_camera.h = camera::initialize, Camera.txt:136-175) for raw public fields."""
    cam = Camera()
    v3 = lambda v: (C.c_double * 3)(*v)  # noqa: E731
    rc = host_lib().rtkh_camera_derive(image_width, aspect_ratio, spp, max_depth, vfov, v3(lookfrom), v3(lookat), v3(vup), defocus_angle, focus_dist, C.byref(cam))
    if rc != 0:
        raise ValueError("rtkh_camera_derive failed")
    return cam


# The six faces of a cube capture, in this order, as (forward axis, up vector): the layout of cube maps in graphics APIs
# (+x, -x, +y, -y, +z, -z; the side faces hang from -y, the top and bottom faces from +z / -z).
CUBE_FACES = (((1.0, 0.0, 0.0), (0.0, -1.0, 0.0)), ((-1.0, 0.0, 0.0), (0.0, -1.0, 0.0)), ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
              ((0.0, -1.0, 0.0), (0.0, 0.0, -1.0)), ((0.0, 0.0, 1.0), (0.0, -1.0, 0.0)), ((0.0, 0.0, -1.0), (0.0, -1.0, 0.0)))


def cube_face_cameras(center, face_size: int, *, spp: int = 10, max_depth: int = 10, background=(0.0, 0.0, 0.0)):
    """Six square 90-degree cameras at `center` looking down CUBE_FACES' axes with their up vectors, each derive_camera's (so
    a batch of them is Renderer.render_views' cube capture); `background` is set on every face."""
    cams = []
    for axis, up in CUBE_FACES:
        cam = derive_camera(face_size, 1.0, spp=spp, max_depth=max_depth, vfov=90.0, lookfrom=tuple(center),
                            lookat=tuple(center[k] + axis[k] for k in range(3)), vup=up, defocus_angle=0.0, focus_dist=1.0)
        cam.background = Vec3(*background)
        cams.append(cam)
    return cams


def load_image_texels(path: str):
    """The RGB8 texels image_texture reads for an image file (PPM or baseline JPEG), as rtw_image holds them
    (stbi_loadf's gamma-2.2 mapping and float_to_byte applied).  Returns an (H, W, 3) uint8 array or None."""
    import numpy as np

    w, h = C.c_int(), C.c_int()
    n = host_lib().rtkh_image_texels(path.encode(), C.byref(w), C.byref(h), None, 0)
    if n < 0:
        return None
    out = np.zeros((h.value, w.value, 3), np.uint8)
    host_lib().rtkh_image_texels(path.encode(), C.byref(w), C.byref(h), out.ctypes.data, n)
    return out


def write_synthetic_earth(path: str, width: int = 1024, height: int = 512) -> str:
    """Procedural RGB8 texture standing in for earthmap.jpg (binary PPM)."""
    import numpy as np

    y, x = np.mgrid[0:height, 0:width]
    lon = x / width * 2 * np.pi
    lat = (y / height - 0.5) * np.pi
    land = np.sin(3 * lon) * np.cos(2 * lat) + 0.5 * np.sin(7 * lon + 1.3) * np.sin(5 * lat) + 0.25 * np.cos(13 * lon * np.cos(lat))
    r = np.where(land > 0.15, 60 + 120 * np.clip(land, 0, 1), 20)
    g = np.where(land > 0.15, 110 + 90 * np.clip(1 - land, 0, 1), 60 + 40 * np.cos(lat))
    b = np.where(land > 0.15, 40, 150 + 80 * np.cos(lat))
    img = np.stack([r, g, b], -1).clip(0, 255).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (width, height))
        f.write(img.tobytes())
    return path


# ----------------------------------------------------------------------------- renderer
class Renderer:
    """One rtk_ctx bound to a HIP device.  Raises RtkError when no gfx950 device is usable."""

    def __init__(self, device: int = 0):
        self._lib = hip_lib()
        ctx = C.c_void_p()
        self._check(self._lib.rtk_init(device, C.byref(ctx)))
        self._ctx = ctx
        self.device = device

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise RtkError(rc, self._lib.rtk_last_error().decode())

    def upload(self, scene) -> None:
        self._check(self._lib.rtk_scene_upload(self._ctx, scene.desc_ptr))

    def upload_fast(self, scene, eye: Optional[Vec3] = None, max_leaf: int = 0, prim_cost_scale: float = 0.0, free_media_order: bool = False) -> dict:
        """rtk_scene_upload_fast: optimise the visiting order and upload, with the fast-order kernels.
        Returns the rtk_optimize_info fields."""
        opts = _optimize_opts(eye, max_leaf, prim_cost_scale, free_media_order)
        info = OptimizeInfo()
        self._check(self._lib.rtk_scene_upload_fast(self._ctx, scene.desc_ptr, C.byref(opts), C.byref(info)))
        return _optimize_info(info)

    def upload_optimized(self, scene, eye: Optional[Vec3] = None, free_media_order: bool = False) -> None:
        """rtk_scene_upload_optimized: a description that already IS a re-grouped hierarchy (rtk_scene_optimize output, or a
        hand-built one whose primitive nodes carry reference ranks in rtk_node.c), with the fast-order kernels."""
        opts = _optimize_opts(eye, 0, 0.0, free_media_order)
        self._check(self._lib.rtk_scene_upload_optimized(self._ctx, scene.desc_ptr, C.byref(opts)))

    def scene_info(self) -> dict:
        n, b64, b32 = C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self._lib.rtk_scene_info(self._ctx, C.byref(n), C.byref(b64), C.byref(b32)))
        return {"program_ops": n.value, "bytes_f64": b64.value, "bytes_f32": b32.value}

    def kernel_name(self, real_mode: int = RTK_REAL_F64, variant: int = 0) -> str:
        return self._lib.rtk_kernel_name(self._ctx, real_mode, variant).decode()

    def render_device(self, cam: Camera, d_linear: int, d_rgb8: int = 0, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64,
                      rank: int = 0, n_ranks: int = 1, d_counters: int = 0, variant: int = 0, stream: int = 0) -> None:
        """Enqueue the render kernel; all pointers are raw device addresses, nothing synchronises."""
        opts = RenderOpts(seed, real_mode, rank, n_ranks, 1 if d_counters else 0, variant, stream or None)
        self._check(self._lib.rtk_render_device(self._ctx, C.byref(cam), C.byref(opts), d_linear or None, d_rgb8 or None, d_counters or None))

    def unpermute(self, width: int, height: int, n_ranks: int, real_mode: int, d_gathered: int, d_linear: int, d_rgb8: int = 0, stream: int = 0) -> None:
        self._check(self._lib.rtk_tiles_unpermute(self._ctx, width, height, n_ranks, real_mode, d_gathered, d_linear or None, d_rgb8 or None, stream or None))

    def render_host(self, cam: Camera, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, count: bool = False, variant: int = 0):
        """Render the whole image and return (linear float64 HxWx3, rgb8 HxWx3, counters dict | None)."""
        import numpy as np

        h, w = cam.image_height, cam.image_width
        linear = np.zeros((h, w, 3), np.float64)
        rgb8 = np.zeros((h, w, 3), np.uint8)
        counters = WorkCounters()
        opts = RenderOpts(seed, real_mode, 0, 1, 1 if count else 0, variant, None)
        self._check(self._lib.rtk_render_host(self._ctx, C.byref(cam), C.byref(opts), linear.ctypes.data, rgb8.ctypes.data,
                                              C.byref(counters) if count else None))
        return linear, rgb8, (counters.as_dict() if count else None)

    @staticmethod
    def _view_arrays(cams, seeds):
        cams = list(cams)
        c_cams = (Camera * max(len(cams), 1))(*cams)
        c_seeds = None
        if seeds is not None:
            seeds = [int(x) for x in seeds]
            if len(seeds) != len(cams):
                raise ValueError("render_views: one seed per camera")
            c_seeds = (C.c_uint32 * max(len(seeds), 1))(*seeds)
        return len(cams), c_cams, c_seeds

    def view_kernel_name(self, real_mode: int = RTK_REAL_F64, variant: int = 0) -> str:
        """rtk_view_kernel_name: what a view batch dispatches -- the view kernel, or the plain kernel where it runs view by view."""
        return self._lib.rtk_view_kernel_name(self._ctx, real_mode, variant).decode()

    def render_views_device(self, cams, d_linear: int, d_rgb8: int = 0, d_counters: int = 0, *, seeds=None, seed: int = RENDER_SEED,
                            real_mode: int = RTK_REAL_F64, variant: int = 0, stream: int = 0) -> None:
        """rtk_render_views: enqueue a batch of same-sized views into [N,H,W,3] device planes (raw addresses); nothing synchronises."""
        n, c_cams, c_seeds = self._view_arrays(cams, seeds)
        opts = RenderOpts(seed, real_mode, 0, 1, 1 if d_counters else 0, variant, stream or None)
        self._check(self._lib.rtk_render_views(self._ctx, n, c_cams, c_seeds, C.byref(opts), d_linear or None, d_rgb8 or None, d_counters or None))

    def render_views(self, cams, *, seeds=None, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, count: bool = False, variant: int = 0):
        """rtk_render_views_host: render the batch and return (linear float64 [N,H,W,3], rgb8 [N,H,W,3], counters dict | None);
        view v is render_host(cams[v], seed=seeds[v]) bit for bit."""
        import numpy as np

        n, c_cams, c_seeds = self._view_arrays(cams, seeds)
        h, w = (c_cams[0].image_height, c_cams[0].image_width) if n else (0, 0)
        linear = np.zeros((n, max(h, 0), max(w, 0), 3), np.float64)
        rgb8 = np.zeros((n, max(h, 0), max(w, 0), 3), np.uint8)
        counters = WorkCounters()
        opts = RenderOpts(seed, real_mode, 0, 1, 1 if count else 0, variant, None)
        self._check(self._lib.rtk_render_views_host(self._ctx, n, c_cams, c_seeds, C.byref(opts), linear.ctypes.data, rgb8.ctypes.data,
                                                    C.byref(counters) if count else None))
        return linear, rgb8, (counters.as_dict() if count else None)

    def closest_hit(self, rays, keys, real_mode: int = RTK_REAL_F64):
        """Known-answer helper: hittable::hit of the scene root for rays [n,9] (o, d, time, tmin, tmax) with RNG keys
        [n,3] (seed, pixel, sample).  Returns (records [n,12], draws [n])."""
        import numpy as np

        rays = np.ascontiguousarray(rays, np.float64)
        keys = np.ascontiguousarray(keys, np.uint32)
        n = rays.shape[0]
        out = np.zeros((n, 12), np.float64)
        draws = np.zeros(n, np.uint64)
        self._check(self._lib.rtk_debug_closest_hit(self._ctx, real_mode, n, rays.ctypes.data, keys.ctypes.data, out.ctypes.data, draws.ctypes.data))
        return out, draws

    def debug_scatter(self, materials, rays, records, keys, real_mode: int = RTK_REAL_F64):
        """rtk_debug_scatter: (out [n][14] = scattered, scattered ray o(3) d(3), attenuation(3), time, emitted(3); draws [n])."""
        import numpy as np

        materials = np.ascontiguousarray(materials, np.int32)
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        records = np.ascontiguousarray(records, np.float64).reshape(-1, 11)
        keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 3)
        n = materials.shape[0]
        out, draws = np.zeros((n, 14), np.float64), np.zeros(n, np.uint64)
        self._check(self._lib.rtk_debug_scatter(self._ctx, real_mode, n, materials.ctypes.data, rays.ctypes.data, records.ctypes.data, keys.ctypes.data,
                                                out.ctypes.data, draws.ctypes.data))
        return out, draws

    def debug_texture(self, textures, uvp, real_mode: int = RTK_REAL_F64):
        """rtk_debug_texture: (colour [n][3], work [n][2] = perlin::noise calls, texel fetches)."""
        import numpy as np

        textures = np.ascontiguousarray(textures, np.int32)
        uvp = np.ascontiguousarray(uvp, np.float64).reshape(-1, 5)
        n = textures.shape[0]
        out, work = np.zeros((n, 3), np.float64), np.zeros((n, 2), np.uint64)
        self._check(self._lib.rtk_debug_texture(self._ctx, real_mode, n, textures.ctypes.data, uvp.ctypes.data, out.ctypes.data, work.ctypes.data))
        return out, work

    def debug_get_ray(self, cam: Camera, seed: int, pixel_sample, real_mode: int = RTK_REAL_F64):
        """rtk_debug_get_ray: (ray [n][7] = origin, direction, time; draws [n]) for pixel_sample [n][3] = i, j, sample."""
        import numpy as np

        ijs = np.ascontiguousarray(pixel_sample, np.int32).reshape(-1, 3)
        n = ijs.shape[0]
        out, draws = np.zeros((n, 7), np.float64), np.zeros(n, np.uint64)
        self._check(self._lib.rtk_debug_get_ray(self._ctx, real_mode, C.byref(cam), seed, n, ijs.ctypes.data, out.ctypes.data, draws.ctypes.data))
        return out, draws

    def _query_rays(self, who: str, rays):
        import numpy as np

        rays = np.ascontiguousarray(rays, ray_dtype())
        if rays.ndim != 1:
            raise ValueError(f"{who}: rays must be a one-dimensional array of ray records, not {rays.shape}")
        return rays

    def query_hits(self, rays, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_query_hits_host: hittable::hit(r, interval(tmin, tmax), rec) of the scene root for ray records (``ray_dtype``,
        see ``make_rays`` / ``camera_rays``).  Returns hit records (``ray_hit_dtype``)."""
        import numpy as np

        rays = self._query_rays("query_hits", rays)
        hits = np.zeros(rays.shape[0], ray_hit_dtype())
        self._check(self._lib.rtk_query_hits_host(self._ctx, C.byref(_query_opts(seed, real_mode)), rays.shape[0], rays.ctypes.data, hits.ctypes.data))
        return hits

    def query_occluded(self, rays, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_query_occluded_host: int32 (n,), the ``hit`` flag ``query_hits`` returns for the same rays."""
        import numpy as np

        rays = self._query_rays("query_occluded", rays)
        occluded = np.zeros(rays.shape[0], np.int32)
        self._check(self._lib.rtk_query_occluded_host(self._ctx, C.byref(_query_opts(seed, real_mode)), rays.shape[0], rays.ctypes.data, occluded.ctypes.data))
        return occluded

    def query_radiance(self, rays, *, max_depth: int, background=(0.0, 0.0, 0.0), samples: int = 1, count: bool = False, seed: int = RENDER_SEED,
                       real_mode: int = RTK_REAL_F64):
        """rtk_query_radiance_host: ray_color of every ray, the mean over ``samples`` samples with stream keys (seed, pixel,
        sample + s).  Returns float64 (n, 3) -- F32 results widened -- or, with ``count``, (radiance, draws uint32 (n,))."""
        import numpy as np

        rays = self._query_rays("query_radiance", rays)
        out = np.zeros((rays.shape[0], 3), np.float64)
        draws = np.zeros(rays.shape[0], np.uint32) if count else None
        opts = _query_opts(seed, real_mode, max_depth, samples, background)
        self._check(self._lib.rtk_query_radiance_host(self._ctx, C.byref(opts), rays.shape[0], rays.ctypes.data, out.ctypes.data,
                                                      draws.ctypes.data if count else None))
        return (out, draws) if count else out

    def query_hits_device(self, n: int, d_rays: int, d_hits: int, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_query_hits with raw device pointers (n rtk_ray records in, n rtk_ray_hit records out); asynchronous on ``stream``."""
        self._check(self._lib.rtk_query_hits(self._ctx, C.byref(_query_opts(seed, real_mode, stream=stream)), int(n), d_rays or None, d_hits or None))

    def query_occluded_device(self, n: int, d_rays: int, d_occluded: int, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_query_occluded with raw device pointers (int32 [n] out); asynchronous on ``stream``."""
        self._check(self._lib.rtk_query_occluded(self._ctx, C.byref(_query_opts(seed, real_mode, stream=stream)), int(n), d_rays or None, d_occluded or None))

    def query_radiance_device(self, n: int, d_rays: int, d_radiance: int, d_draws: int = 0, *, max_depth: int, background=(0.0, 0.0, 0.0), samples: int = 1,
                              seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_query_radiance with raw device pointers ([n][3] reals of ``real_mode`` out, uint32 [n] draws when ``d_draws`` is
        given); asynchronous on ``stream``."""
        opts = _query_opts(seed, real_mode, max_depth, samples, background, stream)
        self._check(self._lib.rtk_query_radiance(self._ctx, C.byref(opts), int(n), d_rays or None, d_radiance or None, d_draws or None))

    def probe_rays(self, positions, *, rays: int = 1024, samples: int = 1, first_key: int = 0, time: float = 0.0):
        """rtk_probe_rays_host: the ray records (``ray_dtype``, (n * rays,), probe-major) that ``bake_probes`` traces for probes at
        ``positions`` (n, 3): the fixed direction set, stream keys pixel = first_key + k, sample = j * samples."""
        import numpy as np

        (positions,) = _host_inputs("probe_rays", "(n, 3) probe positions", (positions, np.float64, (np.shape(positions)[0] if np.ndim(positions) else 0, 3)))
        n = positions.shape[0]
        opts = _probe_opts(samples=samples, rays=rays, first_key=first_key, time=time)
        out = np.zeros(n * (opts.rays or 1024), ray_dtype())
        self._check(self._lib.rtk_probe_rays_host(self._ctx, C.byref(opts), n, positions.ctypes.data, out.ctypes.data))
        return out

    def bake_probes(self, positions, *, max_depth: int, rays: int = 1024, samples: int = 1, background=(0.0, 0.0, 0.0), first_key: int = 0, time: float = 0.0,
                    seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_probe_bake_host: SH coefficients of the radiance arriving at probes at ``positions`` (n, 3): float64 (n, 9, 3) --
        F32 results widened -- c[k][i] = (4 pi / rays) sum_j L_kj Y_i(d_j) over the rays ``probe_rays`` returns."""
        import numpy as np

        (positions,) = _host_inputs("bake_probes", "(n, 3) probe positions", (positions, np.float64, (np.shape(positions)[0] if np.ndim(positions) else 0, 3)))
        n = positions.shape[0]
        out = np.zeros((n, PROBE_COEFFS, 3), np.float64)
        opts = _probe_opts(seed, real_mode, max_depth, samples, rays, first_key, background, time)
        self._check(self._lib.rtk_probe_bake_host(self._ctx, C.byref(opts), n, positions.ctypes.data, out.ctypes.data))
        return out

    def probe_irradiance(self, grid, sh, points, normals, *, real_mode: int = RTK_REAL_F64):
        """rtk_probe_irradiance_host: irradiance float64 (m, 3) at ``points`` (m, 3) with ``normals`` (m, 3) from the coefficients
        ``sh`` (nx * ny * nz, 9, 3) of the probes of ``grid`` (a ``ProbeGrid`` or (origin, spacing, counts))."""
        import numpy as np

        grid = grid if isinstance(grid, ProbeGrid) else probe_grid(*grid)
        probes = max(grid.counts[0], 0) * max(grid.counts[1], 0) * max(grid.counts[2], 0)
        m = np.shape(points)[0] if np.ndim(points) else 0
        sh, points, normals = _host_inputs("probe_irradiance", f"a grid of {probes} probes and m points with normals", (sh, np.float64, (probes, PROBE_COEFFS, 3)),
                                           (points, np.float64, (m, 3)), (normals, np.float64, (m, 3)))
        out = np.zeros((m, 3), np.float64)
        self._check(self._lib.rtk_probe_irradiance_host(self._ctx, real_mode, C.byref(grid), sh.ctypes.data, m, points.ctypes.data, normals.ctypes.data,
                                                        out.ctypes.data))
        return out

    def probe_rays_device(self, n: int, d_positions: int, d_rays: int, *, rays: int = 1024, samples: int = 1, first_key: int = 0, time: float = 0.0,
                          stream: int = 0) -> None:
        """rtk_probe_rays with raw device pointers ([n][3] doubles in, n * rays rtk_ray records out); asynchronous on ``stream``."""
        opts = _probe_opts(samples=samples, rays=rays, first_key=first_key, time=time, stream=stream)
        self._check(self._lib.rtk_probe_rays(self._ctx, C.byref(opts), int(n), d_positions or None, d_rays or None))

    def bake_probes_device(self, n: int, d_positions: int, d_sh: int, *, max_depth: int, rays: int = 1024, samples: int = 1, background=(0.0, 0.0, 0.0),
                           first_key: int = 0, time: float = 0.0, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_probe_bake with raw device pointers ([n][3] doubles in, [n][9][3] reals of ``real_mode`` out); asynchronous on ``stream``."""
        opts = _probe_opts(seed, real_mode, max_depth, samples, rays, first_key, background, time, stream)
        self._check(self._lib.rtk_probe_bake(self._ctx, C.byref(opts), int(n), d_positions or None, d_sh or None))

    def probe_irradiance_device(self, grid, d_sh: int, m: int, d_points: int, d_normals: int, d_irradiance: int, *, real_mode: int = RTK_REAL_F64,
                                stream: int = 0) -> None:
        """rtk_probe_irradiance with raw device pointers (reals of ``real_mode`` throughout); asynchronous on ``stream``."""
        grid = grid if isinstance(grid, ProbeGrid) else probe_grid(*grid)
        self._check(self._lib.rtk_probe_irradiance(self._ctx, real_mode, C.byref(grid), d_sh or None, int(m), d_points or None, d_normals or None,
                                                   d_irradiance or None, stream or None))

    def gather_rays(self, points, normals, *, rays: int = 256, samples: int = 1, first_key: int = 0, rotate: int = 0, time: float = 0.0,
                    max_distance: float = 0.0):
        """rtk_gather_rays_host: the ray records (``ray_dtype``, (n * rays,), point-major) that ``gather_irradiance`` and
        ``gather_occlusion`` trace for ``points`` (n, 3) with unit ``normals`` (n, 3): the cosine-weighted set around each normal,
        stream keys pixel = first_key + k, sample = j * samples, tmax = max_distance (0 = inf).  Needs no scene."""
        import numpy as np

        points, normals = _gather_inputs("gather_rays", points, normals)
        n = points.shape[0]
        opts = _gather_opts(samples=samples, rays=rays, first_key=first_key, rotate=rotate, time=time, max_distance=max_distance)
        out = np.zeros(n * (opts.rays or 256), ray_dtype())
        self._check(self._lib.rtk_gather_rays_host(self._ctx, C.byref(opts), n, points.ctypes.data, normals.ctypes.data, out.ctypes.data))
        return out

    def gather_irradiance(self, points, normals, *, max_depth: int, rays: int = 256, samples: int = 1, background=(0.0, 0.0, 0.0), first_key: int = 0,
                          rotate: int = 0, batch_points: int = 0, time: float = 0.0, max_distance: float = 0.0, seed: int = RENDER_SEED,
                          real_mode: int = RTK_REAL_F64):
        """rtk_gather_irradiance_host: E[k] = (pi / rays) sum_j L_kj over the rays ``gather_rays`` returns: float64 (n, 3), F32
        results widened.  ``max_distance`` is checked and changes nothing: the radiance query ignores a record's tmax."""
        import numpy as np

        points, normals = _gather_inputs("gather_irradiance", points, normals)
        n = points.shape[0]
        out = np.zeros((n, 3), np.float64)
        opts = _gather_opts(seed, real_mode, max_depth, samples, rays, first_key, rotate, batch_points, background, time, max_distance)
        self._check(self._lib.rtk_gather_irradiance_host(self._ctx, C.byref(opts), n, points.ctypes.data, normals.ctypes.data, out.ctypes.data))
        return out

    def gather_occlusion(self, points, normals, *, rays: int = 256, samples: int = 1, max_distance: float = 0.0, first_key: int = 0, rotate: int = 0,
                         batch_points: int = 0, time: float = 0.0, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_gather_occlusion_host: (open, bent): the open fraction of each point's rays, float64 (n,), and the mean of the open
        rays' directions over all rays (the bent normal, not normalised), float64 (n, 3); F32 results widened."""
        import numpy as np

        points, normals = _gather_inputs("gather_occlusion", points, normals)
        n = points.shape[0]
        open_, bent = np.zeros(n, np.float64), np.zeros((n, 3), np.float64)
        opts = _gather_opts(seed, real_mode, 0, samples, rays, first_key, rotate, batch_points, (0.0, 0.0, 0.0), time, max_distance)
        self._check(self._lib.rtk_gather_occlusion_host(self._ctx, C.byref(opts), n, points.ctypes.data, normals.ctypes.data, open_.ctypes.data,
                                                        bent.ctypes.data))
        return open_, bent

    def gather_rays_device(self, n: int, d_points: int, d_normals: int, d_rays: int, *, rays: int = 256, samples: int = 1, first_key: int = 0, rotate: int = 0,
                           time: float = 0.0, max_distance: float = 0.0, stream: int = 0) -> None:
        """rtk_gather_rays with raw device pointers ([n][3] doubles twice in, n * rays rtk_ray records out); asynchronous on ``stream``."""
        opts = _gather_opts(samples=samples, rays=rays, first_key=first_key, rotate=rotate, time=time, max_distance=max_distance, stream=stream)
        self._check(self._lib.rtk_gather_rays(self._ctx, C.byref(opts), int(n), d_points or None, d_normals or None, d_rays or None))

    def gather_irradiance_device(self, n: int, d_points: int, d_normals: int, d_irradiance: int, *, max_depth: int, rays: int = 256, samples: int = 1,
                                 background=(0.0, 0.0, 0.0), first_key: int = 0, rotate: int = 0, batch_points: int = 0, time: float = 0.0,
                                 max_distance: float = 0.0, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_gather_irradiance with raw device pointers ([n][3] reals of ``real_mode`` out); asynchronous on ``stream``.
        ``max_distance`` is checked and changes nothing."""
        opts = _gather_opts(seed, real_mode, max_depth, samples, rays, first_key, rotate, batch_points, background, time, max_distance, stream)
        self._check(self._lib.rtk_gather_irradiance(self._ctx, C.byref(opts), int(n), d_points or None, d_normals or None, d_irradiance or None))

    def gather_occlusion_device(self, n: int, d_points: int, d_normals: int, d_open: int, d_bent: int, *, rays: int = 256, samples: int = 1,
                                max_distance: float = 0.0, first_key: int = 0, rotate: int = 0, batch_points: int = 0, time: float = 0.0,
                                seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_gather_occlusion with raw device pointers ([n] and [n][3] reals of ``real_mode`` out, either may be 0); asynchronous
        on ``stream``."""
        opts = _gather_opts(seed, real_mode, 0, samples, rays, first_key, rotate, batch_points, (0.0, 0.0, 0.0), time, max_distance, stream)
        self._check(self._lib.rtk_gather_occlusion(self._ctx, C.byref(opts), int(n), d_points or None, d_normals or None, d_open or None, d_bent or None))

    def lens_rays(self, lens: Lens, samples: int = 1, *, first_sample: int = 0, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_lens_rays_host: the ray records (``ray_dtype``, (H * W * samples,), pixel-major, samples inner) of samples
        first_sample .. first_sample + samples - 1 of every pixel of ``lens``.  Needs no scene."""
        import numpy as np

        out = np.zeros(max(lens.cam.image_height, 0) * max(lens.cam.image_width, 0) * max(int(samples), 0), ray_dtype())
        opts = _whole_image_opts(seed, real_mode)
        self._check(self._lib.rtk_lens_rays_host(self._ctx, C.byref(lens), C.byref(opts), int(first_sample), int(samples), out.ctypes.data))
        return out

    def lens_render(self, lens: Lens, *, first_sample: int = 0, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_lens_render_host: (linear float64 (H, W, 3) -- F32 widened --, se float32 (H, W)) of lens.cam.samples_per_pixel
        samples per pixel from ``first_sample`` on: the sum in sample order times lens.cam.pixel_samples_scale."""
        import numpy as np

        h, w = lens.cam.image_height, lens.cam.image_width
        linear, noise = np.zeros((h, w, 3), np.float64), np.zeros((h, w), np.float32)
        opts = _whole_image_opts(seed, real_mode)
        self._check(self._lib.rtk_lens_render_host(self._ctx, C.byref(lens), C.byref(opts), int(first_sample), linear.ctypes.data, noise.ctypes.data))
        return linear, noise

    def lens_aovs(self, lens: Lens, samples: int = 4, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_lens_aovs_host: ``aovs`` through ``lens``, float32 (H, W, 8)."""
        import numpy as np

        out = np.zeros((lens.cam.image_height, lens.cam.image_width, 8), np.float32)
        opts = _whole_image_opts(seed, real_mode)
        self._check(self._lib.rtk_lens_aovs_host(self._ctx, C.byref(lens), C.byref(opts), int(samples), out.ctypes.data))
        return out

    def lens_guides(self, lens: Lens, samples: int = 4, *, follow: int = GUIDE_FOLLOW_MIRROR, max_bounces: int = 0, seed: int = RENDER_SEED,
                    real_mode: int = RTK_REAL_F64):
        """rtk_lens_guides_host: ``guides`` through ``lens``, float32 (H, W, 16)."""
        import numpy as np

        out = np.zeros((lens.cam.image_height, lens.cam.image_width, 16), np.float32)
        opts = _whole_image_opts(seed, real_mode)
        gopts = GuideOpts(int(follow), int(max_bounces))
        self._check(self._lib.rtk_lens_guides_host(self._ctx, C.byref(lens), C.byref(opts), int(samples), C.byref(gopts), out.ctypes.data))
        return out

    def lens_rays_device(self, lens: Lens, samples: int, d_rays: int, *, first_sample: int = 0, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64,
                         stream: int = 0) -> None:
        """rtk_lens_rays with a raw device pointer (H * W * samples rtk_ray records out); asynchronous on ``stream``."""
        opts = _whole_image_opts(seed, real_mode, stream)
        self._check(self._lib.rtk_lens_rays(self._ctx, C.byref(lens), C.byref(opts), int(first_sample), int(samples), d_rays or None))

    def lens_render_device(self, lens: Lens, d_linear: int, d_noise: int = 0, *, first_sample: int = 0, seed: int = RENDER_SEED,
                           real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_lens_render with raw device pointers ([H][W][3] reals of ``real_mode``, float [H][W] se when ``d_noise`` is given);
        asynchronous on ``stream``."""
        opts = _whole_image_opts(seed, real_mode, stream)
        self._check(self._lib.rtk_lens_render(self._ctx, C.byref(lens), C.byref(opts), int(first_sample), d_linear or None, d_noise or None))

    def lens_aovs_device(self, lens: Lens, samples: int, d_aov: int, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_lens_aovs with a raw device pointer (float [H][W][8], 16-byte aligned); asynchronous on ``stream``."""
        opts = _whole_image_opts(seed, real_mode, stream)
        self._check(self._lib.rtk_lens_aovs(self._ctx, C.byref(lens), C.byref(opts), int(samples), d_aov or None))

    def lens_guides_device(self, lens: Lens, samples: int, d_guides: int, *, follow: int = GUIDE_FOLLOW_MIRROR, max_bounces: int = 0,
                           seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_lens_guides with a raw device pointer (float [H][W][16], 16-byte aligned); asynchronous on ``stream``."""
        opts = _whole_image_opts(seed, real_mode, stream)
        gopts = GuideOpts(int(follow), int(max_bounces))
        self._check(self._lib.rtk_lens_guides(self._ctx, C.byref(lens), C.byref(opts), int(samples), C.byref(gopts), d_guides or None))

    def camera_rays(self, cam: Camera, seed: int, pixel_sample, real_mode: int = RTK_REAL_F64):
        """The render's own rays as ray records: ``debug_get_ray`` of ``pixel_sample`` [n][3] = i, j, sample, with the stream
        keys of that pixel and sample (pixel = j * W + i) and skip = the draws get_ray consumed, so that a query continues the
        stream where the render's ray generation left it.  tmin / tmax are ray_color's interval(0.001, inf)."""
        import numpy as np

        ijs = np.ascontiguousarray(pixel_sample, np.int32).reshape(-1, 3)
        ray, draws = self.debug_get_ray(cam, seed, ijs, real_mode)
        return make_rays(ray[:, 0:3], ray[:, 3:6], time=ray[:, 6], pixel=(ijs[:, 1] * cam.image_width + ijs[:, 0]).astype(np.uint32),
                         sample=ijs[:, 2].astype(np.uint32), skip=draws.astype(np.uint32))

    def aovs(self, cam: Camera, samples: int = 4, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64):
        """rtk_render_aovs_host: the denoiser's first-hit guide buffers, float32 (H, W, 8) = albedo(3), hit fraction, mean
        normal(3), depth over ``samples`` primary rays per pixel (the render's own rays for ``seed``)."""
        import numpy as np

        out = np.zeros((cam.image_height, cam.image_width, 8), np.float32)
        opts = _whole_image_opts(seed, real_mode)
        self._check(self._lib.rtk_render_aovs_host(self._ctx, C.byref(cam), C.byref(opts), int(samples), out.ctypes.data))
        return out

    def denoise(self, linear, aov, noise, *, real_mode: int = RTK_REAL_F64, iterations: int = 0, sigma_l: float = 0.0, sigma_n: float = 0.0,
                sigma_z: float = 0.0, sigma_a: float = 0.0):
        """rtk_denoise_host: the a-trous filter of ``linear`` (H, W, 3; rounded to float32 first when real_mode is F32) guided
        by ``aov`` (H, W, 8) and the per-pixel standard error ``noise`` (H, W).  Options left 0 take their defaults.
        Returns (linear float64 (H, W, 3), rgb8 (H, W, 3))."""
        import numpy as np

        h, w = np.shape(linear)[:2]
        linear, aov, noise = _host_inputs("denoise", "one (H, W) image", (linear, np.float64, (h, w, 3)), (aov, np.float32, (h, w, 8)), (noise, np.float32, (h, w)))
        out, rgb8 = np.zeros((h, w, 3)), np.zeros((h, w, 3), np.uint8)
        opts = _denoise_opts(iterations, sigma_l, sigma_n, sigma_z, sigma_a)
        self._check(self._lib.rtk_denoise_host(self._ctx, w, h, real_mode, linear.ctypes.data, aov.ctypes.data, noise.ctypes.data, C.byref(opts),
                                               out.ctypes.data, rgb8.ctypes.data))
        return out, rgb8

    def guides(self, cam: Camera, samples: int = 4, *, follow: int = GUIDE_FOLLOW_MIRROR, max_bounces: int = 0, seed: int = RENDER_SEED,
               real_mode: int = RTK_REAL_F64):
        """rtk_render_guides_host: the guide buffers that follow mirrors (``follow`` = GUIDE_FOLLOW_* bits, at most ``max_bounces``
        followed hits per sample, 0 = 4), float32 (H, W, 16): [..., :8] are ``aovs``' values; [..., 8:16] the seen albedo(3), end-hit
        fraction, end normal(3) and path length of the surface a mirror shows."""
        import numpy as np

        out = np.zeros((cam.image_height, cam.image_width, 16), np.float32)
        opts = _whole_image_opts(seed, real_mode)
        gopts = GuideOpts(int(follow), int(max_bounces))
        self._check(self._lib.rtk_render_guides_host(self._ctx, C.byref(cam), C.byref(opts), int(samples), C.byref(gopts), out.ctypes.data))
        return out

    def guides_device(self, cam: Camera, samples: int, d_guides: int, *, follow: int = GUIDE_FOLLOW_MIRROR, max_bounces: int = 0, seed: int = RENDER_SEED,
                      real_mode: int = RTK_REAL_F64, stream: int = 0) -> None:
        """rtk_render_guides with a raw device pointer (float [H][W][16], 16-byte aligned); asynchronous on ``stream``."""
        opts = _whole_image_opts(seed, real_mode, stream)
        gopts = GuideOpts(int(follow), int(max_bounces))
        self._check(self._lib.rtk_render_guides(self._ctx, C.byref(cam), C.byref(opts), int(samples), C.byref(gopts), d_guides or None))

    def denoise_guided(self, linear, guides, noise, *, demodulate: bool = False, real_mode: int = RTK_REAL_F64, iterations: int = 0,
                       sigma_l: float = 0.0, sigma_n: float = 0.0, sigma_z: float = 0.0, sigma_a: float = 0.0):
        """rtk_denoise_guided_host: ``denoise`` guided by ``guides`` (H, W, 16) -- normal and depth weights are the smaller of the
        first-hit and the seen surface's, the albedo weight is taken on the seen albedo.  ``demodulate`` filters colour / albedo
        instead (no albedo weight) and multiplies the albedo back.  Returns (linear float64 (H, W, 3), rgb8 (H, W, 3))."""
        import numpy as np

        h, w = np.shape(linear)[:2]
        linear, guides, noise = _host_inputs("denoise_guided", "one (H, W) image", (linear, np.float64, (h, w, 3)), (guides, np.float32, (h, w, 16)),
                                             (noise, np.float32, (h, w)))
        out, rgb8 = np.zeros((h, w, 3)), np.zeros((h, w, 3), np.uint8)
        opts = _denoise_opts(iterations, sigma_l, sigma_n, sigma_z, sigma_a)
        flags = DENOISE_DEMODULATE if demodulate else 0
        self._check(self._lib.rtk_denoise_guided_host(self._ctx, w, h, real_mode, linear.ctypes.data, guides.ctypes.data, noise.ctypes.data,
                                                      C.byref(opts), flags, out.ctypes.data, rgb8.ctypes.data))
        return out, rgb8

    def upsample(self, full_cam: Camera, low_linear, low_noise, low_guides, guides, *, factor: int = 2, demodulate: bool = False,
                 real_mode: int = RTK_REAL_F64, sigma_n: float = 0.0, sigma_z: float = 0.0, sigma_a: float = 0.0):
        """rtk_upsample_host: the frame of ``upsample_camera(full_cam, factor)`` -- ``low_linear`` (LH, LW, 3), its se ``low_noise``
        (LH, LW) and its guides ``low_guides`` (LH, LW, 16) -- rebuilt at ``full_cam``'s size, steered by ``guides`` (H, W, 16) of
        ``full_cam``.  ``demodulate`` interpolates colour / seen albedo and multiplies the full-resolution albedo back.  Returns
        (linear float64 (H, W, 3), se float32 (H, W), rgb8 (H, W, 3), support float32 (H, W))."""
        import numpy as np

        h, w = full_cam.image_height, full_cam.image_width
        f = int(factor) or 2
        lh, lw = -(-h // f), -(-w // f)
        low_linear, low_noise, low_guides, guides = _host_inputs(
            "upsample", f"a ({lh}, {lw}) image and the guides of a ({h}, {w}) one", (low_linear, np.float64, (lh, lw, 3)), (low_noise, np.float32, (lh, lw)),
            (low_guides, np.float32, (lh, lw, 16)), (guides, np.float32, (h, w, 16)))
        out, out_noise = np.zeros((h, w, 3)), np.zeros((h, w), np.float32)
        rgb8, support = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.float32)
        o = _upsample_opts(factor, demodulate, sigma_n, sigma_z, sigma_a)
        self._check(self._lib.rtk_upsample_host(self._ctx, C.byref(full_cam), real_mode, low_linear.ctypes.data, low_noise.ctypes.data, low_guides.ctypes.data,
                                                guides.ctypes.data, C.byref(o), out.ctypes.data, out_noise.ctypes.data, rgb8.ctypes.data, support.ctypes.data))
        return out, out_noise, rgb8, support

    def upsample_device(self, full_cam: Camera, d_low_linear: int, d_low_noise: int, d_low_guides: int, d_guides: int, d_out_linear: int = 0,
                        d_out_noise: int = 0, d_out_rgb8: int = 0, d_out_support: int = 0, *, real_mode: int = RTK_REAL_F64, stream: int = 0, **opts) -> None:
        """rtk_upsample with raw device pointers (any output may be 0, not all); asynchronous on ``stream``.  ``opts``: factor,
        demodulate, sigma_n, sigma_z, sigma_a."""
        o = _upsample_opts(**opts)
        self._check(self._lib.rtk_upsample(self._ctx, C.byref(full_cam), real_mode, d_low_linear or None, d_low_noise or None, d_low_guides or None,
                                           d_guides or None, C.byref(o), d_out_linear or None, d_out_noise or None, d_out_rgb8 or None, d_out_support or None,
                                           stream or None))

    def tiles_select(self, below_map=None, above_map=None, *, below: float = 0.0, above: float = 0.0, dilate: int = 0):
        """rtk_tiles_select_host: tile flags (int32, one per 8x8 tile, row-major) from (H, W) float32 maps: a pixel is raw-flagged
        when ``below_map`` is given and not >= ``below``, or ``above_map`` is given and not <= ``above`` (a NaN flags); a tile is
        flagged when a raw-flagged pixel lies within ``dilate`` pixels of it."""
        import numpy as np

        given = [m for m in (below_map, above_map) if m is not None]
        if not given:
            raise ValueError("tiles_select: below_map or above_map is needed")
        h, w = np.shape(given[0])
        maps = _host_inputs("tiles_select", f"({h}, {w}) maps", *[(m, np.float32, (h, w)) for m in given])
        b = maps[0] if below_map is not None else None
        a = maps[-1] if above_map is not None else None
        flags = np.zeros(tiles_per_rank(w, h, 1), np.int32)
        o = TileSelectOpts(float(below), float(above), int(dilate), 0)
        self._check(self._lib.rtk_tiles_select_host(self._ctx, w, h, None if b is None else b.ctypes.data, None if a is None else a.ctypes.data, C.byref(o),
                                                    flags.ctypes.data))
        return flags

    def tiles_select_device(self, width: int, height: int, d_below_map: int, d_above_map: int, d_tile_flags: int, *, below: float = 0.0, above: float = 0.0,
                            dilate: int = 0, stream: int = 0) -> None:
        """rtk_tiles_select with raw device pointers (either map may be 0, not both); asynchronous on ``stream``."""
        o = TileSelectOpts(float(below), float(above), int(dilate), 0)
        self._check(self._lib.rtk_tiles_select(self._ctx, int(width), int(height), d_below_map or None, d_above_map or None, C.byref(o), d_tile_flags or None,
                                               stream or None))

    def render_tiles(self, cam: Camera, tile_flags, *, linear=None, rgb8=None, noise=None, support=None, max_tiles: int = 0, seed: int = RENDER_SEED,
                     real_mode: int = RTK_REAL_F64, variant: int = 0):
        """rtk_render_tiles_host: render the tiles of ``cam``'s frame whose flag is non-zero with the render kernel.  ``linear``
        (H, W, 3) float64, ``rgb8`` (H, W, 3) uint8, ``noise`` and ``support`` (H, W) float32 are the initial contents (zeros when
        not given): pixels of unflagged tiles keep them, pixels of flagged tiles get ``render_host``'s values, a one-step
        session's standard error and support 1.  More than ``max_tiles`` (> 0) flagged tiles: nothing is rendered.  Returns
        (linear, rgb8, noise, support, {"flagged", "rendered"}); the arrays are new ones."""
        import numpy as np

        h, w = cam.image_height, cam.image_width
        init = [(linear, np.float64, (h, w, 3)), (rgb8, np.uint8, (h, w, 3)), (noise, np.float32, (h, w)), (support, np.float32, (h, w))]
        outs = [np.zeros(shape, dtype) if a is None else np.array(_host_inputs("render_tiles", f"a ({h}, {w}) image", (a, dtype, shape))[0])
                for a, dtype, shape in init]
        (flags,) = _host_inputs("render_tiles", f"the {tiles_per_rank(w, h, 1)} tile flags of a ({h}, {w}) image", (tile_flags, np.int32, (tiles_per_rank(w, h, 1),)))
        info = np.zeros(2, np.int32)
        opts = RenderOpts(seed, real_mode, 0, 1, 0, variant, None)
        self._check(self._lib.rtk_render_tiles_host(self._ctx, C.byref(cam), C.byref(opts), flags.ctypes.data, int(max_tiles), *[o.ctypes.data for o in outs],
                                                    info.ctypes.data))
        return (*outs, {"flagged": int(info[0]), "rendered": int(info[1])})

    def render_tiles_device(self, cam: Camera, d_tile_flags: int, d_linear: int = 0, d_rgb8: int = 0, d_noise: int = 0, d_support: int = 0, d_info: int = 0, *,
                            max_tiles: int = 0, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, variant: int = 0, stream: int = 0) -> None:
        """rtk_render_tiles with raw device pointers (any output may be 0, not all); every launch goes to ``stream``."""
        opts = RenderOpts(seed, real_mode, 0, 1, 0, variant, stream or None)
        self._check(self._lib.rtk_render_tiles(self._ctx, C.byref(cam), C.byref(opts), d_tile_flags or None, int(max_tiles), d_linear or None, d_rgb8 or None,
                                               d_noise or None, d_support or None, d_info or None))

    def upsample_refined(self, full_cam: Camera, low_linear, low_noise, low_guides, guides, *, refine_below: float, refine_dilate: int = 1, max_share: float = 0.0,
                         factor: int = 2, demodulate: bool = False, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, sigma_n: float = 0.0,
                         sigma_z: float = 0.0, sigma_a: float = 0.0):
        """``upsample``, then ``tiles_select`` on its support map (support not >= ``refine_below``, grown by ``refine_dilate``
        pixels), then ``render_tiles`` of ``full_cam`` into the upsample's four outputs: the tiles the interpolation had nothing
        to go on are the full-resolution frame's.  ``max_share`` > 0: with more than that share of the tiles flagged nothing is
        re-rendered.  Returns (linear, se, rgb8, support, info), info = {"flagged", "rendered", "tiles"}."""
        out, out_noise, rgb8, support = self.upsample(full_cam, low_linear, low_noise, low_guides, guides, factor=factor, demodulate=demodulate,
                                                      real_mode=real_mode, sigma_n=sigma_n, sigma_z=sigma_z, sigma_a=sigma_a)
        flags = self.tiles_select(support, below=refine_below, dilate=refine_dilate)
        max_tiles = max(1, int(max_share * flags.size)) if max_share > 0.0 else 0
        out, rgb8, out_noise, support, info = self.render_tiles(full_cam, flags, linear=out, rgb8=rgb8, noise=out_noise, support=support, max_tiles=max_tiles,
                                                                seed=seed, real_mode=real_mode)
        info["tiles"] = int(flags.size)
        return out, out_noise, rgb8, support, info

    def temporal(self, width: int, height: int, real_mode: int = RTK_REAL_F64, stream: int = 0) -> "Temporal":
        """rtk_temporal_create: an object that carries the frames of a moving camera along (``Temporal.accumulate``), bound to
        ``stream``."""
        h = C.c_void_p()
        self._check(self._lib.rtk_temporal_create(self._ctx, int(width), int(height), real_mode, stream or None, C.byref(h)))
        return Temporal(self, h, int(width), int(height), real_mode)

    def display(self, width: int, height: int, real_mode: int = RTK_REAL_F64, stream: int = 0) -> "Display":
        """rtk_display_create: an object that turns linear frames of ``width`` x ``height`` into display pixels (``Display.apply``:
        metered exposure, bloom, tone curve, encoding), bound to ``stream`` (0 = the null stream)."""
        h = C.c_void_p()
        self._check(self._lib.rtk_display_create(self._ctx, int(width), int(height), real_mode, stream or None, C.byref(h)))
        return Display(self, h, int(width), int(height), real_mode)

    def progressive(self, cam: Camera, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, rank: int = 0, n_ranks: int = 1,
                    stream: int = 0, rel_target: float | None = None, min_samples: int | None = None) -> "Progressive":
        """rtk_progressive_create: a session that renders the frame of ``cam`` (samples_per_pixel = the target) in steps.
        ``rel_target`` makes it tile-adaptive (rtk_progressive_set_adaptive): a tile retires once, after at least ``min_samples``
        samples (default: two chunks), the largest relative standard error of its pixels is <= rel_target."""
        opts = RenderOpts(seed, real_mode, rank, n_ranks, 0, 0, stream or None)
        h = C.c_void_p()
        self._check(self._lib.rtk_progressive_create(self._ctx, C.byref(cam), C.byref(opts), C.byref(h)))
        p = Progressive(self, h, cam, real_mode, n_ranks, rank)
        if rel_target is not None or min_samples is not None:
            if rel_target is None:
                p.close()
                raise ValueError("min_samples needs rel_target")
            ms = 2 * p.chunk_size if min_samples is None else int(min_samples)
            rc = self._lib.rtk_progressive_set_adaptive(p._h, C.byref(AdaptiveOpts(float(rel_target), ms, 0)))
            if rc != 0:
                err = RtkError(rc, self._lib.rtk_last_error().decode())
                p.close()
                raise err
        return p

    def resume(self, cam: Camera, blob: bytes, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, rank: int = 0, n_ranks: int = 1,
               stream: int = 0) -> "Progressive":
        """rtk_progressive_resume: continue a session from ``Progressive.save()``'s bytes (refused -- RtkError -- when they were
        made with another camera, seed, real mode, rank split, target or scene)."""
        opts = RenderOpts(seed, real_mode, rank, n_ranks, 0, 0, stream or None)
        buf = C.create_string_buffer(bytes(blob), len(blob))
        h = C.c_void_p()
        self._check(self._lib.rtk_progressive_resume(self._ctx, C.byref(cam), C.byref(opts), buf, len(blob), C.byref(h)))
        return Progressive(self, h, cam, real_mode, n_ranks, rank)

    def set_progress(self, fn=None, interval_ms: int = 100) -> None:
        """rtk_set_progress_callback: ``fn(done, total)`` is called from the thread that runs a blocking render
        (render_host), at most every ``interval_ms``; None switches it off."""
        self._progress = PROGRESS_FN(lambda done, total, _user: fn(done, total)) if fn else C.cast(None, PROGRESS_FN)
        self._check(self._lib.rtk_set_progress_callback(self._ctx, self._progress, None, interval_ms))

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.rtk_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_inputs(who: str, what: str, *inputs):
    """The array inputs of a ``*_host`` wrapper, (array, dtype, shape) each, as contiguous arrays of those dtypes; ValueError
    naming ``who``, the shapes found and ``what`` they should describe unless every one has its shape."""
    import numpy as np

    arrays = [np.ascontiguousarray(a, dtype) for a, dtype, _ in inputs]
    if any(a.shape != tuple(shape) for a, (_, _, shape) in zip(arrays, inputs)):
        one = len(arrays) == 1
        raise ValueError(f"{who}: shape{'' if one else 's'} {', '.join(str(a.shape) for a in arrays)} do{'es' if one else ''} not describe {what}")
    return arrays


def _gather_inputs(who: str, points, normals):
    """The points and normals of a ``gather_*`` wrapper as float64 (n, 3) arrays (``_host_inputs``)."""
    import numpy as np

    n = np.shape(points)[0] if np.ndim(points) else 0
    return _host_inputs(who, "(n, 3) points with (n, 3) normals", (points, np.float64, (n, 3)), (normals, np.float64, (n, 3)))


class _Handle:
    """What the wrappers of a C object created through a ``Renderer`` share: the handle, the renderer that keeps its context
    alive, the error check, and ``close`` through the C destroy function a subclass names in ``_destroy``."""

    _destroy = ""

    def __init__(self, renderer: Renderer, handle: C.c_void_p):
        self._r = renderer      # keeps the context alive
        self._lib = renderer._lib
        self._h = handle

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise RtkError(rc, self._lib.rtk_last_error().decode())

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ImageObject(_Handle):
    """A stateful image pass bound to one image size and arithmetic type (``Temporal``, ``Display``)."""

    def __init__(self, renderer: Renderer, handle: C.c_void_p, width: int, height: int, real_mode: int):
        super().__init__(renderer, handle)
        self.width, self.height, self.real_mode = width, height, real_mode


class Progressive(_Handle):
    """A progressive session (rtk_progressive): one frame rendered in steps of whole sample chunks, with a per-pixel noise
    estimate and checkpoints.  The finished frame is bit-identical to ``Renderer.render_host`` of the same camera."""

    _destroy = "rtk_progressive_destroy"

    def __init__(self, renderer: Renderer, handle: C.c_void_p, cam: Camera, real_mode: int, n_ranks: int, rank: int = 0):
        super().__init__(renderer, handle)
        self.width, self.height, self.target = cam.image_width, cam.image_height, cam.samples_per_pixel
        self.real_mode, self.n_ranks, self.rank = real_mode, n_ranks, rank

    @property
    def samples_done(self) -> int:
        return self._lib.rtk_progressive_samples_done(self._h)

    @property
    def chunk_size(self) -> int:
        return self._lib.rtk_progressive_chunk_size(self._h)

    def step(self, n: int, *, count: bool = False):
        """Add the next ``n`` samples of every pixel.  Returns (linear float64, rgb8, noise float32) -- (H, W, 3), (H, W, 3),
        (H, W) for one rank; the compact [tiles, 3, 64] buffer, None and [tiles, 64] for one of several -- plus the step's work
        counters when ``count``."""
        import numpy as np

        if self.n_ranks == 1:
            linear, rgb8, noise = np.zeros((self.height, self.width, 3)), np.zeros((self.height, self.width, 3), np.uint8), np.zeros((self.height, self.width), np.float32)
        else:
            t = tiles_per_rank(self.width, self.height, self.n_ranks)
            linear, rgb8, noise = np.zeros((t, 3, 64)), None, np.zeros((t, 64), np.float32)
        counters = WorkCounters()
        self._check(self._lib.rtk_progressive_step_host(self._h, n, linear.ctypes.data, rgb8.ctypes.data if rgb8 is not None else None,
                                                        noise.ctypes.data, C.byref(counters) if count else None))
        return (linear, rgb8, noise, counters.as_dict()) if count else (linear, rgb8, noise)

    def step_device(self, n: int, d_linear: int = 0, d_rgb8: int = 0, d_noise: int = 0, d_counters: int = 0) -> None:
        """rtk_progressive_step with raw device pointers (any may be 0); asynchronous on the session's stream."""
        self._check(self._lib.rtk_progressive_step(self._h, n, d_linear or None, d_rgb8 or None, d_noise or None, d_counters or None))

    def noise(self) -> dict:
        out = NoiseStats()
        self._check(self._lib.rtk_progressive_noise(self._h, C.byref(out)))
        return out.as_dict()

    def adaptive_status(self) -> dict:
        """rtk_adaptive_status: {active_tiles, retired_tiles, pixel_samples, mean_spp} of this rank (synchronises)."""
        out = AdaptiveState()
        self._check(self._lib.rtk_adaptive_status(self._h, C.byref(out)))
        return out.as_dict()

    def tile_samples(self):
        """rtk_adaptive_tile_samples: int32 [tiles_per_rank], each local tile's sample count (0 for a rank's padding tiles)."""
        import numpy as np

        out = np.zeros(tiles_per_rank(self.width, self.height, self.n_ranks), np.int32)
        self._check(self._lib.rtk_adaptive_tile_samples(self._h, out.ctypes.data))
        return out

    def sample_map(self):
        """(H, W) int32: every pixel's sample count -- its tile's -- for this rank's tiles; 0 for the other ranks' pixels."""
        import numpy as np

        spp = self.tile_samples()
        tx, ty = (self.width + 7) // 8, (self.height + 7) // 8
        grid = np.zeros(tx * ty, np.int32)
        tiles = np.arange(len(spp)) * self.n_ranks + self.rank
        keep = tiles < tx * ty
        grid[tiles[keep]] = spp[keep]
        return np.repeat(np.repeat(grid.reshape(ty, tx), 8, 0), 8, 1)[: self.height, : self.width].copy()

    def denoised(self, aov_samples: int = 4, **opts):
        """rtk_progressive_denoise_host: the current preview denoised with the session's own noise estimate (needs two full
        chunks; one rank).  ``opts``: iterations, sigma_l, sigma_n, sigma_z, sigma_a (0 = default).  The session is not
        changed.  Returns (linear float64 (H, W, 3), rgb8 (H, W, 3))."""
        import numpy as np

        out, rgb8 = np.zeros((self.height, self.width, 3)), np.zeros((self.height, self.width, 3), np.uint8)
        o = _denoise_opts(**opts)
        self._check(self._lib.rtk_progressive_denoise_host(self._h, int(aov_samples), C.byref(o), out.ctypes.data, rgb8.ctypes.data))
        return out, rgb8

    def denoised_guided(self, aov_samples: int = 4, *, follow: int = GUIDE_FOLLOW_MIRROR, max_bounces: int = 0, demodulate: bool = False, **opts):
        """rtk_progressive_denoise_guided_host: ``denoised`` with the guides of ``Renderer.guides`` (kept on the session per
        aov_samples, follow and max_bounces) and, with ``demodulate``, on colour / albedo.  The session is not changed."""
        import numpy as np

        out, rgb8 = np.zeros((self.height, self.width, 3)), np.zeros((self.height, self.width, 3), np.uint8)
        o = _denoise_opts(**opts)
        g = GuideOpts(int(follow), int(max_bounces))
        self._check(self._lib.rtk_progressive_denoise_guided_host(self._h, int(aov_samples), C.byref(g), C.byref(o), DENOISE_DEMODULATE if demodulate else 0,
                                                                  out.ctypes.data, rgb8.ctypes.data))
        return out, rgb8

    def save(self) -> bytes:
        n = self._lib.rtk_progressive_checkpoint_bytes(self._h)
        if n <= 0:
            self._check(int(n) or -1)
        buf = C.create_string_buffer(n)
        self._check(self._lib.rtk_progressive_save(self._h, buf, n))
        return buf.raw


class Temporal(_ImageObject):
    """Temporal accumulation (rtk_temporal): per frame, the history -- the frame returned last time -- is reprojected into the new
    camera, history of another surface is rejected, and colour, variance and history length are blended (include/rtk.h has the
    rule).  Feed ``accumulate`` a noisy frame with its se and the guides of the same camera; its outputs are inputs of
    ``Renderer.denoise_guided``."""

    _destroy = "rtk_temporal_destroy"

    @property
    def frames(self) -> int:
        """Frames accumulated since creation / ``reset``."""
        n = self._lib.rtk_temporal_frames(self._h)
        if n < 0:
            self._check(n)
        return n

    def accumulate(self, cam: Camera, linear, guides, noise, **opts):
        """rtk_temporal_accumulate_host: ``linear`` (H, W, 3), ``guides`` (H, W, 16) of ``cam``, ``noise`` (H, W) se.  ``opts``:
        max_history, depth_tol, normal_cos, albedo_tol (0 = default), check_albedo.  Returns (linear float64 (H, W, 3), noise
        float32 (H, W), rgb8 (H, W, 3), history float32 (H, W))."""
        import numpy as np

        h, w = self.height, self.width
        linear, guides, noise = _host_inputs("accumulate", f"one ({h}, {w}) image", (linear, np.float64, (h, w, 3)), (guides, np.float32, (h, w, 16)),
                                             (noise, np.float32, (h, w)))
        out, out_noise = np.zeros((h, w, 3)), np.zeros((h, w), np.float32)
        rgb8, history = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.float32)
        o = _temporal_opts(**opts)
        self._check(self._lib.rtk_temporal_accumulate_host(self._h, C.byref(cam), linear.ctypes.data, guides.ctypes.data, noise.ctypes.data, C.byref(o),
                                                           out.ctypes.data, out_noise.ctypes.data, rgb8.ctypes.data, history.ctypes.data))
        return out, out_noise, rgb8, history

    def accumulate_device(self, cam: Camera, d_linear: int, d_guides: int, d_noise: int, d_out_linear: int = 0, d_out_noise: int = 0, d_out_rgb8: int = 0,
                          d_out_history: int = 0, **opts) -> None:
        """rtk_temporal_accumulate with raw device pointers (any output may be 0); asynchronous on the object's stream."""
        o = _temporal_opts(**opts)
        self._check(self._lib.rtk_temporal_accumulate(self._h, C.byref(cam), d_linear or None, d_guides or None, d_noise or None, C.byref(o),
                                                      d_out_linear or None, d_out_noise or None, d_out_rgb8 or None, d_out_history or None))

    def reset(self) -> None:
        """The next frame starts a new history."""
        self._check(self._lib.rtk_temporal_reset(self._h))


class Display(_ImageObject):
    """The display transform (rtk_display): per frame the luminance is metered into a histogram, an exposure is adapted towards the
    trimmed log-average, bloom is added on request, and a tone curve and an encoding give the pixels (include/rtk.h has the rule).
    The exposure stays on the device between the passes; ``exposure()`` and ``histogram()`` fetch it and block."""

    _destroy = "rtk_display_destroy"

    def frames(self) -> int:
        """Frames applied since creation / ``reset``."""
        n = self._lib.rtk_display_frames(self._h)
        if n < 0:
            self._check(n)
        return n

    def apply(self, linear, **opts):
        """rtk_display_apply_host: ``linear`` (H, W, 3).  ``opts``: the fields of ``DisplayOpts`` but ``reserved`` (0 = default).
        Returns (out_linear float64 (H, W, 3), rgb8 (H, W, 3), exposure)."""
        import numpy as np

        h, w = self.height, self.width
        (linear,) = _host_inputs("apply", f"a ({h}, {w}) image", (linear, np.float64, (h, w, 3)))
        out, rgb8 = np.zeros((h, w, 3)), np.zeros((h, w, 3), np.uint8)
        o = _display_opts(**opts)
        self._check(self._lib.rtk_display_apply_host(self._h, linear.ctypes.data, C.byref(o), out.ctypes.data, rgb8.ctypes.data))
        return out, rgb8, self.exposure()[0]

    def apply_device(self, d_linear: int, d_out_linear: int = 0, d_out_rgb8: int = 0, **opts) -> None:
        """rtk_display_apply with raw device pointers (one output may be 0); asynchronous on the object's stream."""
        o = _display_opts(**opts)
        self._check(self._lib.rtk_display_apply(self._h, d_linear or None, C.byref(o), d_out_linear or None, d_out_rgb8 or None))

    def exposure(self):
        """(E, E_target) of the last apply; blocks."""
        out = (C.c_double * 2)()
        self._check(self._lib.rtk_display_exposure(self._h, out))
        return float(out[0]), float(out[1])

    def histogram(self):
        """The luminance histogram of the last metered apply: uint32 [320], 8 bins per octave from 2^-20; blocks."""
        import numpy as np

        out = (C.c_uint32 * DISPLAY_BINS)()
        self._check(self._lib.rtk_display_histogram(self._h, out))
        return np.array(out[:], np.uint32)

    def reset(self) -> None:
        """The next frame is a first frame: its exposure is its target."""
        self._check(self._lib.rtk_display_reset(self._h))


def temporal_reproject_matrix(cam: Camera):
    """rtk_temporal_reproject_matrix (host-only, no GPU): float64 [12] = the row-major inverse of [pixel_delta_u | pixel_delta_v |
    pixel00_loc - center], then center.  Raises RtkError for a singular camera."""
    import numpy as np

    lib = hip_lib()
    out = (C.c_double * 12)()
    rc = lib.rtk_temporal_reproject_matrix(C.byref(cam), out)
    if rc != 0:
        raise RtkError(rc, lib.rtk_last_error().decode())
    return np.array(out[:], np.float64)


def upsample_camera(cam: Camera, factor: int = 2) -> Camera:
    """rtk_upsample_camera (host-only, no GPU): the camera that renders ``cam``'s view at 1 / ``factor`` of the width and height
    (rounded up), each of its pixels covering ``factor`` x ``factor`` of ``cam``'s.  Raises RtkError for a factor outside 2..4."""
    lib = hip_lib()
    low = Camera()
    rc = lib.rtk_upsample_camera(C.byref(cam), int(factor), C.byref(low))
    if rc != 0:
        raise RtkError(rc, lib.rtk_last_error().decode())
    return low


def checkpoint_info(blob: bytes) -> dict:
    """rtk_checkpoint_read_info: the header of a checkpoint, checked (magic, version, size, checksum).  Host-only, no GPU.
    Raises RtkError for a blob the library would refuse."""
    lib = hip_lib()
    info = CheckpointInfo()
    buf = C.create_string_buffer(bytes(blob), max(1, len(blob)))
    rc = lib.rtk_checkpoint_read_info(buf, len(blob), C.byref(info))
    if rc != 0:
        raise RtkError(rc, lib.rtk_last_error().decode())
    out = info.as_dict()
    if info.version == 2:  # an adaptive session's: its options and the tiles' sample counts as well
        import numpy as np

        ad = AdaptiveOpts()
        spp = np.zeros(tiles_per_rank(info.width, info.height, info.n_ranks), np.int32)
        rc = lib.rtk_checkpoint_read_adaptive(buf, len(blob), C.byref(ad), spp.ctypes.data)
        if rc != 0:
            raise RtkError(rc, lib.rtk_last_error().decode())
        out.update(rel_target=ad.rel_target, min_samples=ad.min_samples, tile_spp=spp)
    return out


class MultiRenderer:
    """rtk_multi: several GPUs of one node behind one call (one host thread, replicated scene, interleaved tiles, one
    gather to the first device).  ``devices`` are HIP ordinals; an ordinal may repeat (ranks then share a GPU)."""

    def __init__(self, devices, gather: int = GATHER_AUTO):
        self._lib = hip_lib()
        devs = (C.c_int * len(devices))(*devices)
        handle = C.c_void_p()
        self._check(self._lib.rtk_init_multi(len(devices), devs, gather, C.byref(handle)))
        self._m = handle
        self.devices = list(devices)

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise RtkError(rc, self._lib.rtk_last_error().decode())

    @property
    def uses_rccl(self) -> bool:
        return bool(self._lib.rtk_multi_uses_rccl(self._m))

    def upload(self, scene) -> None:
        self._check(self._lib.rtk_multi_scene_upload(self._m, scene.desc_ptr))

    def upload_fast(self, scene, eye: Optional[Vec3] = None) -> dict:
        opts = _optimize_opts(eye, 0, 0.0, False)
        info = OptimizeInfo()
        self._check(self._lib.rtk_multi_scene_upload_fast(self._m, scene.desc_ptr, C.byref(opts), C.byref(info)))
        return _optimize_info(info)

    def kernel_name(self, real_mode: int = RTK_REAL_F64, variant: int = 0) -> str:
        return self._lib.rtk_kernel_name(self._lib.rtk_multi_ctx(self._m, 0), real_mode, variant).decode()

    def set_progress(self, fn=None, interval_ms: int = 100) -> None:
        self._progress = PROGRESS_FN(lambda done, total, _user: fn(done, total)) if fn else C.cast(None, PROGRESS_FN)
        self._check(self._lib.rtk_set_progress_callback(self._lib.rtk_multi_ctx(self._m, 0), self._progress, None, interval_ms))

    def render_host(self, cam: Camera, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, variant: int = 0):
        """rtk_render_multi: (linear float64 HxWx3, rgb8 HxWx3)."""
        import numpy as np

        h, w = cam.image_height, cam.image_width
        linear = np.zeros((h, w, 3), np.float64)
        rgb8 = np.zeros((h, w, 3), np.uint8)
        opts = RenderOpts(seed, real_mode, 0, 1, 0, variant, None)
        self._check(self._lib.rtk_render_multi(self._m, C.byref(cam), C.byref(opts), linear.ctypes.data, rgb8.ctypes.data))
        return linear, rgb8

    def render_device(self, cam: Camera, d_linear: int, d_rgb8: int = 0, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, variant: int = 0) -> None:
        """rtk_render_multi_device: blocking; the image is resident on devices[0] on return."""
        opts = RenderOpts(seed, real_mode, 0, 1, 0, variant, None)
        self._check(self._lib.rtk_render_multi_device(self._m, C.byref(cam), C.byref(opts), d_linear or None, d_rgb8 or None))

    def enqueue_device(self, cam: Camera, d_linear: int, d_rgb8: int = 0, *, seed: int = RENDER_SEED, real_mode: int = RTK_REAL_F64, variant: int = 0) -> None:
        """rtk_render_multi_enqueue: returns once the frame is enqueued (two frames in flight: this frame's gather and
        un-permute overlap the next frame's renders); the buffers must stay valid until wait()."""
        opts = RenderOpts(seed, real_mode, 0, 1, 0, variant, None)
        self._check(self._lib.rtk_render_multi_enqueue(self._m, C.byref(cam), C.byref(opts), d_linear or None, d_rgb8 or None))

    def wait(self) -> None:
        """rtk_multi_wait: every enqueued frame is complete on devices[0]."""
        self._check(self._lib.rtk_multi_wait(self._m))

    def close(self) -> None:
        if getattr(self, "_m", None):
            self._lib.rtk_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
