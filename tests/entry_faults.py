"""The lane-per-ray entry points (include/rtk.h: ray queries, rtk_debug_*, light probes, surface gathers, lens models) as a table:
for each of the 30 a good call with a null context and the named faults it can be given.

A fault is a field or an argument with a bad value: Fault(name, group, sets, names, solo).  `sets` overrides entries of the good
call's state ({key: value}, or a function of the Buffers for values that are addresses); `group` is the field it makes bad, so that
mutually exclusive bad values of one field are alternatives of one group; `names` is the part of the refusal's text that names the
fault (the peel chains of tests/golden/make_entry_refusals.py remove the fault the text names); `solo` faults override more than
their own field -- or are no faults at all, such as n = 0 -- and are only ever applied alone.

tests/golden/make_entry_refusals.py records what a library answers to them, tests/test_entry_refusals.py replays the record.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

Fault = namedtuple("Fault", "name group sets names solo")
Entry = namedtuple("Entry", "name good invoke faults terminal")

NAN, INF, PI = float("nan"), float("inf"), math.pi


def fault(name, group, sets, names="", solo=False):
    return Fault(name, group, sets, names, solo)


def _carve(nbytes, fill):
    """(owner, view): `nbytes` bytes on a 64-byte boundary, every byte of the owner `fill`."""
    raw = np.full(nbytes + 64, fill, np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw, raw[off:off + nbytes]


class Buffers:
    """The arrays every call points at: four rays, four points, four normals, the coefficients of two probes, and an output
    large enough for anything an entry point could write for them.  untouched() is what the refusal tests end with."""

    def __init__(self, rt):
        self._owners = []
        self.rays = self._input(4 * 88)
        self._view(self.rays).view(rt.ray_dtype())[:] = rt.make_rays(np.zeros((4, 3)), np.ones((4, 3)))
        self.points = self._input(4 * 24)
        self.normals = self._input(4 * 24)
        self._view(self.normals).view(np.float64)[:] = np.tile([0.0, 0.0, 1.0], 4)
        self.sh = self._input(2 * 27 * 8)
        self.out = self._input(128 * 1024, 0x5A)
        self._before = [raw.copy() for raw, _ in self._owners]

    def _input(self, nbytes, fill=0):
        self._owners.append(_carve(nbytes, fill))
        return self._owners[-1][1].ctypes.data

    def _view(self, address):
        return next(view for _, view in self._owners if view.ctypes.data == address)

    def untouched(self):
        return all(np.array_equal(raw, before) for (raw, _), before in zip(self._owners, self._before))


def _state(good, faults, b):
    """The good call's state with `faults` applied; values that depend on the buffers resolved."""
    s = dict(good)
    for f in faults:
        s.update(f.sets)
    return {k: (v(b) if callable(v) else v) for k, v in s.items()}


def call(entry, lib, rt, b, faults):
    """(return code, rtk_last_error text) of `entry` with `faults` (Fault records) applied to its good null-context call."""
    rc = entry.invoke(lib, rt, _state(entry.good, faults, b))
    return int(rc), lib.rtk_last_error().decode()


OPTS_FAULTS = [fault("null_opts", "opts", {"opts": False}, "null opts"),
               fault("real_mode_2", "real_mode", {"real_mode": 2}, "unknown real_mode"),
               fault("real_mode_negative", "real_mode", {"real_mode": -1}, "unknown real_mode"),
               fault("max_depth_negative", "max_depth", {"max_depth": -1}, "max_depth must not be negative"),
               fault("samples_negative", "samples", {"samples": -1}, "samples must not be negative")]


# ------------------------------------------------------------------------------------------------------ ray queries --
def _query(name):
    host, kind = name.endswith("_host"), name.split("_")[2]
    p, radiance = ("h_" if host else "d_"), kind == "radiance"
    good = {"opts": True, "real_mode": 0, "max_depth": 5, "samples": 1, "reserved": (0, 0), "n": 4, "rays": lambda b: b.rays, "out": lambda b: b.out,
            "draws": None}

    def invoke(lib, rt, s):
        o = rt.QueryOpts(7, s["real_mode"], s["max_depth"], s["samples"], rt.Vec3(0.5, 0.5, 0.5), None, (C.c_int32 * 2)(*s["reserved"]))
        extra = (s["draws"],) if radiance else ()
        return getattr(lib, name)(None, C.byref(o) if s["opts"] else None, s["n"], s["rays"], s["out"], *extra)

    faults = OPTS_FAULTS + [
        fault("reserved_first", "reserved", {"reserved": (1, 0)}, "reserved must be 0"), fault("reserved_second", "reserved", {"reserved": (0, -5)}, "reserved must be 0"),
        fault("n_negative", "n", {"n": -1}, " n must be"), fault("n_2p31", "n", {"n": 2 ** 31}, " n must be"), fault("n_2p40", "n", {"n": 2 ** 40}, " n must be"),
        fault("null_rays", "rays", {"rays": None}, "null %srays" % p), fault("null_out", "out", {"out": None}, "null %s%s" % (p, kind)),
        fault("n_zero", "n", {"n": 0}, solo=True)]
    if not host:
        faults += [fault("rays_misaligned", "rays", {"rays": lambda b: b.rays + 4}, "d_rays must be"),
                   fault("out_misaligned", "out", {"out": lambda b: b.out + (2 if kind == "occluded" else 4)}, "d_%s must be" % kind),
                   fault("out_inside_rays", "out", {"out": lambda b: b.rays + 88 * 3 + 80}, "d_%s overlaps d_rays" % kind),    # starts inside the last ray record
                   fault("out_before_rays", "out", {"rays": lambda b: b.rays + 8, "out": lambda b: b.rays}, solo=True)]
    if radiance and not host:
        faults += [fault("draws_misaligned", "draws", {"draws": lambda b: b.out + 4096 + 2}, "d_draws must be"),
                   fault("draws_inside_rays", "draws", {"draws": lambda b: b.rays + 8}, "d_draws overlaps d_rays"),
                   fault("f32_out_4_bytes", "out", {"real_mode": 1, "out": lambda b: b.out + 4}, solo=True),                   # F32 radiance needs 4 bytes only
                   fault("f32_out_2_bytes", "out", {"real_mode": 1, "out": lambda b: b.out + 2}, solo=True)]
    return Entry(name, good, invoke, faults, "null context")


# -------------------------------------------------------------------------------------- known-answer entry points --
DEBUG_POINTERS = {"rtk_debug_closest_hit": ("rays", "keys", "out", "draws"), "rtk_debug_scatter": ("materials", "rays", "records", "keys", "out", "draws"),
                  "rtk_debug_texture": ("textures", "uvp", "out", "work"), "rtk_debug_get_ray": ("pixel_sample", "out", "draws")}


def _debug(name):
    pointers, get_ray = DEBUG_POINTERS[name], name == "rtk_debug_get_ray"
    good = {"real_mode": 0, "n": 4, "cam": True}
    good.update({k: (lambda b: b.out) if k in ("out", "draws", "work") else (lambda b: b.points) for k in pointers})

    def invoke(lib, rt, s):
        head = (None, s["real_mode"])
        if get_ray:
            cam = rt.Camera()
            cam.image_width = cam.image_height = 8
            head += (C.byref(cam) if s["cam"] else None, 7)
        return getattr(lib, name)(*head, s["n"], *(s[k] for k in pointers))

    faults = [fault("n_negative", "n", {"n": -1}, "bad argument"), fault("real_mode_2", "real_mode", {"real_mode": 2}, "bad argument"),
              fault("n_zero", "n", {"n": 0}, solo=True)]
    faults += [fault("null_" + k, k, {k: None}, "bad argument") for k in pointers]
    if get_ray:
        faults.append(fault("null_cam", "cam", {"cam": False}, "bad argument"))
    return Entry(name, good, invoke, faults, "bad argument")


# ----------------------------------------------------------------------------------------------------- light probes --
def _probe(name):
    host, bake = name.endswith("_host"), "bake" in name
    p, out = ("h_" if host else "d_"), ("sh" if bake else "rays")
    good = {"opts": True, "real_mode": 0, "max_depth": 5, "samples": 1, "rays": 256, "reserved": (0, 0), "n": 4, "positions": lambda b: b.points,
            "out": lambda b: b.out}

    def invoke(lib, rt, s):
        o = rt.ProbeOpts(7, s["real_mode"], s["max_depth"], s["samples"], s["rays"], 0, rt.Vec3(0.5, 0.5, 0.5), 0.0, None, (C.c_int32 * 2)(*s["reserved"]))
        return getattr(lib, name)(None, C.byref(o) if s["opts"] else None, s["n"], s["positions"], s["out"])

    faults = OPTS_FAULTS + [
        fault("reserved_first", "reserved", {"reserved": (1, 0)}, "reserved must be 0"), fault("reserved_second", "reserved", {"reserved": (0, -5)}, "reserved must be 0"),
        fault("n_negative", "n", {"n": -1}, " n must not be negative"), fault("n_times_rays_2p31", "n", {"n": 2 ** 23}, "n * rays must not exceed"),
        fault("null_positions", "positions", {"positions": None}, "null %spositions" % p), fault("null_out", "out", {"out": None}, "null %s%s" % (p, out)),
        fault("n_zero", "n", {"n": 0}, solo=True), fault("most_rays_allowed", "n", {"rays": 65536, "n": 2 ** 15 - 1}, solo=True)]
    faults += [fault("rays_%d" % r, "rays", {"rays": r}, "rays must be a multiple of 256") for r in (255, 128, 257, 1000, 65536 + 256)]
    faults.append(fault("rays_negative", "rays", {"rays": -256}, "rays must be a multiple of 256"))
    faults += [fault("n_times_rays_%d_%d" % (r, k), "n", {"rays": r, "n": 2 ** k}, solo=True) for r, k in ((65536, 15), (0, 21), (256, 40))]
    if not host:
        faults += [fault("positions_misaligned", "positions", {"positions": lambda b: b.points + 4}, "d_positions must be"),
                   fault("out_misaligned", "out", {"out": lambda b: b.out + 4}, "d_%s must be" % out)]
    if bake and not host:                                           # F32 coefficients need 4 bytes only
        faults += [fault("f32_out_4_bytes", "out", {"real_mode": 1, "out": lambda b: b.out + 4}, solo=True),
                   fault("f32_out_2_bytes", "out", {"real_mode": 1, "out": lambda b: b.out + 2}, solo=True)]
    return Entry(name, good, invoke, faults, "null context")


def _probe_irradiance(name):
    host = name.endswith("_host")
    p = "h_" if host else "d_"
    arrays = ("sh", "points", "normals", "irradiance")
    good = {"real_mode": 0, "grid": True, "counts": (2, 1, 1), "spacing": (1.0, 1.0, 1.0), "grid_reserved": 0, "m": 4, "sh": lambda b: b.sh,
            "points": lambda b: b.points, "normals": lambda b: b.normals, "irradiance": lambda b: b.out}

    def invoke(lib, rt, s):
        g = rt.ProbeGrid(rt.Vec3(0.0, 0.0, 0.0), rt.Vec3(*s["spacing"]), (C.c_int32 * 3)(*s["counts"]), s["grid_reserved"])
        extra = () if host else (None,)
        return getattr(lib, name)(None, s["real_mode"], C.byref(g) if s["grid"] else None, s["sh"], s["m"], s["points"], s["normals"], s["irradiance"], *extra)

    faults = [fault("real_mode_2", "real_mode", {"real_mode": 2}, "unknown real_mode"), fault("real_mode_negative", "real_mode", {"real_mode": -1}, "unknown real_mode"),
              fault("null_grid", "grid", {"grid": False}, "null grid"),
              fault("counts_x_zero", "counts", {"counts": (0, 1, 1)}, "grid counts must be at least 1 (counts[0]"),
              fault("counts_y_negative", "counts", {"counts": (2, -1, 1)}, "grid counts must be at least 1 (counts[1]"),
              fault("counts_z_zero", "counts", {"counts": (2, 1, 0)}, "grid counts must be at least 1 (counts[2]"),
              fault("counts_2p32_probes", "counts", {"counts": (65536, 65536, 1)}, "grid counts: more than"),
              fault("spacing_x_zero", "spacing", {"spacing": (0.0, 1.0, 1.0)}, "grid spacing must be positive in the real type (spacing[0]"),
              fault("spacing_y_negative", "spacing", {"spacing": (1.0, -2.0, 1.0)}, "grid spacing must be positive in the real type (spacing[1]"),
              fault("spacing_z_nan", "spacing", {"spacing": (1.0, 1.0, NAN)}, "grid spacing must be positive in the real type (spacing[2]"),
              fault("spacing_y_zero_as_float", "spacing", {"real_mode": 1, "spacing": (1.0, 1e-50, 1.0)}, solo=True),
              fault("spacing_y_tiny_as_double", "spacing", {"spacing": (1.0, 1e-50, 1.0)}, solo=True),
              fault("grid_reserved", "grid_reserved", {"grid_reserved": 3}, "grid reserved must be 0"),
              fault("m_negative", "m", {"m": -1}, " m must be"), fault("m_2p31", "m", {"m": 2 ** 31}, " m must be"), fault("n_zero", "m", {"m": 0}, solo=True)]
    faults += [fault("null_" + k, k, {k: None}, "null %s%s" % (p, k)) for k in arrays]
    if not host:
        source = {"sh": lambda b: b.sh + 4, "points": lambda b: b.points + 4, "normals": lambda b: b.normals + 4, "irradiance": lambda b: b.out + 4}
        faults += [fault(k + "_misaligned", k, {k: source[k]}, "d_%s must be" % k) for k in arrays]
        faults += [fault("f32_%s_4_bytes" % k, k, {"real_mode": 1, k: source[k]}, solo=True) for k in arrays]       # F32: 4 bytes are enough
    return Entry(name, good, invoke, faults, "null context")


# -------------------------------------------------------------------------------------------------- surface gathers --
def _gather(name):
    host, occlusion = name.endswith("_host"), "occlusion" in name
    p, out = ("h_" if host else "d_"), name.split("_")[2].replace("occlusion", "open")
    good = {"opts": True, "real_mode": 0, "max_depth": 5, "samples": 1, "rays": 64, "rotate": 0, "batch_points": 0, "max_distance": 0.0, "reserved": (0, 0, 0, 0),
            "n": 4, "points": lambda b: b.points, "normals": lambda b: b.normals, "out": lambda b: b.out, "bent": lambda b: b.out + 2048}

    def invoke(lib, rt, s):
        o = rt.GatherOpts(7, s["real_mode"], s["max_depth"], s["samples"], s["rays"], 0, s["rotate"], s["batch_points"], rt.Vec3(0.5, 0.5, 0.5), 0.0, s["max_distance"],
                          None, (C.c_int32 * 4)(*s["reserved"]))
        extra = (s["bent"],) if occlusion else ()
        return getattr(lib, name)(None, C.byref(o) if s["opts"] else None, s["n"], s["points"], s["normals"], s["out"], *extra)

    faults = OPTS_FAULTS + [
        fault("reserved_first", "reserved", {"reserved": (1, 0, 0, 0)}, "reserved must be 0"), fault("reserved_last", "reserved", {"reserved": (0, 0, 0, -5)}, "reserved must be 0"),
        fault("n_negative", "n", {"n": -1}, " n must not be negative"), fault("n_times_rays_2p31", "n", {"n": 2 ** 25}, "n * rays must not exceed"),
        fault("rotate_2", "rotate", {"rotate": 2}, "rotate must be 0 or 1"), fault("rotate_negative", "rotate", {"rotate": -1}, "rotate must be 0 or 1"),
        fault("batch_points_negative", "batch_points", {"batch_points": -1}, "batch_points must not be negative"),
        fault("max_distance_negative", "max_distance", {"max_distance": -1.0}, "max_distance must not be negative"),
        fault("max_distance_nan", "max_distance", {"max_distance": NAN}, "max_distance must not be negative"),
        fault("null_points", "points", {"points": None}, "null %spoints" % p), fault("null_normals", "normals", {"normals": None}, "null %snormals" % p),
        fault("n_zero", "n", {"n": 0}, solo=True)]
    faults += [fault("rays_%d" % r, "rays", {"rays": r}, "rays must be a multiple of 64") for r in (63, 96, 16448, 32)]
    faults.append(fault("rays_negative", "rays", {"rays": -64}, "rays must be a multiple of 64"))
    faults += [fault("n_times_rays_%d_%d" % (r, k), "n", {"rays": r, "n": 2 ** k}, solo=True) for r, k in ((16384, 17), (0, 23), (64, 40))]
    faults += [fault("every_option_%d" % r, "rays", {"rays": r, "rotate": 1, "batch_points": 3, "max_distance": 2.5, "n": 1}, solo=True) for r in (64, 16384, 0)]
    if occlusion:                                                 # both outputs null; one alone is enough
        faults += [fault("null_open_and_bent", "out", {"out": None, "bent": None}, "null %sopen and %sbent" % (p, p), solo=True),
                   fault("null_open_alone", "out", {"out": None}, solo=True), fault("null_bent_alone", "bent", {"bent": None}, solo=True)]
    else:
        faults.append(fault("null_out", "out", {"out": None}, "null %s%s" % (p, out)))
    if not host:
        faults += [fault("points_misaligned", "points", {"points": lambda b: b.points + 4}, "d_points must be"),
                   fault("normals_misaligned", "normals", {"normals": lambda b: b.normals + 4}, "d_normals must be"),
                   fault("out_misaligned", "out", {"out": lambda b: b.out + 4}, "d_%s must be" % out),
                   fault("out_inside_points", "out", {"out": lambda b: b.points + 8}, "d_%s overlaps d_points" % out),
                   fault("out_at_normals", "out", {"out": lambda b: b.normals}, "d_%s overlaps d_normals" % out)]
        if occlusion:
            faults += [fault("bent_misaligned", "bent", {"bent": lambda b: b.out + 2052}, "d_bent must be"),
                       fault("bent_inside_normals", "bent", {"bent": lambda b: b.normals + 16}, "d_bent overlaps d_normals")]
        if name != "rtk_gather_rays":                             # F32 reals need 4 bytes only
            faults += [fault("f32_out_4_bytes", "out", {"real_mode": 1, "out": lambda b: b.out + 4}, solo=True),
                       fault("f32_out_2_bytes", "out", {"real_mode": 1, "out": lambda b: b.out + 2}, solo=True)]
    return Entry(name, good, invoke, faults, "null context")


# ------------------------------------------------------------------------------------------------------ lens models --
LENS_EQUIRECT, LENS_FISHEYE, LENS_ORTHOGRAPHIC = 1, 2, 3
LENS_OUT = {"rays": "rays", "render": "linear", "aovs": "aov", "guides": "guides"}


def _lens(name):
    host, form = name.endswith("_host"), name.split("_")[2]
    p, out = ("h_" if host else "d_"), LENS_OUT[form]
    good = {"lens": True, "opts": True, "real_mode": 0, "n_ranks": 1, "first": 0, "n": 3, "out": lambda b: b.out, "noise": None, "gopts": None}

    def invoke(lib, rt, s):
        lens = rt.derive_lens(LENS_EQUIRECT, 24, 16, spp=3, max_depth=5, lookfrom=(0, 0, 1), lookat=(0, 0, -1), background=(0.5, 0.6, 0.7), ortho_width=4.0,
                              ortho_height=3.0)
        for k, v in s.items():
            if k.startswith("cam."):
                setattr(lens.cam, k[4:], rt.Vec3(*v) if isinstance(v, tuple) else v)
            elif k.startswith("lens."):
                setattr(lens, k[5:], rt.Vec3(*v) if isinstance(v, tuple) else v)
        o = rt.RenderOpts(7, s["real_mode"], 0, s["n_ranks"], 0, 0, None)
        head = (None, C.byref(lens) if s["lens"] else None, C.byref(o) if s["opts"] else None)
        gopts = C.byref(rt.GuideOpts(*s["gopts"])) if s["gopts"] else None
        tail = {"rays": (s["first"], s["n"], s["out"]), "render": (s["first"], s["out"], s["noise"]), "aovs": (s["n"], s["out"]), "guides": (s["n"], gopts, s["out"])}[form]
        return getattr(lib, name)(*head, *tail)

    def field(key, value, names, tag):
        return fault("%s_%s" % (key.split(".")[1], tag), key, {key: value}, names)

    faults = [fault("null_lens", "lens", {"lens": False}, "null lens"), fault("null_opts", "opts", {"opts": False}, "null opts"),
              fault("null_out", "out", {"out": None}, "null %s%s" % (p, out)),
              field("lens.model", 4, "unknown model", "4"), field("lens.model", -1, "unknown model", "negative"), field("lens.reserved", 1, "reserved must be 0", "1"),
              field("lens.fov_h", -0.5, "fov_h must lie", "negative"), field("lens.fov_h", 2 * PI + 1e-9, "fov_h must lie", "above_2pi"),
              field("lens.fov_h", NAN, "fov_h must be finite", "nan"), field("lens.fov_h", INF, "fov_h must be finite", "inf"),
              field("lens.fov_v", -1.0, "fov_v must lie", "negative"), field("lens.fov_v", PI + 1e-9, "fov_v must lie", "above_pi"),
              field("lens.fov_v", NAN, "fov_v must be finite", "nan"), field("lens.ortho_width", INF, "ortho_width must be finite", "inf"),
              field("lens.u", (NAN, 0, 0), " u must be finite", "nan"), field("lens.v", (0, INF, 0), " v must be finite", "inf"),
              field("lens.w", (0, 0, -INF), " w must be finite", "inf"), field("cam.center", (0, NAN, 0), "cam.center must be finite", "nan"),
              field("cam.background", (INF, 0, 0), "cam.background must be finite", "inf"),
              field("cam.pixel_samples_scale", NAN, "cam.pixel_samples_scale must be finite", "nan"),
              field("cam.image_width", 0, "bad camera dimensions", "zero"), field("cam.image_width", 65537, "bad camera dimensions", "65537"),
              field("cam.image_height", -3, "bad camera dimensions", "negative"), field("cam.max_depth", -1, "cam.max_depth must not be negative", "negative"),
              field("cam.samples_per_pixel", -1, "cam.samples_per_pixel must not be negative", "negative"),
              fault("real_mode_2", "real_mode", {"real_mode": 2}, "unknown real_mode"), fault("real_mode_negative", "real_mode", {"real_mode": -1}, "unknown real_mode"),
              fault("n_ranks_2", "n_ranks", {"n_ranks": 2}, "whole images only"), fault("n_ranks_0", "n_ranks", {"n_ranks": 0}, "whole images only")]
    ortho = {"lens.model": LENS_ORTHOGRAPHIC}                      # the window is the orthographic lens's alone, fov_v the panorama's
    faults += [fault("ortho_width_zero", "lens.ortho_width", dict(ortho, **{"lens.ortho_width": 0.0}), solo=True),
               fault("ortho_width_negative", "lens.ortho_width", dict(ortho, **{"lens.ortho_width": -2.0}), solo=True),
               fault("ortho_height_zero", "lens.ortho_height", dict(ortho, **{"lens.ortho_height": 0.0}), solo=True),
               fault("ortho_height_nan", "lens.ortho_height", dict(ortho, **{"lens.ortho_height": NAN}), solo=True),
               fault("fisheye_ignores_fov_v", "lens.fov_v", {"lens.model": LENS_FISHEYE, "lens.fov_v": -1.0}, solo=True),
               fault("widest_extents", "lens.fov_h", {"lens.fov_h": 2 * PI, "lens.fov_v": PI}, solo=True),
               fault("default_extents", "lens.fov_h", {"lens.fov_h": 0.0, "lens.fov_v": 0.0, "lens.ortho_width": 0.0, "lens.ortho_height": 0.0}, solo=True)]
    if form in ("rays", "render"):
        faults.append(fault("first_sample_negative", "first", {"first": -1}, "first_sample must not be negative"))
    if form == "render":
        faults += [field("cam.samples_per_pixel", 0, "cam.samples_per_pixel must be at least 1", "zero"),
                   fault("frame_of_2p32_samples", "n", {"cam.image_width": 65536, "cam.image_height": 65536, "cam.samples_per_pixel": 1}, solo=True)]
    else:
        faults += [fault("n_samples_negative", "n", {"n": -1}, "n_samples must be at least"),
                   fault("frame_of_2p31_samples", "n", {"cam.image_width": 32768, "cam.image_height": 32768, "n": 2}, solo=True),
                   fault("frame_of_2p30_samples", "n", {"cam.image_width": 32768, "cam.image_height": 32768, "n": 1}, solo=True),
                   fault("n_zero", "n", {"n": 0}, solo=True)]
    if form == "guides":
        faults += [fault("follow_bits_unknown", "gopts", {"gopts": (4, 0)}, "unknown follow bits"), fault("max_bounces_9", "gopts", {"gopts": (0, 9)}, "max_bounces 9 out of range"),
                   fault("n_samples_above_2p20", "n", {"n": 2 ** 20 + 1}, "n_samples must be 1 .. 2^20")]
    if not host:                                                  # alignment: 8 for records and F64 reals, 4 for F32 reals and se, 16 for guides
        faults.append(fault("out_misaligned", "out", {"out": lambda b: b.out + 4}, "d_%s must be" % out))
        if form == "render":
            faults += [fault("noise_misaligned", "noise", {"noise": lambda b: b.out + 65536 + 2}, "d_noise must be"),
                       fault("f32_out_4_bytes", "out", {"real_mode": 1, "out": lambda b: b.out + 4}, solo=True)]
        if form in ("aovs", "guides"):
            faults.append(fault("out_8_bytes", "out", {"out": lambda b: b.out + 8}, "d_%s must be" % out))
    return Entry(name, good, invoke, faults, "null context")


def _both(maker, *names):
    return [maker(n + suffix) for suffix in ("", "_host") for n in names]


ENTRIES = {e.name: e for e in (_both(_query, "rtk_query_hits", "rtk_query_occluded", "rtk_query_radiance") + [_debug(n) for n in DEBUG_POINTERS] +
                               _both(_probe, "rtk_probe_rays", "rtk_probe_bake") + _both(_probe_irradiance, "rtk_probe_irradiance") +
                               _both(_gather, "rtk_gather_rays", "rtk_gather_irradiance", "rtk_gather_occlusion") +
                               _both(_lens, "rtk_lens_rays", "rtk_lens_render", "rtk_lens_aovs", "rtk_lens_guides"))}
assert len(ENTRIES) == 30
