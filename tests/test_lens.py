"""Lens models (include/rtk.h "Lens models"): panoramic, fisheye and orthographic frames made on the device.

The sample rule is restated in numpy in tests/lens_rules.py, which uses nothing of the package.

CPU tests: the entry points are declared and exported and RTK_ABI_VERSION stays 2; rtk_lens is 312 bytes with the header's
offsets; every refusal comes back as RTK_ERR_INVALID naming its entry point and its argument, with no device and no context;
rtk_lens_look_at is the frame derive_camera computes, bit for bit; no seed in 2^20 makes the centre pixel's jitter vanish.

GPU tests (shapes 24x16 and 19x11: partial tiles and a partial last workgroup; S = 3; first_sample 0 and 5):
  3. the emitted rays are the restatement's;
  4. RTK_LENS_PERSPECTIVE is get_ray: rays, AOVs and guides bit for bit, the frame under the F64 bound;
  5. the frame is the radiance query over its rays, summed in sample order: bit for bit; se within one float ulp;
  6. F64 against the oracle's ray_color over the records;
  7. AOVs against rtk_query_hits over the rekeyed records;
  8. continuation, repeatability, caller streams and carved buffers, misaligned guide buffers;
  9. a light on the +u side shows in the right half, and in the left half from the opposite side;
  10. camera::projection of the host C++ API (tests/helpers/lens_camera_check.cpp).
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import lens_rules as rules
from tests.conftest import GOLDEN, ROOT
from tests.scene_cases import IMAGE_CASES, SCENE_SEED, scene_file

PKG = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
ENTRY_POINTS = ("rtk_lens_rays", "rtk_lens_render", "rtk_lens_aovs", "rtk_lens_guides")
CASES = {c[0]: c for c in IMAGE_CASES}
ORDERS = ("reference", "fast")
MODES = pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
MODELS = (rules.EQUIRECT, rules.FISHEYE, rules.ORTHOGRAPHIC)
MODEL_NAMES = {rules.PERSPECTIVE: "perspective", rules.EQUIRECT: "equirect", rules.FISHEYE: "fisheye", rules.ORTHOGRAPHIC: "orthographic"}
U64 = 2.0 ** -53
SEED = 5
S = 3
# (width, height, first_sample, explicit extents?): every shape has partial 8x8 tiles; 19x11 also leaves the last workgroup of
# rtk_lens_rays partly empty (627 records) and takes the models' extents from the lens instead of the defaults.
SHAPES = ((24, 16, 0, False), (19, 11, 5, True))

# Where the lens stands in each scene, what it looks at, and the orthographic window (checked against
# host/scenes/scene_library.h: every point is off every surface; the Cornell lens is inside the box).
VIEWS = {"three_spheres": ((0.0, 0.25, 0.5), (0.0, 0.0, -1.0), 4.0, 2.7),
         "cornell_box": ((278.0, 278.0, 60.0), (278.0, 260.0, 555.0), 500.0, 330.0),
         "single_fog": ((0.0, 0.0, 1.0), (0.0, 0.0, -3.0), 3.0, 2.0),
         "material_zoo": ((0.0, 2.0, -2.0), (0.0, 1.0, 5.0), 12.0, 8.0),
         "book1_final": ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 10.0, 6.0)}


def _lens(rt, model, name, width, height, spp, depth, background, explicit=False):
    lookfrom, lookat, ow, oh = VIEWS[name]
    fov = {}
    if explicit:
        fov = dict(fov_h=4.0, fov_v=2.0) if model == rules.EQUIRECT else dict(fov_h=2.6)
    return rt.derive_lens(model, width, height, spp=spp, max_depth=depth, lookfrom=lookfrom, lookat=lookat, background=background, ortho_width=ow, ortho_height=oh,
                          **(fov if model != rules.ORTHOGRAPHIC else {}))


def _v3(v):
    return np.array([v.x, v.y, v.z])


def _restated(lens, samples, first_sample, seed, jitter=None):
    half_h, half_v = rules.halves(lens.model, lens.fov_h, lens.fov_v, lens.ortho_width, lens.ortho_height)
    return rules.film_records(lens.model, lens.cam.image_width, lens.cam.image_height, samples, first_sample, seed, _v3(lens.cam.center), _v3(lens.u), _v3(lens.v),
                              _v3(lens.w), half_h, half_v, jitter)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ------------------------------------------------------------------------------------------------------------- CPU --
def test_entry_points_are_declared_and_exported(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    assert "#define RTK_ABI_VERSION 2" in header and "Lens models ---" in header
    for k, name in enumerate(("PERSPECTIVE", "EQUIRECT", "FISHEYE", "ORTHOGRAPHIC")):
        assert re.search(r"#define RTK_LENS_%s\s+%d\b" % (name, k), header), name
    for name in ENTRY_POINTS:
        for form in (name, name + "_host"):
            assert re.search(r"\bint %s\(rtk_ctx\* ctx, const rtk_lens\* lens, const rtk_render_opts\* opts, " % form, header), form
    assert re.search(r"\bint rtk_lens_look_at\(rtk_lens\* lens, rtk_vec3 lookfrom, rtk_vec3 lookat, rtk_vec3 vup\);", header)
    lib = C.CDLL(rt.HIP_LIB_PATH)                                 # loads without a GPU
    missing = [n for n in ENTRY_POINTS + tuple(n + "_host" for n in ENTRY_POINTS) + ("rtk_lens_look_at",) if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.rtk_abi_version() == 2
    assert (rt.LENS_PERSPECTIVE, rt.LENS_EQUIRECT, rt.LENS_FISHEYE, rt.LENS_ORTHOGRAPHIC) == (0, 1, 2, 3)
    import __graft_entry__

    assert "rtk_lens.cpp" in __graft_entry__.HIP_SOURCES
    for method in ("lens_rays", "lens_render", "lens_aovs", "lens_guides", "lens_rays_device", "lens_render_device", "lens_aovs_device", "lens_guides_device"):
        assert callable(getattr(rt.Renderer, method)), method
    camera_h = open(os.path.join(PKG, "host", "rtk_camera.h")).read()
    assert all(word in camera_h for word in ("projection", "equirect", "fisheye", "orthographic", "ortho_width", "rtk_lens_render_host"))
    with pytest.raises(ValueError):
        rt.derive_lens(rt.LENS_PERSPECTIVE, 8, 8)                 # the perspective lens is a whole camera
    with pytest.raises(ValueError):
        rt.derive_lens(rt.LENS_FISHEYE, cam=rt.Camera())


def test_the_structure_has_the_headers_layout(rt, tmp_path):
    """sizeof(rtk_lens) == 312 and every field offset of the ctypes structure equals that of a C program compiled against rtk.h."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rtk.h"', "int main(void) {", '    printf("size %zu\\n", sizeof(rtk_lens));']
    for field, _ in rt.Lens._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(rtk_lens, %s));' % (field, field))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = {line.split()[0]: int(line.split()[1]) for line in subprocess.check_output([str(exe)]).decode().splitlines()}
    assert want["size"] == 312 == C.sizeof(rt.Lens)
    for field, _ in rt.Lens._fields_:
        assert getattr(rt.Lens, field).offset == want[field], field
    assert (want["cam"], want["model"], want["reserved"], want["u"], want["w"], want["fov_h"], want["ortho_height"]) == (0, 200, 204, 208, 256, 280, 304)


def _good(rt, model=rules.EQUIRECT, **kw):
    lens = rt.derive_lens(model, 24, 16, spp=3, max_depth=5, lookfrom=(0, 0, 1), lookat=(0, 0, -1), background=(0.5, 0.6, 0.7), ortho_width=4.0, ortho_height=3.0)
    for k, v in kw.items():
        obj, field = (lens.cam, k[4:]) if k.startswith("cam_") else (lens, k)
        setattr(obj, field, v)
    return lens


def test_refusals_need_no_device(rt):
    """Every refusal of the header's list is RTK_ERR_INVALID, the text starting with the entry point and naming the argument,
    from all eight entry points with a null context: the checks come before anything that needs a device.  With nothing to
    refuse the answer is "null context".  Nothing is written."""
    lib = rt.hip_lib()
    err = lambda: lib.rtk_last_error().decode()  # noqa: E731
    out = np.full(24 * 16 * 3 * 88 + 64, 0x5A, np.uint8)          # large enough for any output of a 24x16 lens with three samples
    out_ptr = out.ctypes.data + (-out.ctypes.data) % 16
    opts = rt.RenderOpts(7, 0, 0, 1, 0, 0, None)
    nan, inf, pi = float("nan"), float("inf"), math.pi
    V = rt.Vec3
    bad_lens = [(dict(model=4), "model"), (dict(model=-1), "model"), (dict(reserved=1), "reserved"),
                (dict(fov_h=-0.5), "fov_h"), (dict(fov_h=2 * pi + 1e-9), "fov_h"), (dict(fov_h=nan), "fov_h"), (dict(fov_h=inf), "fov_h"),
                (dict(fov_v=-1.0), "fov_v"), (dict(fov_v=pi + 1e-9), "fov_v"), (dict(fov_v=nan), "fov_v"),
                (dict(model=rules.ORTHOGRAPHIC, ortho_width=0.0), "ortho_width"), (dict(model=rules.ORTHOGRAPHIC, ortho_width=-2.0), "ortho_width"),
                (dict(model=rules.ORTHOGRAPHIC, ortho_height=0.0), "ortho_height"), (dict(model=rules.ORTHOGRAPHIC, ortho_height=nan), "ortho_height"),
                (dict(ortho_width=inf), "ortho_width"),
                (dict(u=V(nan, 0, 0)), " u "), (dict(v=V(0, inf, 0)), " v "), (dict(w=V(0, 0, -inf)), " w "),
                (dict(cam_center=V(0, nan, 0)), "cam.center"), (dict(cam_background=V(inf, 0, 0)), "cam.background"),
                (dict(cam_pixel_samples_scale=nan), "cam.pixel_samples_scale"),
                (dict(cam_image_width=0), "camera dimensions"), (dict(cam_image_height=-3), "camera dimensions"), (dict(cam_image_width=65537), "camera dimensions"),
                (dict(cam_max_depth=-1), "max_depth"), (dict(cam_samples_per_pixel=-1), "samples_per_pixel")]
    calls = {"rtk_lens_rays": lambda fn, ctx, lens, o, p, first=0, n=3: fn(ctx, lens, o, first, n, p),
             "rtk_lens_render": lambda fn, ctx, lens, o, p, first=0, n=3: fn(ctx, lens, o, first, p, None),
             "rtk_lens_aovs": lambda fn, ctx, lens, o, p, first=0, n=3: fn(ctx, lens, o, n, p),
             "rtk_lens_guides": lambda fn, ctx, lens, o, p, first=0, n=3: fn(ctx, lens, o, n, None, p)}
    for base, call in calls.items():
        for name in (base, base + "_host"):
            fn = getattr(lib, name)
            host = name.endswith("_host")
            ok = lambda word: word in err() and err().startswith(name + ":")  # noqa: E731,B023
            for fields, word in bad_lens:
                assert call(fn, None, C.byref(_good(rt, **fields)), C.byref(opts), out_ptr) == -1, (name, fields)
                assert ok(word), (name, fields, err())
            assert call(fn, None, None, C.byref(opts), out_ptr) == -1 and ok("null lens"), err()
            assert call(fn, None, C.byref(_good(rt)), None, out_ptr) == -1 and ok("null opts"), err()
            assert call(fn, None, C.byref(_good(rt)), C.byref(opts), None) == -1 and re.search(r"null [dh]_(rays|linear|aov|guides)", err()) and ok("null"), err()
            for mode in (2, -1):
                assert call(fn, None, C.byref(_good(rt)), C.byref(rt.RenderOpts(7, mode, 0, 1, 0, 0, None)), out_ptr) == -1 and ok("real_mode"), err()
            for ranks in (2, 0):
                assert call(fn, None, C.byref(_good(rt)), C.byref(rt.RenderOpts(7, 0, 0, ranks, 0, 0, None)), out_ptr) == -1 and ok("n_ranks"), err()
            # fov_v is the panorama's alone, the window the orthographic lens's alone; 0 is the default of every extent
            assert call(fn, None, C.byref(_good(rt, model=rules.FISHEYE, fov_v=-1.0)), C.byref(opts), out_ptr) == -1 and ok("null context"), err()
            assert call(fn, None, C.byref(_good(rt, fov_h=2 * pi, fov_v=pi)), C.byref(opts), out_ptr) == -1 and ok("null context"), err()
            assert call(fn, None, C.byref(_good(rt, fov_h=0.0, fov_v=0.0, ortho_width=0.0, ortho_height=0.0)), C.byref(opts), out_ptr) == -1 and ok("null context"), err()
            if base in ("rtk_lens_rays", "rtk_lens_render"):
                assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr, first=-1) == -1 and ok("first_sample"), err()
            if base == "rtk_lens_render":
                assert call(fn, None, C.byref(_good(rt, cam_samples_per_pixel=0)), C.byref(opts), out_ptr) == -1 and ok("samples_per_pixel"), err()
                big = _good(rt, cam_image_width=65536, cam_image_height=65536, cam_samples_per_pixel=1)
                assert call(fn, None, C.byref(big), C.byref(opts), out_ptr) == -1 and ok("2^31"), err()
            else:
                assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr, n=-1) == -1 and ok("n_samples"), err()
                big = _good(rt, cam_image_width=32768, cam_image_height=32768)
                assert call(fn, None, C.byref(big), C.byref(opts), out_ptr, n=2) == -1 and ok("2^31"), err()           # 2^31 records
                assert call(fn, None, C.byref(big), C.byref(opts), out_ptr, n=1) == -1 and ok("null context"), err()   # 2^30: fine
                if base == "rtk_lens_rays":
                    assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr, n=0) == -1 and ok("null context"), err()
                else:
                    assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr, n=0) == -1 and ok("n_samples"), err()
            if base == "rtk_lens_guides":
                assert fn(None, C.byref(_good(rt)), C.byref(opts), 3, C.byref(rt.GuideOpts(4, 0)), out_ptr) == -1 and err().startswith(name + ":"), err()
                assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr, n=2 ** 20 + 1) == -1 and ok("n_samples"), err()
            if not host:                                          # alignment: 8 for records and F64 reals, 4 for F32 reals and se, 16 for guides
                f32 = rt.RenderOpts(7, 1, 0, 1, 0, 0, None)
                if base == "rtk_lens_rays":
                    assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr + 4) == -1 and ok("d_rays") and "aligned" in err(), err()
                elif base == "rtk_lens_render":
                    assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr + 4) == -1 and ok("d_linear") and "aligned" in err(), err()
                    assert call(fn, None, C.byref(_good(rt)), C.byref(f32), out_ptr + 4) == -1 and ok("null context"), err()
                    assert fn(None, C.byref(_good(rt)), C.byref(opts), 0, out_ptr, out_ptr + 2) == -1 and ok("d_noise") and "aligned" in err(), err()
                else:
                    word = "d_aov" if base == "rtk_lens_aovs" else "d_guides"
                    for off in (4, 8):
                        assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr + off) == -1 and ok(word) and "16-byte" in err(), err()
            assert call(fn, None, C.byref(_good(rt)), C.byref(opts), out_ptr) == -1 and ok("null context"), err()
    assert lib.rtk_lens_look_at(None, V(0, 0, 0), V(0, 0, -1), V(0, 1, 0)) == -1 and "rtk_lens_look_at" in err()
    assert np.all(out == 0x5A)


def test_look_at_is_derive_cameras_frame(rt):
    """rtk_lens_look_at against (a) the restatement of Camera.txt:147-149 in numpy, every bit of center, u, v, w; (b) derive_camera
    itself for the same lookfrom, lookat and vup: its defocus_disk_u / _v are u and v times the defocus radius focus_dist *
    tan(radians(defocus_angle / 2)) (Camera.txt:167-169), one rounding each -- the same product of the lens's u and v has the same
    bits -- and with focus_dist = 1 its viewport corner holds w: pixel00_loc and the deltas are recomputed from u, v, w in the
    reference's order and compared bit for bit."""
    views = [((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0)),
             ((0.3, -1.7, 2.9), (4.1, 0.2, -0.6), (0.1, 0.9, -0.2)), ((1.0, 4.0, -10.0), (0.0, 1.0, 5.0), (0.0, 0.0, 1.0))]
    for lookfrom, lookat, vup in views:
        lens = rt.derive_lens(rt.LENS_EQUIRECT, 8, 8, lookfrom=lookfrom, lookat=lookat, vup=vup)
        c, u, v, w = rules.look_at(lookfrom, lookat, vup)
        for got, want in ((lens.cam.center, c), (lens.u, u), (lens.v, v), (lens.w, w)):
            assert _same_bits(_v3(got), want), (lookfrom, _v3(got), want)
        assert abs(np.dot(u, v)) < 4 * U64 and abs(np.dot(u, w)) < 4 * U64 and abs(np.linalg.norm(w) - 1.0) < 4 * U64
        angle, focus, width, aspect, vfov = 2.0, 1.0, 40, 1.6, 70.0
        cam = rt.derive_camera(width, aspect, vfov=vfov, lookfrom=lookfrom, lookat=lookat, vup=vup, defocus_angle=angle, focus_dist=focus)
        radius = focus * math.tan((angle / 2) * 3.1415926535897932385 / 180.0)
        assert _same_bits(_v3(cam.defocus_disk_u), _v3(lens.u) * radius) and _same_bits(_v3(cam.defocus_disk_v), _v3(lens.v) * radius)
        height = int(width / aspect)
        vh = 2 * math.tan((vfov * 3.1415926535897932385 / 180.0) / 2) * focus
        vw = vh * (float(width) / height)
        vu, vv = vw * _v3(lens.u), vh * -_v3(lens.v)
        du, dv = (1 / width) * vu, (1 / height) * vv
        corner = _v3(lens.cam.center) - (focus * _v3(lens.w)) - (1 / 2) * vu - (1 / 2) * vv
        assert _same_bits(_v3(cam.pixel_delta_u), du) and _same_bits(_v3(cam.pixel_delta_v), dv)
        assert _same_bits(_v3(cam.pixel00_loc), corner + 0.5 * (du + dv)) and _same_bits(_v3(cam.center), _v3(lens.cam.center))


def _centre_seeds(orc, width, height):
    """Seeds below 2^20 whose stream for the centre pixel of a width x height frame, sample 0, starts with two draws of exactly 0.5
    (oy = ox = 0): the restated generator, checked against the oracle's on a few streams."""
    pixel = (height // 2) * width + width // 2
    for seed, px, sample in ((1, 0, 0), (SEED, pixel, 0), (2 ** 20 - 1, 77, 9)):
        state, want = rules.stream_key(seed, px, sample), orc.rng_stream(seed, px, sample, 4)
        for k in range(4):
            state, d = rules.draw(state)
            assert d == want[k], (seed, px, sample, k)
    seeds = np.arange(2 ** 20, dtype=np.uint64)
    state, oy = rules.draw(rules.stream_key(seeds, pixel, 0))
    _, ox = rules.draw(state)
    return seeds[(oy == 0.5) & (ox == 0.5)]


def test_no_seed_centres_the_jitter(orc):
    """The r == 0 branch of the fisheye needs a sample whose two jitter draws are exactly 0.5 at the centre pixel of an odd frame.
    Each draw is one of 2^24 values, so a seed does it with probability 2^-48: none of the first 2^20 does, for either odd shape
    tried.  The branch is therefore reached on the device by no test; the restatement takes it with a forced jitter below, and the
    device code is the two-line `if (rr != 0.0)` of lens_local."""
    for width, height in ((19, 11), (9, 7)):
        assert len(_centre_seeds(orc, width, height)) == 0
    rec = rules.film_records(rules.FISHEYE, 19, 11, 1, 0, 1, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), np.pi / 2, np.pi / 2, jitter=(0.0, 0.0))
    centre = (11 // 2) * 19 + 19 // 2
    assert rec["x"][centre] == 0.0 and rec["y"][centre] == 0.0 and np.array_equal(rec["direction"][centre], [0.0, 0.0, -1.0])
    assert np.isfinite(rec["direction"]).all()


# ------------------------------------------------------------------------------------------------------------- GPU --
@pytest.fixture(scope="module")
def scenes(rt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rt.Scene.build(name, SCENE_SEED, scene_file(name, GOLDEN))
        return cache[name]
    return get


def _upload(renderer, scene, order, eye):
    if order == "fast":
        renderer.upload_fast(scene, eye)
    else:
        renderer.upload(scene)


# The bound of test 3 on |device - numpy| per direction component, in units of 2^-53 = U.  Film coordinates, lon, lat, r, theta,
# x / r and yy / r are IEEE +, -, *, /, sqrt of the same operands in the same order on both sides (contraction off): the same bits.
# The device's sin and cos and numpy's are each within one ulp of a value of magnitude at most 1, so within U of the true value
# and within 2 U of each other (as tests/test_light_probes.py test 1 takes them).  A product of two values of magnitude <= 1
# rounds within U / 2 on either side: U between the sides.  A sum of magnitude <= 2 rounds within U on either side: 2 U.
#   EQUIRECT  lx = c * sin(lon): |c| 2 U + |sin| 2 U + U = 5 U;  ly = sin(lat): 2 U;  lz = -(c * cos(lon)): 5 U.
#   FISHEYE   lx = sin(theta) * (x / r): 2 U + U = 3 U;  ly likewise 3 U;  lz = -cos(theta): 2 U.
#   world     (lx u_k + ly v_k) + lz w_k with |u_k|, |v_k|, |w_k| <= 1 (an orthonormal frame): the local errors, then three
#             products (3 U) and two sums (4 U): 12 + 7 = 19 U for EQUIRECT, 8 + 7 = 15 U for FISHEYE.
#   ORTHOGRAPHIC  the local direction is (0, 0, -1) and the origin (center + (x hw) u) + (y hh) v: IEEE operations only.  0.
DIRECTION_BOUND = {rules.EQUIRECT: 19, rules.FISHEYE: 15, rules.ORTHOGRAPHIC: 0}


@pytest.mark.gpu
def test_emitted_rays_are_the_restatement(rt):
    """Needs no scene.  The three film models on both shapes, three views, both real modes (the record is double in both):
    pixel, sample, skip == 3, reserved, time, tmin, tmax and every origin exactly -- an EQUIRECT or FISHEYE origin is cam.center,
    an ORTHOGRAPHIC one is made of IEEE operations alone --; directions within DIRECTION_BOUND (derived above from the operation
    count, not fitted).  The r == 0 branch of the fisheye is reached by no seed (test_no_seed_centres_the_jitter).
    Observed on the MI355X: 2.000 units of 2^-53 for EQUIRECT and FISHEYE, 0 for ORTHOGRAPHIC (DESIGN.md "lens models")."""
    r = rt.Renderer(0)                                            # a context without a scene
    worst = {m: 0.0 for m in MODELS}
    for name in ("three_spheres", "material_zoo", "cornell_box"):
        for model in MODELS:
            for width, height, first, explicit in SHAPES:
                lens = _lens(rt, model, name, width, height, S, 5, (0.1, 0.2, 0.3), explicit)
                frame = np.stack([_v3(lens.u), _v3(lens.v), _v3(lens.w)])
                assert np.abs(frame).max() <= 1.0 + 4 * U64
                want = _restated(lens, S, first, SEED)
                for real_mode in (0, 1):
                    got = r.lens_rays(lens, S, first_sample=first, seed=SEED, real_mode=real_mode)
                    assert got.shape == (width * height * S,) and got.dtype == rt.ray_dtype()
                    assert np.array_equal(got["pixel"], want["pixel"]) and np.array_equal(got["sample"], want["sample"])
                    assert np.all(got["skip"] == 3) and not got["reserved"].any()
                    assert np.array_equal(got["time"], want["time"]) and np.all(got["tmin"] == 0.001) and np.all(got["tmax"] == np.inf)
                    assert _same_bits(got["origin"], want["origin"]), (name, model)
                    err = float(np.abs(got["direction"] - want["direction"]).max())
                    bound = DIRECTION_BOUND[model] * U64
                    worst[model] = max(worst[model], err / U64)
                    assert err <= bound, (name, MODEL_NAMES[model], width, err / U64)
                if model != rules.ORTHOGRAPHIC:
                    assert np.abs(np.linalg.norm(got["direction"], axis=1) - 1.0).max() < 64 * U64
                else:
                    assert len(np.unique(got["origin"], axis=0)) == len(got) and len(np.unique(got["direction"], axis=0)) == 1
    print("emitted rays: worst |direction - numpy| in units of 2^-53: " + ", ".join(f"{MODEL_NAMES[m]} {worst[m]:.3f} (bound {DIRECTION_BOUND[m]})" for m in MODELS))
    assert len(r.lens_rays(_lens(rt, rules.FISHEYE, "three_spheres", 19, 11, S, 5, (0, 0, 0)), 0)) == 0
    r.close()


def _all_pixel_samples(width, height, samples, first):
    return np.array([[p % width, p // width, first + s] for p in range(width * height) for s in range(samples)], np.int32)


@pytest.mark.gpu
@MODES
def test_the_perspective_lens_is_get_ray(rt, renderer, scenes, real_mode):
    """book1_final's camera (a thin lens: the rejection loop runs and skip varies), both shapes: lens_rays equals camera_rays for
    the same camera, seed and samples, every bit of every field; lens_aovs equals aovs and lens_guides the mirror-following guides,
    bit for bit, in both orders."""
    name = "book1_final"
    scene = scenes(name)
    depth = CASES[name][4]
    for width, height, first, _ in SHAPES:
        cam = scene.camera(width, height, S, depth)
        lens = rt.derive_lens(cam=cam)
        got = renderer.lens_rays(lens, S, first_sample=first, seed=SEED, real_mode=real_mode)
        want = renderer.camera_rays(cam, SEED, _all_pixel_samples(width, height, S, first), real_mode)
        assert got.dtype == want.dtype and _same_bits(got, want), [f for f in got.dtype.names if not _same_bits(got[f], want[f])]
        assert len(set(got["skip"].tolist())) > 1
        for order in ORDERS:
            _upload(renderer, scene, order, cam.center)
            assert _same_bits(renderer.lens_aovs(lens, S, seed=SEED, real_mode=real_mode), renderer.aovs(cam, S, seed=SEED, real_mode=real_mode)), (order, width)
            guides = renderer.guides(cam, S, follow=rt.GUIDE_FOLLOW_MIRROR, seed=SEED, real_mode=real_mode)
            assert _same_bits(renderer.lens_guides(lens, S, follow=rt.GUIDE_FOLLOW_MIRROR, seed=SEED, real_mode=real_mode), guides), (order, width)
            assert guides[..., 3].any() and not _same_bits(guides[..., 0:8], guides[..., 8:16])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["book1_final", "three_spheres", "cornell_box"])
def test_the_perspective_frame_is_the_render(rt, renderer, scenes, name):
    """lens_render of the perspective lens at S = 1 equals render_host at spp = 1 under F64_BOUND, the rule of
    test_radiance_of_the_camera_rays_is_the_frame (tests/test_ray_query.py), in both orders and on both shapes."""
    from tests.test_ray_query import F64_BOUND

    scene = scenes(name)
    depth = CASES[name][4]
    for width, height, _, _ in SHAPES:
        cam = scene.camera(width, height, 1, depth)
        lens = rt.derive_lens(cam=cam)
        for order in ORDERS:
            _upload(renderer, scene, order, cam.center)
            frame, _, _ = renderer.render_host(cam, seed=SEED)
            got, se = renderer.lens_render(lens, seed=SEED)
            err = np.abs(got - frame) / np.maximum(1.0, np.abs(frame))
            print(f"{name} {order} {width}x{height}: worst |lens frame - render| / max(1, |render|) = {err.max():.3e}")
            assert frame.any() and err.max() <= F64_BOUND, (order, float(err.max()))
            assert not se.any()                                   # S < 2: no estimate


def _composed(rt, renderer, lens, first, real_mode, depth, background, seed=SEED):
    """(frame [H][W][3] as float64, se [H][W] float64, per-sample radiance [pixels][S][3], records): lens_rays, then one
    single-sample radiance query per record, summed in sample order in the mode's type and scaled once."""
    real = np.float64 if real_mode == 0 else np.float32
    n = lens.cam.samples_per_pixel
    records = renderer.lens_rays(lens, n, first_sample=first, seed=seed, real_mode=real_mode)
    radiance = renderer.query_radiance(records, max_depth=depth, background=background, samples=1, seed=seed, real_mode=real_mode)
    per_sample = radiance.reshape(-1, n, 3)
    total = np.zeros((per_sample.shape[0], 3), real)
    for s in range(n):
        total = total + per_sample[:, s].astype(real)
    frame = (total * real(lens.cam.pixel_samples_scale)).astype(np.float64).reshape(lens.cam.image_height, lens.cam.image_width, 3)
    return frame, rules.standard_error(per_sample).reshape(lens.cam.image_height, lens.cam.image_width), per_sample, records


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", ["three_spheres", "cornell_box", "single_fog", "material_zoo"])
def test_the_frame_is_the_query_over_its_rays(rt, renderer, scenes, name, real_mode):
    """Each film model, both shapes (first_sample 0 and 5), both visiting orders: lens_render equals the sum, in sample order and
    in the mode's type, of query_radiance(lens_rays(...), samples = 1) times the scale, BIT FOR BIT -- the kernels share
    lens_begin and the path loop, and contraction is off; single_fog's medium draws continue the stream past skip -- and se is
    the restatement's in double within one float ulp.  In F64 the two orders give the same bits."""
    scene = scenes(name)
    depth = CASES[name][4]
    bg = scene.camera(8, 8, 1, depth).background
    for model in MODELS:
        for width, height, first, explicit in SHAPES:
            lens = _lens(rt, model, name, width, height, S, depth, bg, explicit)
            frames = {}
            for order in ORDERS:
                _upload(renderer, scene, order, lens.cam.center)
                got, se = renderer.lens_render(lens, first_sample=first, seed=SEED, real_mode=real_mode)
                want, want_se, per_sample, _ = _composed(rt, renderer, lens, first, real_mode, depth, bg)
                differ = np.argwhere(got != want)
                assert _same_bits(got, want), (MODEL_NAMES[model], order, width, len(differ), differ[:4].tolist())
                assert np.isfinite(got).all() and got.any() and per_sample.shape[1] == S
                assert np.all(np.abs(se.astype(np.float64) - want_se) <= _ulp32(want_se)), (MODEL_NAMES[model], order, float(np.abs(se - want_se).max()))
                frames[order] = got
            if real_mode == rt.RTK_REAL_F64:
                assert _same_bits(frames["reference"], frames["fast"]), (MODEL_NAMES[model], width)
    assert se.any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_spheres", "cornell_box", "single_fog", "material_zoo"])
def test_the_frame_is_the_oracles_ray_color(rt, orc, renderer, scenes, name):
    """F64, each film model on both shapes, both orders: the frame against the ORACLE's ray_color over the downloaded records
    (oracle/rt_oracle.cpp, one sample per record), summed in sample order and scaled alike:
    |got - want| <= scale * sum_s F64_BOUND max(1, |L_s|) per channel -- each L_s of the device may differ from the oracle's by the
    F64 bound of the radiance query (tests/test_ray_query.py), and the sum and the scale add roundings far below it."""
    from tests.test_ray_query import F64_BOUND

    scene = scenes(name)
    depth = CASES[name][4]
    bg = scene.camera(8, 8, 1, depth).background
    worst = 0.0
    for model in MODELS:
        for width, height, first, explicit in SHAPES:
            lens = _lens(rt, model, name, width, height, S, depth, bg, explicit)
            records = renderer.lens_rays(lens, S, first_sample=first, seed=SEED)
            radiance, _ = orc.ray_color(scene.desc_ptr, records, max_depth=depth, background=bg, samples=1, seed=SEED)
            per_sample = radiance.reshape(-1, S, 3)
            want = ((per_sample[:, 0] + per_sample[:, 1]) + per_sample[:, 2]) * lens.cam.pixel_samples_scale
            bound = lens.cam.pixel_samples_scale * (F64_BOUND * np.maximum(1.0, np.abs(per_sample))).sum(1)
            for order in ORDERS:
                _upload(renderer, scene, order, lens.cam.center)
                got, _ = renderer.lens_render(lens, first_sample=first, seed=SEED)
                err = np.abs(got.reshape(-1, 3) - want)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (MODEL_NAMES[model], order, width, float((err / bound).max()))
            assert want.any()
    print(f"{name}: worst |lens frame - oracle| / bound = {worst:.4f}")


def _hit_sums(rt, renderer, scene, lens, n, real_mode, seed=SEED):
    """What rtk_lens_aovs accumulates per pixel from rtk_query_hits over the lens's records rekeyed to sample + 2^31, skip 0:
    (hit fraction, summed normal / n, depth, per-record hits, records), each as the float the kernel writes (HitSums: sums in the
    mode's type in sample order, divided once)."""
    from tests.desc_builder import MAT_ISOTROPIC, SceneDesc

    real = np.float64 if real_mode == 0 else np.float32
    records = renderer.lens_rays(lens, n, seed=seed, real_mode=real_mode)
    rekeyed = records.copy()
    rekeyed["sample"] = records["sample"] + np.uint32(2 ** 31)
    rekeyed["skip"] = 0
    hits = renderer.query_hits(rekeyed, seed=seed, real_mode=real_mode)
    desc = C.cast(C.c_void_p(scene.desc_ptr), C.POINTER(SceneDesc)).contents
    kinds = np.array([desc.materials[k].kind for k in range(desc.n_materials)])
    hit = hits["hit"].reshape(-1, n) != 0
    surface = hit & (kinds[np.maximum(hits["material"], 0)].reshape(-1, n) != MAT_ISOTROPIC)
    d = records["direction"].astype(real)
    length = hits["t"].astype(real) * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    normal = hits["normal"].astype(real).reshape(-1, n, 3)
    length = length.reshape(-1, n)
    count, nsum, lsum = np.zeros(hit.shape[0], real), np.zeros((hit.shape[0], 3), real), np.zeros(hit.shape[0], real)
    for s in range(n):
        count = count + hit[:, s].astype(real)
        nsum = nsum + np.where(surface[:, s, None], normal[:, s], real(0))
        lsum = lsum + np.where(hit[:, s], length[:, s], real(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.where(count > 0, lsum / np.where(count > 0, count, real(1)), real(0))
    return (count / real(n)).astype(np.float32), (nsum / real(n)).astype(np.float32), depth.astype(np.float32), hits, records, desc


def _within_an_ulp(got, want):
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= _ulp32(want))


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", ["single_fog", "three_spheres", "cornell_box"])
def test_aovs_are_the_hits_of_the_lens_rays(rt, renderer, scenes, name, real_mode):
    """Each film model on both shapes, both orders: hit fraction, summed normal and depth of lens_aovs equal what query_hits
    gives over the lens's records rekeyed to sample + 2^31, skip 0, accumulated as HitSums does, within one float ulp
    (single_fog: isotropic hits count and add a zero normal).  three_spheres (solid colours): the albedo from hit.material and
    the description's material table.  cornell_box, lens inside: the box is open on the side its own camera looks in through, so
    the full panorama has misses; a panorama whose extent leaves the opening out has hit fraction 1 at every pixel.  The
    first eight floats of lens_guides are the AOVs, bit for bit."""
    from tests.desc_builder import MAT_DIELECTRIC, MAT_LAMBERTIAN, MAT_METAL, TEX_SOLID

    scene = scenes(name)
    depth = CASES[name][4]
    bg = scene.camera(8, 8, 1, depth).background
    real = np.float64 if real_mode == 0 else np.float32
    medium_hits = 0
    for model in MODELS:
        for width, height, _, explicit in SHAPES:
            lens = _lens(rt, model, name, width, height, S, depth, bg, explicit)
            for order in ORDERS:
                _upload(renderer, scene, order, lens.cam.center)
                aov = renderer.lens_aovs(lens, S, seed=SEED, real_mode=real_mode).reshape(-1, 8)
                fraction, normal, dist, hits, records, desc = _hit_sums(rt, renderer, scene, lens, S, real_mode)
                assert _within_an_ulp(aov[:, 3], fraction) and _within_an_ulp(aov[:, 4:7], normal) and _within_an_ulp(aov[:, 7], dist), (MODEL_NAMES[model], order, width)
                assert np.isfinite(aov).all() and aov[:, 3].any()
                guides = renderer.lens_guides(lens, S, seed=SEED, real_mode=real_mode).reshape(-1, 16)
                assert _same_bits(guides[:, 0:8], aov), (MODEL_NAMES[model], order, width)
                medium_hits += int((hits["prim_kind"][hits["hit"] != 0] == rt.NODE_MEDIUM).sum())
                if name == "cornell_box" and model == rules.EQUIRECT:
                    # The box is open towards z < 0 (scene_library.h: five walls), so the full panorama sees the background
                    # through the opening; a panorama of 3 rad < pi about +z from z = 60 cannot reach it: every ray hits.
                    assert (aov[:, 3] < 1.0).any() and (aov[:, 3] == 1.0).any()
                    inward = rt.derive_lens(model, width, height, spp=S, max_depth=depth, lookfrom=(278.0, 278.0, 60.0), lookat=(278.0, 278.0, 555.0),
                                            background=bg, fov_h=3.0)
                    closed = renderer.lens_aovs(inward, S, seed=SEED, real_mode=real_mode)
                    assert np.all(closed[..., 3] == 1.0), (order, width, float(closed[..., 3].min()))
                if name == "three_spheres":
                    colour = np.zeros((len(hits), 3), real)
                    miss = np.clip(np.array([bg.x, bg.y, bg.z]).astype(real), real(0), real(1))
                    for k, h in enumerate(hits):
                        if not h["hit"]:
                            colour[k] = miss
                            continue
                        m = desc.materials[int(h["material"])]
                        if m.kind == MAT_LAMBERTIAN:
                            t = desc.textures[m.texture]
                            assert t.kind == TEX_SOLID
                            colour[k] = np.array([t.color.x, t.color.y, t.color.z]).astype(real)
                        elif m.kind == MAT_METAL:
                            colour[k] = np.array([m.albedo.x, m.albedo.y, m.albedo.z]).astype(real)
                        else:
                            assert m.kind == MAT_DIELECTRIC
                            colour[k] = 1
                    colour = colour.reshape(-1, S, 3)
                    total = np.zeros((colour.shape[0], 3), real)
                    for s in range(S):
                        total = total + colour[:, s]
                    assert _within_an_ulp(aov[:, 0:3], (total / real(S)).astype(np.float32)), (MODEL_NAMES[model], order, width)
                    if model == rules.EQUIRECT:
                        assert len({int(m) for m in hits["material"] if m >= 0}) >= 3
    assert (medium_hits > 0) == (name == "single_fog")


def _carved(torch, dev, nbytes, residue):
    """(buffer, offset): nbytes at an address = residue mod 16 inside a poisoned allocation, 64 guard bytes on either side."""
    buf = torch.full((nbytes + 160,), 0xA5, dtype=torch.uint8, device=dev)
    off = 64 + (residue - (buf.data_ptr() + 64)) % 16
    return buf, off


def _guards_intact(buf, off, nbytes):
    host = buf.cpu().numpy()
    return bool((host[:off] == 0xA5).all() and (host[off + nbytes:] == 0xA5).all())


@pytest.mark.gpu
@MODES
def test_continuation_streams_and_carved_buffers(rt, renderer, scenes, real_mode):
    """material_zoo, each film model, 19x11.  A frame of S = 6 equals, bit for bit, the sample-order sum rebuilt from two lens_rays
    batches (first_sample 0 and 3); the same call twice gives the same bits; the four device entry points on a caller stream, writing
    into carved buffers 8 bytes past a 16-byte boundary (records, reals; the se 4 past; guides on it), leave the guard bytes intact and
    give the bits of the _host forms; d_aov and d_guides off a 16-byte boundary are refused with nothing launched or written."""
    import torch

    name = "material_zoo"
    scene = scenes(name)
    depth = CASES[name][4]
    bg = scene.camera(8, 8, 1, depth).background
    real = np.float64 if real_mode == 0 else np.float32
    dev = torch.device("cuda", renderer.device)
    width, height = 19, 11
    px = width * height
    for model in MODELS:
        lens6 = _lens(rt, model, name, width, height, 6, depth, bg)
        lens3 = _lens(rt, model, name, width, height, 3, depth, bg)
        _upload(renderer, scene, "fast", lens6.cam.center)
        got, se = renderer.lens_render(lens6, seed=SEED, real_mode=real_mode)
        again, se_again = renderer.lens_render(lens6, seed=SEED, real_mode=real_mode)
        assert _same_bits(got, again) and _same_bits(se, se_again)
        total = np.zeros((px, 3), real)
        batches = []
        for first in (0, 3):
            records = renderer.lens_rays(lens3, 3, first_sample=first, seed=SEED, real_mode=real_mode)
            assert np.array_equal(records["sample"].reshape(-1, 3), np.tile(np.arange(first, first + 3, dtype=np.uint32), (px, 1)))
            radiance = renderer.query_radiance(records, max_depth=depth, background=bg, samples=1, seed=SEED, real_mode=real_mode).reshape(px, 3, 3)
            batches.append(radiance)
            for s in range(3):
                total = total + radiance[:, s].astype(real)
        want = (total * real(lens6.cam.pixel_samples_scale)).astype(np.float64).reshape(height, width, 3)
        assert _same_bits(got, want), MODEL_NAMES[model]
        want_se = rules.standard_error(np.concatenate(batches, 1))
        assert np.all(np.abs(se.reshape(-1).astype(np.float64) - want_se) <= _ulp32(want_se))
        # ... and a frame that starts at sample 3 is the second batch alone
        late, _ = renderer.lens_render(lens3, first_sample=3, seed=SEED, real_mode=real_mode)
        second = np.zeros((px, 3), real)
        for s in range(3):
            second = second + batches[1][:, s].astype(real)
        assert _same_bits(late, (second * real(lens3.cam.pixel_samples_scale)).astype(np.float64).reshape(height, width, 3))

        stream = torch.cuda.Stream(device=dev)
        real_bytes = 8 if real_mode == 0 else 4
        rays_buf, rays_off = _carved(torch, dev, px * 3 * 88, 8)
        lin_buf, lin_off = _carved(torch, dev, px * 3 * real_bytes, 8)
        se_buf, se_off = _carved(torch, dev, px * 4, 4)
        aov_buf, aov_off = _carved(torch, dev, px * 8 * 4, 0)
        gd_buf, gd_off = _carved(torch, dev, px * 16 * 4, 0)
        before = (aov_buf.cpu().numpy().copy(), gd_buf.cpu().numpy().copy())
        for off in (4, 8):                                        # refused before anything is launched
            with pytest.raises(rt.RtkError, match="d_aov"):
                renderer.lens_aovs_device(lens3, 3, aov_buf.data_ptr() + aov_off + off, seed=SEED, real_mode=real_mode, stream=stream.cuda_stream)
            with pytest.raises(rt.RtkError, match="d_guides"):
                renderer.lens_guides_device(lens3, 3, gd_buf.data_ptr() + gd_off + off, seed=SEED, real_mode=real_mode, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(aov_buf.cpu().numpy(), before[0]) and np.array_equal(gd_buf.cpu().numpy(), before[1])
        renderer.lens_rays_device(lens3, 3, rays_buf.data_ptr() + rays_off, first_sample=3, seed=SEED, real_mode=real_mode, stream=stream.cuda_stream)
        renderer.lens_render_device(lens3, lin_buf.data_ptr() + lin_off, se_buf.data_ptr() + se_off, first_sample=3, seed=SEED, real_mode=real_mode,
                                    stream=stream.cuda_stream)
        renderer.lens_aovs_device(lens3, 3, aov_buf.data_ptr() + aov_off, seed=SEED, real_mode=real_mode, stream=stream.cuda_stream)
        renderer.lens_guides_device(lens3, 3, gd_buf.data_ptr() + gd_off, seed=SEED, real_mode=real_mode, stream=stream.cuda_stream)
        stream.synchronize()
        for buf, off, n in ((rays_buf, rays_off, px * 3 * 88), (lin_buf, lin_off, px * 3 * real_bytes), (se_buf, se_off, px * 4), (aov_buf, aov_off, px * 32),
                            (gd_buf, gd_off, px * 64)):
            assert _guards_intact(buf, off, n)
        carved = lambda buf, off, n, dtype: buf.cpu().numpy()[off:off + n].copy().view(dtype)  # noqa: E731
        assert _same_bits(carved(rays_buf, rays_off, px * 3 * 88, rt.ray_dtype()), renderer.lens_rays(lens3, 3, first_sample=3, seed=SEED, real_mode=real_mode))
        late_host, late_se = renderer.lens_render(lens3, first_sample=3, seed=SEED, real_mode=real_mode)
        assert _same_bits(carved(lin_buf, lin_off, px * 3 * real_bytes, real).astype(np.float64), late_host.reshape(-1))
        assert _same_bits(carved(se_buf, se_off, px * 4, np.float32), late_se.reshape(-1))
        assert _same_bits(carved(aov_buf, aov_off, px * 32, np.float32), renderer.lens_aovs(lens3, 3, seed=SEED, real_mode=real_mode).reshape(-1))
        assert _same_bits(carved(gd_buf, gd_off, px * 64, np.float32), renderer.lens_guides(lens3, 3, seed=SEED, real_mode=real_mode).reshape(-1))
    no_scene = rt.Renderer(0)
    with pytest.raises(rt.RtkError) as e:
        no_scene.lens_render(lens3, seed=SEED)
    assert e.value.code == -5
    no_scene.close()


@pytest.mark.gpu
@MODES
def test_a_light_on_the_right_shows_on_the_right(rt, renderer, real_mode):
    """A black background and one emissive sphere at (2, 0, -3).  From the origin looking down -z (u = +x) it is on the +u side: the
    brightest column of the EQUIRECT, FISHEYE and ORTHOGRAPHIC frames lies in the right half and the brightest row in the middle
    third (the sphere is at the lens's height: a swapped axis would move it).  From (0, 0, -6) looking down +z, the frame look_at
    gives has u = -x: the brightest column lies in the left half."""
    from tests.desc_builder import DescBuilder

    b = DescBuilder()
    built = b.finish(b.list([b.sphere((2.0, 0.0, -3.0), 0.8, b.light((4.0, 4.0, 4.0)))]))
    renderer.upload(built)
    width, height = 24, 16
    for model in MODELS:
        columns = []
        for lookfrom, lookat in (((0.0, 0.0, 0.0), (0.0, 0.0, -1.0)), ((0.0, 0.0, -6.0), (0.0, 0.0, -3.0))):
            lens = rt.derive_lens(model, width, height, spp=S, max_depth=2, lookfrom=lookfrom, lookat=lookat, background=(0.0, 0.0, 0.0),
                                  fov_h=(2.0 * math.pi if model == rules.FISHEYE else 0.0), ortho_width=8.0, ortho_height=6.0)
            frame, _ = renderer.lens_render(lens, seed=SEED, real_mode=real_mode)
            assert frame.max() > 1.0 and (frame == 0).any()
            columns.append(int(frame.sum((0, 2)).argmax()))
            row = int(frame.sum((1, 2)).argmax())
            assert height // 3 <= row < height - height // 3, (MODEL_NAMES[model], row)
        assert _v3(lens.u)[0] == -1.0
        print(f"{MODEL_NAMES[model]}: brightest column {columns[0]} from the front, {columns[1]} from behind (of {width})")
        assert columns[0] >= width // 2 and columns[1] < width // 2, (MODEL_NAMES[model], columns)


@pytest.mark.gpu
@MODES
def test_the_cameras_projection(rt, renderer, scenes, real_mode, tmp_path):
    """camera::projection = equirect: render() writes the PNG that rtk_lens_render_host and the resolve's gamma give, byte for byte;
    temporal_history or render_scale with that projection make render() fail with a message and write nothing."""
    from tests.test_denoise import _read_png, _to_byte

    exe = str(tmp_path / "lens_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "helpers", "lens_camera_check.cpp"),
                           "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lrtk_hip", "-Wl,-rpath," + PKG, "-o", exe])
    name = "three_spheres"
    scene = scenes(name)
    depth = scene.camera(0, 0, 0, 0).max_depth                    # the scene's own depth, as the helper takes it
    bg = scene.camera(0, 0, 0, 0).background
    out, refused = str(tmp_path / "lens.png"), str(tmp_path / "refused.png")
    p = subprocess.run([exe, name, scene_file(name, GOLDEN), out, refused, str(real_mode)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "lens_camera_check: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stderr.count("camera::render failed") == 2 and "temporal_history" in p.stderr and "perspective" in p.stderr, p.stderr[-2000:]
    assert not os.path.exists(refused)
    lens = rt.derive_lens(rt.LENS_EQUIRECT, 24, 16, spp=3, max_depth=depth, lookfrom=(0.0, 0.25, 0.5), lookat=(0.0, 0.0, -1.0), background=bg, fov_h=4.0, fov_v=2.0)
    renderer.upload(scene)                                        # the reference order, as the helper asks for
    linear, _ = renderer.lens_render(lens, seed=5, real_mode=real_mode)
    png = _read_png(out)
    assert png.shape == (16, 24, 3) and np.array_equal(png, _to_byte(linear)) and len(np.unique(png)) > 8
