"""Surface gathers (include/rtk.h "Surface gathers"): irradiance and occlusion at points with normals, the rays made on the
device, a point's rays cut into passes of 64 over separate waves and added in order by a second stage.

The conventions -- the cosine-weighted Fibonacci set, each point's rotation, the frame, the records -- are restated in numpy in
tests/gather_rules.py, from the header's text alone.

CPU tests: the conventions against figures computed from the rule; the six entry points declared and exported with
RTK_ABI_VERSION 2; the ctypes structure laid out as a C compiler lays out the header's; every refusal RTK_ERR_INVALID naming its
entry point and argument, with no device and no context; stage 1 of the irradiance gather with no more scratch and no fewer waves
per SIMD than the radiance query of its mode (code-object metadata).

GPU tests, in both visiting orders and both real modes unless they read no scene:
  1. the emitted rays are the restatement's (integers, origin, time, tmin, tmax exactly; directions within 14 * 2^-53);
  2. irradiance is the radiance query over those rays, projected, within the classical summation bound; in F64 also the oracle's
     ray_color over them;
  3. occlusion: the open count is the occlusion query's (and, in F64, the oracle's) exactly, the bent normal the numpy sum;
  4. edges: depth 0, a point's place in the batch, batch_points, the 32-bit wrap of the key, rotation, R = 16384, repeatability;
  5. a point that sees only sky; 6. carved, offset buffers with guard bytes on a caller stream; misaligned pointers, no scene;
  7. rtk::surface_gather of the host C++ API (tests/helpers/surface_gather_check.cpp) and rt.quad_texels.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gather_rules as rules
from tests.conftest import GOLDEN, ROOT
from tests.scene_cases import IMAGE_CASES, SCENE_SEED, scene_file

PKG = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
ENTRY_POINTS = ("rtk_gather_rays", "rtk_gather_irradiance", "rtk_gather_occlusion", "rtk_gather_rays_host", "rtk_gather_irradiance_host",
                "rtk_gather_occlusion_host")
CASES = {c[0]: c for c in IMAGE_CASES}
SCENES = ["three_spheres", "cornell_box", "cornell_smoke", "material_zoo"]
ORDERS = ("reference", "fast")
MODES = pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
U64, U32 = 2.0 ** -53, 2.0 ** -24
SEED = 5
# |x - x'|, |y - y'| <= 4 * 2^-53 for the local direction, as tests/test_light_probes.py derives it (sin and cos within one ulp of
# a value at most 1 on either side, one rounding of the product on either side); r, z, phi, t, bt and n are correctly rounded
# operations on the same operands and agree exactly.  Through d_c = x t_c + y bt_c + z n_c with |t_c|, |bt_c| <= 1: 4 + 4 from x
# and y, 2 for the two products' roundings on both sides (2^-54 each: the products are below 1), 4 for the two sums' roundings
# on both sides (2^-53 each: the sums are below 2); z n_c is the same product on both sides.
DIRECTION_BOUND = 14 * U64


# ------------------------------------------------------------------------------------------------------------- CPU --
def test_conventions_in_numpy():
    """The rule against figures computed from it (R: worst |mean d - (0, 0, 2/3)|, worst |mean d d^T - diag(1/4, 1/4, 1/2)| over
    rot in {0, 123456789, 4000000000}: 64: 8.7e-3, 5.7e-3; 256: 2.0e-3, 1.3e-3; 1024: 5.2e-4, 3.6e-4; 16384: 3.3e-5, 2.3e-5),
    with a quarter of headroom; min z > 0; |d|^2 - 1 <= 4 * 2^-52; the frame orthonormal to 2e-15 and right-handed."""
    figures = {64: (8.7e-3, 5.7e-3), 256: (2.0e-3, 1.3e-3), 1024: (5.2e-4, 3.6e-4), 16384: (3.3e-5, 2.3e-5)}
    for rays, (first, second) in figures.items():
        worst1 = worst2 = 0.0
        for rot in (0, 123456789, 4000000000):
            d = rules.local_directions(rays, rot)
            assert d[:, 2].min() > 0 and np.abs((d * d).sum(1) - 1.0).max() <= 4 * 2.0 ** -52
            worst1 = max(worst1, float(np.abs(d.mean(0) - [0.0, 0.0, 2.0 / 3.0]).max()))
            worst2 = max(worst2, float(np.abs(d.T @ d / rays - np.diag([0.25, 0.25, 0.5])).max()))
        print(f"R = {rays}: first moment {worst1:.2e}, second moment {worst2:.2e}")
        assert worst1 <= 1.25 * first and worst2 <= 1.25 * second, (rays, worst1, worst2)
    assert rules.rotation(2 ** 32 - 1, 1, 1) == 0 and rules.rotation(0, 3, 0) == 0 and rules.rotation(1, 1, 1) == (2 * 0x85EBCA6B) % 2 ** 32
    v = np.random.default_rng(3).standard_normal((2000, 3))
    normals = list(v / np.linalg.norm(v, axis=1, keepdims=True))
    normals += [np.array(a) for a in ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (-0.0, -0.0, 1.0), (1.0, 0.0, 0.0), (1.0, 0.0, -0.0), (0.0, -1.0, 0.0), (0.6, 0.8, -0.0))]
    worst = 0.0
    for n in normals:
        t, bt = rules.frame(n)
        m = np.stack([t, bt, n])
        worst = max(worst, float(np.abs(m @ m.T - np.eye(3)).max()))
        assert np.linalg.det(m) > 0, n
    print("frame: worst |Gram - identity| = %.2e" % worst)
    assert worst <= 2e-15
    t, bt = rules.frame(np.array([0.0, 0.0, -1.0]))                # the case the older frame could not do
    assert np.array_equal(t, [1.0, 0.0, 0.0]) and np.array_equal(bt, [0.0, -1.0, 0.0])
    d = rules.world_directions(64, 0, np.array([0.0, 0.0, 1.0]))   # around +z the world directions are the local ones
    assert np.array_equal(d, rules.local_directions(64, 0))


def test_entry_points_are_declared_and_exported(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    assert "#define RTK_ABI_VERSION 2" in header and "Surface gathers ---" in header and "sizeof(rtk_gather_opts) = 96" in header
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(rtk_ctx\* ctx, const rtk_gather_opts\* opts, int64_t n, " % name, header), name
    lib = C.CDLL(rt.HIP_LIB_PATH)                                 # loads without a GPU
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.rtk_abi_version() == 2
    import __graft_entry__

    assert "rtk_gather.cpp" in __graft_entry__.HIP_SOURCES and "rtk_gather.hip" in __graft_entry__.HIP_SOURCES
    assert "rtk_gather_rule.h" in __graft_entry__.HIP_HEADERS
    for method in ("gather_rays", "gather_irradiance", "gather_occlusion", "gather_rays_device", "gather_irradiance_device", "gather_occlusion_device"):
        assert callable(getattr(rt.Renderer, method)), method
    assert "rtk_surface_gather.h" in open(os.path.join(PKG, "host", "rtk_scene_api.h")).read()
    points, normals = rt.quad_texels((1.0, 2.0, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 2.0), 4, 2)
    assert points.shape == (8, 3) and normals.shape == (8, 3)
    assert np.array_equal(points[0], [1.5, 2.0, 3.5]) and np.array_equal(points[1], [2.5, 2.0, 3.5]) and np.array_equal(points[4], [1.5, 2.0, 4.5])
    assert np.array_equal(normals, np.tile([0.0, -1.0, 0.0], (8, 1)))                  # cross(u, v) = (0, -8, 0)
    with pytest.raises(ValueError):
        rt.quad_texels((1.0, 2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 2.0), 4, 2)
    with pytest.raises(ValueError):
        rt.quad_texels((1.0, 2.0, 3.0), (4.0, 0.0, 0.0), (0.0, 0.0, 2.0), 0, 2)
    for call in (lambda: rt.Renderer.gather_rays(None, np.zeros((2, 2)), np.zeros((2, 3))),
                 lambda: rt.Renderer.gather_irradiance(None, np.zeros((2, 3)), np.zeros((3, 3)), max_depth=1),
                 lambda: rt.Renderer.gather_occlusion(None, np.zeros(3), np.zeros(3))):
        with pytest.raises(ValueError):
            call()


def test_structure_has_the_headers_layout(rt, tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rtk.h"', "int main(void) {", '    printf("size %zu\\n", sizeof(rtk_gather_opts));']
    for field, _ in rt.GatherOpts._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(rtk_gather_opts, %s));' % (field, field))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    assert want["size"] == 96 and C.sizeof(rt.GatherOpts) == 96
    assert {f for f, _ in rt.GatherOpts._fields_} == {"seed", "real_mode", "max_depth", "samples", "rays", "first_key", "rotate", "batch_points", "background", "time",
                                                      "max_distance", "stream", "reserved"}
    for field, _ in rt.GatherOpts._fields_:
        assert getattr(rt.GatherOpts, field).offset == want[field], field


def _opts(rt, **kw):
    o = rt.GatherOpts(7, 0, 5, 1, 64, 0, 0, 0, rt.Vec3(0.5, 0.5, 0.5), 0.0, 0.0, None, (C.c_int32 * 4)(0, 0, 0, 0))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_refusals_need_no_device(rt):
    """Every refusal is RTK_ERR_INVALID with the entry point and the argument named, with a null context: the argument checks
    come before anything that needs a device.  Nothing is written."""
    lib = rt.hip_lib()
    err = lambda: lib.rtk_last_error().decode()  # noqa: E731
    pts, nrm = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    out = np.full(4 * 64 * 88 + 16, 0x5A, np.uint8)                # large enough for the rays of four points
    out_ptr = out.ctypes.data + (-out.ctypes.data) % 8
    reserved = lambda *r: (C.c_int32 * 4)(*r)  # noqa: E731
    bad_opts = [(dict(real_mode=2), "real_mode"), (dict(real_mode=-1), "real_mode"), (dict(max_depth=-1), "max_depth"), (dict(samples=-1), "samples"),
                (dict(reserved=reserved(1, 0, 0, 0)), "reserved"), (dict(reserved=reserved(0, 0, 0, -5)), "reserved"),
                (dict(rays=63), "rays"), (dict(rays=96), "rays"), (dict(rays=16448), "rays"), (dict(rays=-64), "rays"), (dict(rays=32), "rays"),
                (dict(rotate=2), "rotate"), (dict(rotate=-1), "rotate"), (dict(batch_points=-1), "batch_points"), (dict(max_distance=-1.0), "max_distance"),
                (dict(max_distance=float("nan")), "max_distance")]
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        host, occlusion = name.endswith("_host"), "occlusion" in name
        extra = (out_ptr + 2048,) if occlusion else ()
        call = lambda o, n, p, q, r: fn(None, o, n, p, q, r, *extra)  # noqa: E731
        good = C.byref(_opts(rt))
        for fields, word in bad_opts:
            assert call(C.byref(_opts(rt, **fields)), 4, pts.ctypes.data, nrm.ctypes.data, out_ptr) == -1, (name, fields)
            assert word in err() and err().startswith(name + ":"), (name, fields, err())
        assert call(None, 4, pts.ctypes.data, nrm.ctypes.data, out_ptr) == -1 and "null opts" in err() and err().startswith(name + ":")
        assert call(good, -1, pts.ctypes.data, nrm.ctypes.data, out_ptr) == -1 and " n " in err() and err().startswith(name + ":"), err()
        for rays, n in ((64, 2 ** 25), (16384, 2 ** 17), (0, 2 ** 23), (64, 2 ** 40)):     # n * rays = 2^31 (rays 0 = 256) and beyond
            assert call(C.byref(_opts(rt, rays=rays)), n, pts.ctypes.data, nrm.ctypes.data, out_ptr) == -1 and "n * rays" in err(), (name, rays, n, err())
        prefix = "h_" if host else "d_"
        assert call(good, 4, None, nrm.ctypes.data, out_ptr) == -1 and "null " + prefix + "points" in err() and err().startswith(name + ":")
        assert call(good, 4, pts.ctypes.data, None, out_ptr) == -1 and "null " + prefix + "normals" in err() and err().startswith(name + ":")
        if occlusion:                                             # both outputs null; one alone is enough
            assert fn(None, good, 4, pts.ctypes.data, nrm.ctypes.data, None, None) == -1 and prefix + "open" in err() and prefix + "bent" in err() and "null" in err()
            assert fn(None, good, 4, pts.ctypes.data, nrm.ctypes.data, out_ptr, None) == -1 and "null context" in err()
            assert fn(None, good, 4, pts.ctypes.data, nrm.ctypes.data, None, out_ptr) == -1 and "null context" in err()
        else:
            assert call(good, 4, pts.ctypes.data, nrm.ctypes.data, None) == -1 and re.search(r"null [dh]_(rays|irradiance)", err()) and err().startswith(name + ":")
        if not host:
            assert call(good, 4, pts.ctypes.data + 4, nrm.ctypes.data, out_ptr) == -1 and "d_points" in err() and "aligned" in err(), err()
            assert call(good, 4, pts.ctypes.data, nrm.ctypes.data + 4, out_ptr) == -1 and "d_normals" in err() and "aligned" in err(), err()
            assert call(good, 4, pts.ctypes.data, nrm.ctypes.data, out_ptr + 4) == -1 and "aligned" in err() and "d_points" not in err(), err()
            if occlusion:
                assert fn(None, good, 4, pts.ctypes.data, nrm.ctypes.data, out_ptr, out_ptr + 2052) == -1 and "d_bent" in err() and "aligned" in err(), err()
            if name != "rtk_gather_rays":                         # F32 reals need 4 bytes only
                f32 = C.byref(_opts(rt, real_mode=1))
                assert call(f32, 4, pts.ctypes.data, nrm.ctypes.data, out_ptr + 4) == -1 and "null context" in err()
                assert call(f32, 4, pts.ctypes.data, nrm.ctypes.data, out_ptr + 2) == -1 and "aligned" in err()
            # an output that overlaps an input
            assert call(good, 4, pts.ctypes.data, nrm.ctypes.data, pts.ctypes.data + 8) == -1 and "overlaps d_points" in err() and err().startswith(name + ":"), err()
            assert call(good, 4, pts.ctypes.data, nrm.ctypes.data, nrm.ctypes.data) == -1 and "overlaps d_normals" in err(), err()
        for n in (4, 0):
            assert call(good, n, pts.ctypes.data, nrm.ctypes.data, out_ptr) == -1 and "null context" in err() and err().startswith(name + ":"), (name, err())
        big = np.zeros(16384 * 88 + 16, np.uint8)                 # the rays of one point at the largest R
        for rays in (64, 16384, 0):
            assert call(C.byref(_opts(rt, rays=rays, rotate=1, batch_points=3, max_distance=2.5)), 1, pts.ctypes.data, nrm.ctypes.data,
                        big.ctypes.data + (-big.ctypes.data) % 8) == -1 and "null context" in err(), (name, rays, err())
    assert np.all(out == 0x5A) and not pts.any()


def test_stage_one_keeps_the_querys_resources(rt, tmp_path):
    """rtk_gather_irradiance_kernel<real> has no more scratch and no fewer waves per SIMD than rtk_query_radiance_kernel<real,
    false>: nothing of the gather is live across the path loop, and it uses no LDS."""
    from tests.test_light_probes import _kernel_metadata, _waves_per_simd

    meta = _kernel_metadata(rt.HIP_LIB_PATH, tmp_path)
    assert meta is not None, "ROCm's LLVM binary tools (llvm-objcopy, clang-offload-bundler, llvm-readelf) belong to the toolchain that built the library"
    for tag in ("d", "f"):
        gather = [v for k, v in meta.items() if re.search(r"rtk_gather_irradiance_kernelI%sE" % tag, k)]
        query = [v for k, v in meta.items() if re.search(r"rtk_query_radiance_kernelI%sLb0EE" % tag, k)]
        assert len(gather) == 1 and len(query) == 1, sorted(meta)[:8]
        print(tag, "gather", gather[0], _waves_per_simd(gather[0]), "query", query[0], _waves_per_simd(query[0]))
        assert gather[0]["scratch"] <= query[0]["scratch"] and _waves_per_simd(gather[0]) >= _waves_per_simd(query[0]) and gather[0]["lds"] == 0
    assert sum("rtk_gather_occlusion_kernel" in k for k in meta) == 4   # both modes, with and without the early exit


# ------------------------------------------------------------------------------------------------------------- GPU --
@pytest.fixture(scope="module")
def scenes(rt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rt.Scene.build(name, SCENE_SEED, scene_file(name, GOLDEN))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def surface(rt, orc, renderer, scenes):
    """name -> (points, normals), five surface points of the scene: p and normal of the ORACLE's hit records for five camera rays
    of a 16x9 frame -- the first hit of every primitive kind the frame sees (spheres, quads, a medium), then hits spread evenly
    over the rest.  Computed once per scene."""
    cache = {}

    def get(name):
        if name not in cache:
            scene = scenes(name)
            cam = scene.camera(16, 9, 1, 1)
            ijs = np.array([(i, j, 0) for j in range(9) for i in range(16)], np.int32)
            hits = orc.hits(scene.desc_ptr, renderer.camera_rays(cam, SEED, ijs), SEED)
            idx = np.nonzero(hits["hit"] == 1)[0]
            assert len(idx) >= 5, name
            chosen = [int(idx[hits["prim_kind"][idx] == kind][0]) for kind in np.unique(hits["prim_kind"][idx])]
            rest = [int(i) for i in idx if int(i) not in chosen]
            chosen += [rest[(2 * k + 1) * len(rest) // (2 * (5 - len(chosen)))] for k in range(5 - len(chosen))]
            chosen = sorted(chosen[:5])
            points, normals = hits["p"][chosen].copy(), hits["normal"][chosen].copy()
            assert np.abs(np.linalg.norm(normals, axis=1) - 1.0).max() < 1e-12
            cache[name] = (points, normals)
        return cache[name]
    return get


def _upload(renderer, scene, order):
    if order == "fast":
        renderer.upload_fast(scene, scene.camera(8, 8, 1, 1).center)
    else:
        renderer.upload(scene)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _summed(radiance, n, rays, real_mode):
    """(want, bound) of E from L [n * R][3]: (R + 4) 2^-53 (pi / R) sum_j |L_j| -- the classical bound of R - 1 additions in any
    order, plus the scale and the division it is made of -- and 2^-24 |want| for the result's rounding in F32."""
    terms = radiance.reshape(n, rays, 3)
    want = np.pi / rays * terms.sum(1)
    bound = (rays + 4) * U64 * (np.pi / rays) * np.abs(terms).sum(1)
    return want, bound + (U32 * np.abs(want) if real_mode == 1 else 0.0)


def _projected(renderer, points, normals, *, rays, samples, max_depth, background, first_key=0, rotate=0, real_mode=0):
    """(want, bound): the radiance query over the emitted rays, summed in numpy float64."""
    records = renderer.gather_rays(points, normals, rays=rays, samples=samples, first_key=first_key, rotate=rotate)
    radiance = renderer.query_radiance(records, max_depth=max_depth, background=background, samples=samples, seed=SEED, real_mode=real_mode)
    return _summed(radiance, len(points), rays, real_mode)


@pytest.mark.gpu
def test_emitted_rays_are_the_restatement(rt):
    """Needs no scene.  n in {1, 3}, R in {64, 192}, S in {1, 2}, rotate in {0, 1}, first_key = 2^32 - 2, normals that cover both
    signs of n.z: integer fields, origin, time, tmin and tmax exactly, directions within DIRECTION_BOUND = 14 * 2^-53 (derived
    above, not tuned).  Observed on the MI355X: 2.000 * 2^-53."""
    r = rt.Renderer(0)                                            # a context without a scene
    points = np.array([(278.0, 0.0, 278.0), (0.5, 1.25, -3.0), (-2.0, 7.0, 1e3)])
    normals = np.array([(0.0, 1.0, 0.0), (0.6, 0.0, -0.8), (2.0 / 3.0, -1.0 / 3.0, 2.0 / 3.0)])
    worst = 0.0
    for n in (1, 3):
        for rays in (64, 192):
            for samples in (1, 2):
                for rotate in (0, 1):
                    for max_distance in (0.0, 12.5):
                        kw = dict(rays=rays, samples=samples, first_key=2 ** 32 - 2, rotate=rotate, time=0.375, max_distance=max_distance)
                        got = r.gather_rays(points[:n], normals[:n], **kw)
                        want = rules.records(rt.ray_dtype(), points[:n], normals[:n], **kw)
                        assert got.shape == (n * rays,) and got.dtype == rt.ray_dtype()
                        for field in ("origin", "time", "tmin", "tmax", "pixel", "sample", "skip", "reserved"):
                            assert np.array_equal(got[field], want[field]), (field, n, rays, samples, rotate)
                        assert np.all(got["tmax"] == (np.inf if max_distance == 0 else 12.5)) and np.all(got["tmin"] == 0.001)
                        worst = max(worst, float(np.abs(got["direction"] - want["direction"]).max()))
    print("emitted rays: worst |d - numpy| = %.3f * 2^-53" % (worst / U64))
    assert worst <= DIRECTION_BOUND
    one_normal = np.tile(normals[:1], (3, 1))
    rot = r.gather_rays(points, one_normal, rays=64, rotate=1)["direction"].reshape(3, 64, 3)
    same = r.gather_rays(points, one_normal, rays=64, rotate=0)["direction"].reshape(3, 64, 3)
    assert _same_bits(same[0], same[2]) and _same_bits(rot[0], same[0])        # key 0 has rotation 0
    assert not _same_bits(rot[1], same[1]) and not _same_bits(rot[1], rot[2])  # ... every other key its own
    assert len(r.gather_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    r.close()


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", SCENES)
def test_irradiance_is_the_query_projected(rt, renderer, scenes, surface, name, real_mode):
    """n = 5 surface points, R in {64, 192, 256} (5, 15 and 20 units: the last workgroup is partly empty), S in {1, 2}, the
    case's depth, both orders: |got - want| <= (R + 4) 2^-53 (pi / R) sum_j |L_j|, plus 2^-24 |want| in F32, where L is the
    query's of the same mode.  F64 results have the same bits in both orders; S = 1 and S = 2 differ.  Observed on the MI355X:
    worst ratio to the bound 0.17 in F64 and 0.91 in F32, where the final rounding to float is the bound."""
    scene = scenes(name)
    depth = CASES[name][4]
    bg = scene.camera(8, 8, 1, depth).background
    points, normals = surface(name)
    worst, results = 0.0, {}
    for order in ORDERS:
        _upload(renderer, scene, order)
        for rays in (64, 192, 256):
            for samples in (1, 2):
                got = renderer.gather_irradiance(points, normals, max_depth=depth, rays=rays, samples=samples, background=bg, seed=SEED, real_mode=real_mode)
                want, bound = _projected(renderer, points, normals, rays=rays, samples=samples, max_depth=depth, background=bg, real_mode=real_mode)
                assert got.shape == (5, 3) and np.isfinite(got).all() and got.any()
                ratio = np.abs(got - want) / np.where(bound > 0, bound, 1.0)
                worst = max(worst, float(ratio.max()))
                assert np.all(np.abs(got - want) <= bound), (order, rays, samples, float(ratio.max()))
                results[order, rays, samples] = got
    print(f"{name} mode {real_mode}: worst |gather - projected query| / bound = {worst:.3f}")
    if real_mode == rt.RTK_REAL_F64:
        assert all(_same_bits(results["reference", r, s], results["fast", r, s]) for r in (64, 192, 256) for s in (1, 2))
    assert not _same_bits(results["reference", 64, 1], results["reference", 64, 2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_irradiance_is_the_oracle_projected(rt, orc, renderer, scenes, surface, name):
    """F64, R in {64, 128}, S in {1, 2}, both orders: E against the numpy sum of the ORACLE's ray_color over the emitted records.
    |got - want| <= the summation bound + (pi / R) sum_j F64_BOUND max(1, |L_j|): each L_j of the device may differ from the
    oracle's by the F64 bound of the radiance query (tests/test_ray_query.py).  Observed on the MI355X: worst ratio 0.0018."""
    from tests.test_ray_query import F64_BOUND

    scene = scenes(name)
    depth = CASES[name][4]
    bg = scene.camera(8, 8, 1, depth).background
    points, normals = surface(name)
    worst = {}
    for rays in (64, 128):
        for samples in (1, 2):
            want = bound = None
            for order in ORDERS:
                _upload(renderer, scene, order)
                if want is None:                                  # (the records need a device, not a scene or an order)
                    records = renderer.gather_rays(points, normals, rays=rays, samples=samples)
                    radiance, _ = orc.ray_color(scene.desc_ptr, records, max_depth=depth, background=bg, samples=samples, seed=SEED)
                    want, bound = _summed(radiance, 5, rays, 0)
                    bound = bound + (np.pi / rays) * (F64_BOUND * np.maximum(1.0, np.abs(radiance))).reshape(5, rays, 3).sum(1)
                got = renderer.gather_irradiance(points, normals, max_depth=depth, rays=rays, samples=samples, background=bg, seed=SEED)
                ratio = np.abs(got - want) / bound
                worst[order] = max(worst.get(order, 0.0), float(ratio.max()))
                assert got.any() and np.all(np.abs(got - want) <= bound), (order, rays, samples, float(ratio.max()))
    print(f"{name}: worst |gather - projected oracle| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# One finite reach per scene, the first of these for which the oracle -- on the CPU -- finds a point that is partly open.
REACHES = {"three_spheres": (1.0, 0.3, 3.0), "material_zoo": (2.0, 0.5, 8.0), "cornell_box": (150.0, 50.0, 400.0), "cornell_smoke": (150.0, 50.0, 400.0)}


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("name", SCENES)
def test_occlusion_is_the_query_counted(rt, orc, renderer, scenes, surface, name, real_mode):
    """n = 5, R = 192, rotate = 1, max_distance in {inf, one finite reach}, both orders: open * R is R - sum(rtk_query_occluded
    over the emitted records) exactly, and in F64 R - the oracle's hits; bent within (R + 4) 2^-53 (1 / R) sum |d_c| over the open
    rays of the numpy sum (plus 2^-24 |want| for the result's rounding in F32).  The finite reach is one for which the ORACLE's
    counts give 0 < open < 1 at one point or more, so the interval is seen."""
    scene = scenes(name)
    points, normals = surface(name)
    rays = 192
    reach = None
    for candidate in REACHES[name]:
        records = rules.records(rt.ray_dtype(), points, normals, rays=rays, first_key=3, rotate=1, max_distance=candidate)
        fraction = 1.0 - orc.hits(scene.desc_ptr, records, SEED)["hit"].reshape(5, rays).mean(1)
        if np.any((fraction > 0) & (fraction < 1)):
            reach = candidate
            break
    assert reach is not None, "no reach of the list leaves a point partly open on the oracle"
    for order in ORDERS:
        _upload(renderer, scene, order)
        for max_distance in (0.0, reach):
            kw = dict(rays=rays, first_key=3, rotate=1, max_distance=max_distance)
            records = renderer.gather_rays(points, normals, **kw)
            occluded = renderer.query_occluded(records, seed=SEED, real_mode=real_mode).reshape(5, rays)
            count = rays - occluded.sum(1)
            open_, bent = renderer.gather_occlusion(points, normals, seed=SEED, real_mode=real_mode, **kw)
            as_real = (lambda a: a.astype(np.float32).astype(np.float64)) if real_mode == 1 else (lambda a: a)
            assert np.array_equal(open_, as_real(count / np.float64(rays))), (order, max_distance, open_, count)
            if real_mode == 0:
                oracle = rays - orc.hits(scene.desc_ptr, records, SEED)["hit"].reshape(5, rays).sum(1)
                assert np.array_equal(count, oracle), (order, max_distance)
                if max_distance > 0:
                    assert np.any((count > 0) & (count < rays))
            d = records["direction"].reshape(5, rays, 3) * (occluded == 0)[:, :, None]
            want = d.sum(1) / rays
            bound = (rays + 4) * U64 * np.abs(d).sum(1) / rays + (U32 * np.abs(want) if real_mode == 1 else 0.0)
            assert np.all(np.abs(bent - want) <= bound), (order, max_distance, float((np.abs(bent - want) / np.where(bound > 0, bound, 1.0)).max()))
            assert not bent[count == 0].any()


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("order", ORDERS)
def test_stream_keys_batches_and_shapes_at_their_edges(rt, renderer, scenes, surface, real_mode, order):
    import torch

    name = "material_zoo"
    scene = scenes(name)
    depth = CASES[name][4]
    bg = scene.camera(8, 8, 1, depth).background
    p, nrm = surface(name)
    _upload(renderer, scene, order)
    common = dict(max_depth=depth, rays=128, samples=2, background=bg, seed=SEED, real_mode=real_mode, rotate=1)
    gather = lambda pts, nn, **kw: renderer.gather_irradiance(pts, nn, **{**common, **kw})  # noqa: E731
    occl = lambda pts, nn, **kw: renderer.gather_occlusion(pts, nn, rays=128, samples=2, seed=SEED, real_mode=real_mode, rotate=1, max_distance=REACHES[name][0], **kw)  # noqa: E731
    assert not gather(p, nrm, max_depth=0).any()                  # depth 0: black
    batch = gather(p, nrm, first_key=7)
    o_batch = occl(p, nrm, first_key=7)
    assert batch.any() and o_batch[0].any()
    for k in range(5):                                            # a point alone, with its key: the bits it has inside the batch
        assert _same_bits(batch[k], gather(p[k:k + 1], nrm[k:k + 1], first_key=7 + k)[0]), k
        alone = occl(p[k:k + 1], nrm[k:k + 1], first_key=7 + k)
        assert _same_bits(o_batch[0][k], alone[0][0]) and _same_bits(o_batch[1][k], alone[1][0]), k
    assert not _same_bits(batch[2], gather(p[2:3], nrm[2:3], first_key=7)[0])            # ... its key matters
    for batch_points in (1, 2):                                   # five and three launches of each stage
        assert _same_bits(gather(p, nrm, first_key=7, batch_points=batch_points), batch), batch_points
        o = occl(p, nrm, first_key=7, batch_points=batch_points)
        assert _same_bits(o[0], o_batch[0]) and _same_bits(o[1], o_batch[1]), batch_points
    wrapped = gather(p[[0, 1]], nrm[[0, 1]], first_key=2 ** 32 - 1)                      # point 1 has key 0
    assert _same_bits(wrapped[1], gather(p[1:2], nrm[1:2], first_key=0)[0]) and _same_bits(wrapped[0], gather(p[0:1], nrm[0:1], first_key=2 ** 32 - 1)[0])
    plain = gather(p, nrm, first_key=7, rotate=0)                 # rotation changes the result, and each meets the projected query
    assert not _same_bits(plain, batch)
    for rotate, got in ((0, plain), (1, batch)):
        want, bound = _projected(renderer, p, nrm, rays=128, samples=2, max_depth=depth, background=bg, first_key=7, rotate=rotate, real_mode=real_mode)
        assert np.all(np.abs(got - want) <= bound), rotate
    # the same gather twice more through the device form on a caller stream: the same bits
    real = np.float64 if real_mode == rt.RTK_REAL_F64 else np.float32
    dev = torch.device("cuda:0")
    d_p, d_n = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(nrm.copy()).to(dev)
    d_e = [torch.zeros(15, dtype=torch.float64 if real is np.float64 else torch.float32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        for e in d_e:
            renderer.gather_irradiance_device(5, d_p.data_ptr(), d_n.data_ptr(), e.data_ptr(), **{**common, "first_key": 7}, stream=stream.cuda_stream)
    stream.synchronize()
    assert _same_bits(d_e[0].cpu().numpy(), batch.astype(real)) and _same_bits(d_e[1].cpu().numpy(), batch.astype(real))
    # one point with R = 16384 at depth 1: 256 passes, against the projected query
    got = gather(p[:1], nrm[:1], rays=16384, samples=1, max_depth=1)
    want, bound = _projected(renderer, p[:1], nrm[:1], rays=16384, samples=1, max_depth=1, background=bg, rotate=1, real_mode=real_mode)
    print("R = 16384 %s: worst ratio to the bound %.3f" % (order, float((np.abs(got - want) / np.where(bound > 0, bound, 1.0)).max())))
    assert got.any() and np.all(np.abs(got - want) <= bound)
    assert renderer.gather_irradiance(np.zeros((0, 3)), np.zeros((0, 3)), max_depth=3).shape == (0, 3)
    o = renderer.gather_occlusion(np.zeros((0, 3)), np.zeros((0, 3)))
    assert o[0].shape == (0,) and o[1].shape == (0, 3)


SKY_POINT = (0.0, 1.0e6, -1.0)   # a million above the ground sphere's centre, looking up: no ray of the hemisphere meets the scene


@pytest.mark.gpu
@MODES
def test_a_point_that_sees_only_sky(rt, renderer, scenes, real_mode):
    """three_spheres from far above with the normal +y: every L is the background, so E = pi * background within the summation
    bound; open = 1 exactly; bent = the mean of the emitted directions within the bound of the occlusion test."""
    scene = scenes("three_spheres")
    bg = np.array([0.7, 0.8, 1.0])
    points, normals = np.array([SKY_POINT]), np.array([(0.0, 1.0, 0.0)])
    rays = 256
    for order in ORDERS:
        _upload(renderer, scene, order)
        records = renderer.gather_rays(points, normals, rays=rays)
        assert records["direction"][:, 1].min() > 0 and not renderer.query_occluded(records, seed=SEED, real_mode=real_mode).any()
        got = renderer.gather_irradiance(points, normals, max_depth=10, rays=rays, background=bg, seed=SEED, real_mode=real_mode)
        bg_real = bg if real_mode == rt.RTK_REAL_F64 else bg.astype(np.float32).astype(np.float64)   # as the kernel holds it
        want, bound = _summed(np.tile(bg_real, (rays, 1)), 1, rays, real_mode)
        assert np.all(np.abs(got - want) <= bound) and np.all(np.abs(want - np.pi * bg_real) <= bound)
        open_, bent = renderer.gather_occlusion(points, normals, rays=rays, seed=SEED, real_mode=real_mode)
        d = records["direction"]
        mean = d.sum(0) / rays
        b = (rays + 4) * U64 * np.abs(d).sum(0) / rays + (U32 * np.abs(mean) if real_mode == 1 else 0.0)
        assert open_[0] == 1.0 and np.all(np.abs(bent[0] - mean) <= b)
        assert abs(bent[0, 1] - 2.0 / 3.0) < 2.5e-3 and np.abs(bent[0, [0, 2]]).max() < 2.5e-3   # the set's mean, (0, 0, 2/3) in the frame of +y


# --- buffers and streams ------------------------------------------------------------------------------------------
POISON = 0xA5


def _arena_layout(sizes):
    """Byte offsets of the pieces in one allocation: each 8 past a 16-byte boundary (8-byte aligned, not 16), with at least 64
    guard bytes behind it."""
    offsets, at = [], 8
    for size in sizes:
        offsets.append(at)
        at = (at + size + 64 + 15) // 16 * 16 + 8
    return offsets, at + 64


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("order", ORDERS)
def test_carved_buffers_guard_bytes_and_a_caller_stream(rt, renderer, scenes, surface, real_mode, order):
    """Five points of cornell_smoke: rays, irradiance (in batches of two) and occlusion on one caller stream with a producer in
    front and a consumer behind, in buffers carved at 8-mod-16 offsets out of a poisoned arena.  Every output equals its _host
    form byte for byte; no guard byte changes."""
    import torch

    name = "cornell_smoke"
    scene = scenes(name)
    depth = CASES[name][4]
    _upload(renderer, scene, order)
    real = np.float64 if real_mode == rt.RTK_REAL_F64 else np.float32
    rb = np.dtype(real).itemsize
    n, rays = 5, 64
    points, normals = surface(name)
    kw = dict(rays=rays, samples=2, first_key=3, rotate=1)
    want_rays = renderer.gather_rays(points, normals, max_distance=150.0, **kw)
    want_e = renderer.gather_irradiance(points, normals, max_depth=depth, seed=SEED, real_mode=real_mode, **kw)
    want_open, want_bent = renderer.gather_occlusion(points, normals, max_distance=150.0, seed=SEED, real_mode=real_mode, **kw)
    assert want_e.any() and want_bent.any()
    sizes = (24 * n, 24 * n, 88 * n * rays, 3 * rb * n, rb * n, 3 * rb * n)
    (o_pts, o_nrm, o_rays, o_e, o_open, o_bent), total = _arena_layout(sizes)
    dev = torch.device("cuda:0")
    as_bytes = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).to(dev)  # noqa: E731
    src_pts, src_nrm = as_bytes(points), as_bytes(normals)
    arena = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    assert base % 16 == 0 and all((base + o) % 16 == 8 for o in (o_pts, o_nrm, o_rays, o_e, o_open, o_bent))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        arena[o_pts:o_pts + sizes[0]].copy_(src_pts)              # the producer: until it has run the inputs are poison
        arena[o_nrm:o_nrm + sizes[1]].copy_(src_nrm)
        s = stream.cuda_stream
        renderer.gather_rays_device(n, base + o_pts, base + o_nrm, base + o_rays, max_distance=150.0, stream=s, **kw)
        renderer.gather_irradiance_device(n, base + o_pts, base + o_nrm, base + o_e, max_depth=depth, seed=SEED, real_mode=real_mode, batch_points=2, stream=s, **kw)
        renderer.gather_occlusion_device(n, base + o_pts, base + o_nrm, base + o_open, base + o_bent, max_distance=150.0, seed=SEED, real_mode=real_mode, stream=s, **kw)
        after = arena.clone()                                     # the consumer, same stream, no host synchronisation in between
    stream.synchronize()
    got = after.cpu().numpy()
    piece = lambda o, size: got[o:o + size].tobytes()  # noqa: E731
    assert piece(o_rays, sizes[2]) == want_rays.tobytes()
    assert piece(o_e, sizes[3]) == want_e.astype(real).tobytes()
    assert piece(o_open, sizes[4]) == want_open.astype(real).tobytes() and piece(o_bent, sizes[5]) == want_bent.astype(real).tobytes()
    outside = np.ones(total, bool)
    for o, size in zip((o_pts, o_nrm, o_rays, o_e, o_open, o_bent), sizes):
        outside[o:o + size] = False
    assert np.all(got[outside] == POISON)                         # every guard byte before, between and behind the buffers
    arena2 = torch.full((total,), POISON, dtype=torch.uint8, device=dev)   # n = 0: RTK_OK, nothing written; one output alone: the other untouched
    base2 = arena2.data_ptr()
    renderer.gather_rays_device(0, base2 + o_pts, base2 + o_nrm, base2 + o_rays)
    renderer.gather_irradiance_device(0, base2 + o_pts, base2 + o_nrm, base2 + o_e, max_depth=depth, real_mode=real_mode)
    renderer.gather_occlusion_device(0, base2 + o_pts, base2 + o_nrm, base2 + o_open, base2 + o_bent, real_mode=real_mode)
    torch.cuda.synchronize()
    assert bool((arena2 == POISON).all())
    arena2[o_pts:o_pts + sizes[0]].copy_(src_pts)
    arena2[o_nrm:o_nrm + sizes[1]].copy_(src_nrm)
    renderer.gather_occlusion_device(n, base2 + o_pts, base2 + o_nrm, 0, base2 + o_bent, max_distance=150.0, seed=SEED, real_mode=real_mode, **kw)
    torch.cuda.synchronize()
    got2 = arena2.cpu().numpy()
    assert got2[o_bent:o_bent + sizes[5]].tobytes() == want_bent.astype(real).tobytes() and np.all(got2[o_open:o_open + sizes[4]] == POISON)


@pytest.mark.gpu
def test_misaligned_device_pointers_and_a_missing_scene_are_refused(rt):
    import torch

    r = rt.Renderer(0)
    buf = torch.full((1 << 17,), POISON, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    for call, who in ((lambda: r.gather_irradiance_device(1, p, p + 1024, p + 2048, max_depth=2, rays=64), "rtk_gather_irradiance"),
                      (lambda: r.gather_occlusion_device(1, p, p + 1024, p + 2048, p + 3072, rays=64), "rtk_gather_occlusion")):
        with pytest.raises(rt.RtkError) as e:
            call()
        assert e.value.code == -5 and "no scene" in str(e.value) and who in str(e.value)      # RTK_ERR_NO_SCENE
    for call, word in ((lambda: r.gather_rays_device(1, p + 4, p + 1024, p + 2048, rays=64), "d_points"),
                       (lambda: r.gather_rays_device(1, p, p + 1028, p + 2048, rays=64), "d_normals"),
                       (lambda: r.gather_rays_device(1, p, p + 1024, p + 2052, rays=64), "d_rays"),
                       (lambda: r.gather_irradiance_device(1, p, p + 1024, p + 2052, max_depth=2, rays=64), "d_irradiance"),
                       (lambda: r.gather_irradiance_device(1, p, p + 1024, p + 2050, max_depth=2, rays=64, real_mode=1), "d_irradiance"),
                       (lambda: r.gather_occlusion_device(1, p, p + 1024, p + 2052, p + 3072, rays=64), "d_open"),
                       (lambda: r.gather_occlusion_device(1, p, p + 1024, p + 2048, p + 3074, rays=64, real_mode=1), "d_bent")):
        with pytest.raises(rt.RtkError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value) and "aligned" in str(e.value), str(e.value)
    with pytest.raises(rt.RtkError) as e:
        r.gather_rays_device(2, p, p + 1024, p + 1040, rays=64)
    assert e.value.code == -1 and "overlaps d_normals" in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())
    buf[:48].zero_()
    r.gather_rays_device(1, p, p + 24, p + 1024, rays=64)         # the rays need no scene (point 0, normal 0: finite)
    torch.cuda.synchronize()
    assert not bool((buf[1024:1024 + 88] == POISON).all()) and bool((buf[1024 + 64 * 88:1024 + 64 * 88 + 64] == POISON).all())
    r.close()


# --- the host APIs ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_quad_texels_lie_on_the_descriptions_quad(rt, renderer, scenes):
    """rt.quad_texels of five of cornell_box's own quads as the scene description holds them: the normal is the description's,
    bit for bit; a texel is Q + a u + b v; and rtk_query_hits from p + 0.01 n along -n reports that quad's index."""
    from tests.desc_builder import SceneDesc

    scene = scenes("cornell_box")
    renderer.upload(scene)
    desc = SceneDesc.from_address(scene.desc_ptr)
    vec = lambda v: np.array([v.x, v.y, v.z])  # noqa: E731
    # the green and the red wall, the light, the ceiling and the back wall of scene_library.h, wherever the description holds
    # them (the floor is left out: the two boxes stand on it, and their bottom faces tie with it)
    world = [((555, 0, 0), (0, 555, 0), (0, 0, 555)), ((0, 0, 0), (0, 555, 0), (0, 0, 555)), ((343, 554, 332), (-130, 0, 0), (0, 0, -105)),
             ((555, 555, 555), (-555, 0, 0), (0, 0, -555)), ((0, 0, 555), (555, 0, 0), (0, 555, 0))]
    found = [k for k in range(desc.n_quads) if any(all(np.array_equal(vec(a), b) for a, b in zip((desc.quads[k].Q, desc.quads[k].u, desc.quads[k].v), w)) for w in world)]
    assert len(found) == 5, found
    for index in found:
        q = desc.quads[index]
        Q, u, v = vec(q.Q), vec(q.u), vec(q.v)
        points, normals = rt.quad_texels(Q, u, v, 4, 3)
        assert points.shape == (12, 3) and _same_bits(normals, np.tile(vec(q.normal), (12, 1)))
        i, j = np.arange(12) % 4, np.arange(12) // 4
        assert np.array_equal(points, Q + ((i + 0.5) / 4)[:, None] * u + ((j + 0.5) / 3)[:, None] * v)
        assert np.array_equal(rt.quad_texels(Q, u, v, 1, 1)[0][0], Q + 0.5 * u + 0.5 * v)
        hits = renderer.query_hits(rt.make_rays(points + 0.01 * normals, -normals), seed=SEED)
        assert np.all(hits["hit"] == 1) and np.all(hits["prim_kind"] == rt.NODE_QUAD) and np.all(hits["prim_index"] == index), (index, hits["prim_index"])
        assert np.abs(hits["t"] - 0.01).max() < 1e-9


@pytest.mark.gpu
@MODES
def test_host_api_surface_gather(rt, renderer, scenes, tmp_path, real_mode):
    """rtk::surface_gather (host/rtk_surface_gather.h) gathers irradiance and occlusion at the 3 x 2 texels of the Cornell box's
    red wall; points, normals and results equal what the Python calls give for the same scene and options, bit for bit, in both
    real modes; a refused call shows in status() and rtk_last_error().  The reference order is the class's own."""
    exe = str(tmp_path / "surface_gather_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "helpers", "surface_gather_check.cpp"),
                           "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lrtk_hip", "-Wl,-rpath," + PKG, "-o", exe])
    name, rays, depth, samples = "cornell_box", 128, 6, 2
    scene = scenes(name)
    renderer.upload(scene)                                        # the reference order, as rtk::surface_gather uploads
    points, normals = rt.quad_texels((0.0, 0.0, 0.0), (0.0, 555.0, 0.0), (0.0, 0.0, 555.0), 3, 2)
    kw = dict(rays=rays, samples=samples, first_key=11, rotate=1, seed=5, real_mode=real_mode)
    e = renderer.gather_irradiance(points, normals, max_depth=depth, background=(0.0, 0.0, 0.0), **kw)
    open_, bent = renderer.gather_occlusion(points, normals, max_distance=200.0, **kw)
    want, bound = _projected(renderer, points, normals, rays=rays, samples=samples, max_depth=depth, background=(0.0, 0.0, 0.0), first_key=11, rotate=1, real_mode=real_mode)
    assert e.any() and np.all(np.abs(e - want) <= bound) and np.any((open_ > 0) & (open_ < 1))
    p = subprocess.run([exe, name, scene_file(name, GOLDEN), str(rays), str(depth), str(samples), str(real_mode)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "surface_gather_check: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    rows = lambda tag: np.array([[float(v) for v in line.split()[1:]] for line in p.stdout.splitlines() if line.startswith(tag + " ")])  # noqa: E731
    assert np.array_equal(rows("point"), points) and np.array_equal(rows("normal"), normals)
    assert np.array_equal(rows("e"), e) and np.array_equal(rows("open")[:, 0], open_) and np.array_equal(rows("bent"), bent)
    refused = [line for line in p.stdout.splitlines() if line.startswith("refused ")]
    assert refused and refused[0].split()[1] == "-1" and "rtk_gather_irradiance_host" in refused[0] and "rays" in refused[0]
