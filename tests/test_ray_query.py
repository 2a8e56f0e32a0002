"""Ray queries (include/rtk.h "Ray queries"): hits, occlusion and radiance for rays the caller chooses.

CPU tests: the six entry points are declared and exported, RTK_ABI_VERSION stays 2, the ctypes structures and numpy dtypes have
the layout a C compiler gives the header's structs, and every refusal of the list in the header comes back as RTK_ERR_INVALID with
the offending argument named -- with no device and no context.

GPU tests, in the order of the header's contract:
  1. query_hits is rtk_debug_closest_hit bit for bit on the reference-generated known-answer rays (both real modes);
  2. prim_kind / prim_index name the primitive in the description's tables, the same in both visiting orders;
  3. skip continues the stream at uniform number `skip`, for any skip (the free path in a medium shows the uniform);
  4. query_occluded is query_hits' hit flag, exactly, with and without the early exit;
  5. query_radiance of the render's own camera rays is the oracle's sample, per pixel, with its draw count;
  6. ... and the spp = 1 frame of the render kernels; F32 within test_f32_parity's coherence rule;
  7. samples = 5 is the sum of five single samples in sample order, divided once, bit for bit;
  8. carved, offset buffers with guard words; a caller stream with a producer in front and a consumer behind; n = 0;
  9. rtk::ray_query of the host C++ API gives the same answers (tests/helpers/ray_query_check.cpp).
"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from tests.desc_builder import DescBuilder
from tests.scene_cases import IMAGE_CASES, RENDER_SEED, SCENE_SEED, scene_file
from tests.test_f32_parity import COHERENT_P99, COHERENT_P99_SCENE, MAX_INCOHERENT, TAU

PKG = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
ENTRY_POINTS = ("rtk_query_hits", "rtk_query_occluded", "rtk_query_radiance", "rtk_query_hits_host", "rtk_query_occluded_host", "rtk_query_radiance_host")
F64_BOUND = 1e-12                                                  # the project's F64_RMSE_BOUND, here per channel of every ray
CASES = {c[0]: c for c in IMAGE_CASES}
ORDERS = ("reference", "fast")
MODES = pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])


# ------------------------------------------------------------------------------------------------------------- CPU --
def test_entry_points_are_declared_and_exported(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    assert "#define RTK_ABI_VERSION 2" in header                  # new entry points only
    assert "Ray queries ---" in header
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(rtk_ctx\* ctx, const rtk_query_opts\* opts, int64_t n, const rtk_ray\* [dh]_rays," % name, header), name
    lib = C.CDLL(rt.HIP_LIB_PATH)                                 # loads without a GPU
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.rtk_abi_version() == 2
    import __graft_entry__

    assert "rtk_query.cpp" in __graft_entry__.HIP_SOURCES
    for method in ("query_hits", "query_occluded", "query_radiance", "query_hits_device", "query_occluded_device", "query_radiance_device", "camera_rays"):
        assert callable(getattr(rt.Renderer, method)), method
    assert "rtk_ray_query.h" in open(os.path.join(PKG, "host", "rtk_scene_api.h")).read()


STRUCTS = {"rtk_ray": "Ray", "rtk_ray_hit": "RayHit", "rtk_query_opts": "QueryOpts"}


def test_structures_have_the_headers_layout(rt, tmp_path):
    """sizeof and every field offset of the ctypes structures equal those of a C program compiled against rtk.h; the numpy
    dtypes equal the structures."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rtk.h"', "int main(void) {"]
    for cname, pyname in STRUCTS.items():
        lines.append('    printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in getattr(rt, pyname)._fields_:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        cname, field, value = line.split()
        want[(cname, field)] = int(value)
    assert (want["rtk_ray", "size"], want["rtk_ray_hit", "size"], want["rtk_query_opts", "size"]) == (88, 96, 56)
    for cname, pyname in STRUCTS.items():
        s = getattr(rt, pyname)
        assert C.sizeof(s) == want[cname, "size"], cname
        for field, _ in s._fields_:
            assert getattr(s, field).offset == want[cname, field], (cname, field)
    for dtype, s in ((rt.ray_dtype(), rt.Ray), (rt.ray_hit_dtype(), rt.RayHit)):
        assert dtype.itemsize == C.sizeof(s) and list(dtype.names) == [f[0] for f in s._fields_]
        for field, ctype in s._fields_:
            assert dtype.fields[field][1] == getattr(s, field).offset, field
            assert dtype.fields[field][0].itemsize == C.sizeof(ctype), field
    assert C.alignment(rt.Ray) == C.alignment(rt.RayHit) == 8
    assert (rt.NODE_SPHERE, rt.NODE_QUAD, rt.NODE_TRIANGLE, rt.NODE_MEDIUM) == (1, 2, 3, 8)


def _opts(rt, **kw):
    o = rt.QueryOpts(7, 0, 5, 1, rt.Vec3(0.5, 0.5, 0.5), None, (C.c_int32 * 2)(0, 0))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_refusals_need_no_device(rt):
    """Every refusal of the header's list is RTK_ERR_INVALID with the argument named, from all six entry points, with a null
    context: the argument checks come before anything that needs a device.  Nothing is written."""
    lib = rt.hip_lib()
    err = lambda: lib.rtk_last_error().decode()  # noqa: E731
    rays = rt.make_rays(np.zeros((4, 3)), np.ones((4, 3)))
    out = np.full(4 * 96 + 16, 0x5A, np.uint8)                    # large enough for any output of four rays
    out_ptr = out.ctypes.data + (-out.ctypes.data) % 8
    bad_opts = [(dict(real_mode=2), "real_mode"), (dict(real_mode=-1), "real_mode"), (dict(max_depth=-1), "max_depth"), (dict(samples=-1), "samples"),
                (dict(reserved=(C.c_int32 * 2)(1, 0)), "reserved"), (dict(reserved=(C.c_int32 * 2)(0, -5)), "reserved")]
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        extra = (None,) if "radiance" in name else ()
        host = name.endswith("_host")
        call = lambda opts, n, r, o: fn(None, opts, n, r, o, *extra)  # noqa: E731
        good = C.byref(_opts(rt))
        for fields, word in bad_opts:
            assert call(C.byref(_opts(rt, **fields)), 4, rays.ctypes.data, out_ptr) == -1, (name, fields)
            assert word in err() and name in err(), (name, fields, err())
        assert call(None, 4, rays.ctypes.data, out_ptr) == -1 and "opts" in err()
        for n in (-1, 2 ** 31, 2 ** 40):
            assert call(good, n, rays.ctypes.data, out_ptr) == -1 and " n " in err(), (name, n, err())
        rays_name = "h_rays" if host else "d_rays"
        assert call(good, 4, None, out_ptr) == -1 and rays_name in err(), (name, err())
        assert call(good, 4, rays.ctypes.data, None) == -1 and "null" in err() and re.search(r"null [dh]_(hits|occluded|radiance)", err()), (name, err())
        if not host:
            assert rays.ctypes.data % 8 == 0
            assert call(good, 4, rays.ctypes.data + 4, out_ptr) == -1 and "d_rays" in err() and "aligned" in err(), (name, err())
            assert call(good, 4, rays.ctypes.data, out_ptr + (2 if "occluded" in name else 4)) == -1 and "aligned" in err() and "d_rays" not in err(), (name, err())
            inside = rays.ctypes.data + 88 * 3 + 80                # an output that starts inside the last ray record
            assert call(good, 4, rays.ctypes.data, inside) == -1 and "overlaps d_rays" in err() and name in err(), (name, err())
            assert call(good, 4, rays.ctypes.data + 8, rays.ctypes.data) == -1 and "overlaps d_rays" in err(), (name, err())
            if "radiance" in name:                                # F32 radiance needs 4 bytes only, its draws 4
                f32 = C.byref(_opts(rt, real_mode=1))
                assert fn(None, f32, 4, rays.ctypes.data, out_ptr + 4, None) == -1 and "null context" in err()
                assert fn(None, f32, 4, rays.ctypes.data, out_ptr + 2, None) == -1 and "d_radiance" in err()
                assert fn(None, good, 4, rays.ctypes.data, out_ptr, out_ptr + 2) == -1 and "d_draws" in err()
        assert call(good, 4, rays.ctypes.data, out_ptr) == -1 and "null context" in err(), (name, err())
        assert call(good, 0, rays.ctypes.data, out_ptr) == -1 and "null context" in err()
    assert np.all(out == 0x5A)
    with pytest.raises(ValueError):
        rt.Renderer._query_rays(None, "query_hits", np.zeros((2, 2), rt.ray_dtype()))


# ------------------------------------------------------------------------------------------------------------- GPU --
@pytest.fixture(scope="module")
def scenes(rt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rt.Scene.build(name, SCENE_SEED, scene_file(name, GOLDEN))
        return cache[name]
    return get


def _upload(renderer, scene, cam, order):
    if order == "fast":
        renderer.upload_fast(scene, cam.center)
    else:
        renderer.upload(scene)


def _pixel_samples(w, h, sample):
    j, i = np.mgrid[0:h, 0:w]
    return np.stack([i.ravel(), j.ravel(), np.full(w * h, sample)], 1).astype(np.int32)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _as_debug_records(hits):
    """rtk_ray_hit records in the [n][12] layout of rtk_debug_closest_hit: hit, t, p(3), normal(3), front_face, u, v, material."""
    return np.column_stack([hits["hit"].astype(np.float64), hits["t"], hits["p"], hits["normal"], hits["front_face"].astype(np.float64), hits["u"], hits["v"],
                            hits["material"].astype(np.float64)])


@pytest.mark.gpu
def test_hits_are_the_known_answer_entry_point_bit_for_bit(rt, renderer, tmp_path):
    """Every object of the known-answer scene, the ~3000 reference-generated rays, seed 7 and the recorded keys: query_hits
    equals rtk_debug_closest_hit field for field and bit for bit, draws included, in F64 and F32 -- and so inherits the goldens
    tests/test_gpu_parity.py holds that entry point to."""
    inp = np.load(os.path.join(GOLDEN, "kat_hit_in.npy"))
    meta = np.load(os.path.join(GOLDEN, "kat_hit_meta.npy"))
    blob = bytearray(open(os.path.join(GOLDEN, "kat_scene.rtks"), "rb").read())
    n_hits = n_draws = 0
    for node in np.unique(meta[:, 0]):
        rows = np.nonzero(meta[:, 0] == node)[0]
        blob[8:12] = np.int32(node).tobytes()                     # make this object the scene root
        path = tmp_path / f"obj_{int(node)}.rtks"
        path.write_bytes(bytes(blob))
        renderer.upload(rt.Scene.load(str(path)))
        keys = np.stack([np.full(len(rows), 7), meta[rows, 1], meta[rows, 2]], 1)
        rays = rt.make_rays(inp[rows, 0:3], inp[rows, 3:6], time=inp[rows, 6], tmin=inp[rows, 7], tmax=inp[rows, 8], pixel=meta[rows, 1].astype(np.uint32),
                            sample=meta[rows, 2].astype(np.uint32))
        for mode in (rt.RTK_REAL_F64, rt.RTK_REAL_F32):
            want, want_draws = renderer.closest_hit(inp[rows], keys, real_mode=mode)
            hits = renderer.query_hits(rays, seed=7, real_mode=mode)
            assert _same_bits(_as_debug_records(hits), want), (int(node), mode)
            assert np.array_equal(hits["draws"].astype(np.int64), want_draws.astype(np.int64)), (int(node), mode)
            miss = hits["hit"] == 0
            assert np.all(hits["prim_index"][miss] == -1) and np.all(hits["prim_kind"][miss] == 0) and np.all(hits["prim_index"][~miss] >= 0)
            if mode == rt.RTK_REAL_F64:
                assert np.array_equal(want_draws.astype(np.int64), meta[rows, 3])   # (the goldens' draws, as test_gpu_parity checks them)
                n_hits += int((~miss).sum())
                n_draws += int(want_draws.sum())
    assert n_hits > 500 and n_draws > 20                          # the comparison saw hits, and media that drew


@pytest.mark.gpu
def test_the_known_answer_entry_point_keys_every_ray_by_itself(rt, renderer, tmp_path):
    """rtk_debug_closest_hit takes its seed per ray (keys[.][0]); query_hits takes one for the call.  On the media of the
    known-answer scene -- the objects whose golden rows drew random numbers -- one closest_hit call with seed 7 on the even rows
    and 11 on the odd ones equals, bit for bit and draw for draw, query_hits(seed=7) on the even rows and query_hits(seed=11) on
    the odd ones, in F64 and F32.  A seed word taken from another ray, or from the wrong key, moves a medium's scattering
    distance: at least one odd row's record differs from what seed 7 gives it."""
    inp = np.load(os.path.join(GOLDEN, "kat_hit_in.npy"))
    meta = np.load(os.path.join(GOLDEN, "kat_hit_meta.npy"))
    blob = bytearray(open(os.path.join(GOLDEN, "kat_scene.rtks"), "rb").read())
    media = [node for node in np.unique(meta[:, 0]) if (meta[meta[:, 0] == node, 3] > 0).any()]
    assert media
    for node in media:
        rows = np.nonzero(meta[:, 0] == node)[0]
        seeds = np.where(np.arange(len(rows)) % 2 == 0, 7, 11)
        groups = {seed: np.nonzero(seeds == seed)[0] for seed in (7, 11)}
        assert all(len(g) > 0 and meta[rows[g], 3].sum() > 0 for g in groups.values()), int(node)   # (the goldens' draws, seed 7)
        blob[8:12] = np.int32(node).tobytes()                     # make this object the scene root
        path = tmp_path / f"obj_{int(node)}.rtks"
        path.write_bytes(bytes(blob))
        renderer.upload(rt.Scene.load(str(path)))
        keys = np.stack([seeds, meta[rows, 1], meta[rows, 2]], 1)
        rays = rt.make_rays(inp[rows, 0:3], inp[rows, 3:6], time=inp[rows, 6], tmin=inp[rows, 7], tmax=inp[rows, 8], pixel=meta[rows, 1].astype(np.uint32),
                            sample=meta[rows, 2].astype(np.uint32))
        for mode in (rt.RTK_REAL_F64, rt.RTK_REAL_F32):
            want, want_draws = renderer.closest_hit(inp[rows], keys, real_mode=mode)
            for seed, g in groups.items():
                hits = renderer.query_hits(rays[g], seed=seed, real_mode=mode)
                assert _same_bits(_as_debug_records(hits), want[g]), (int(node), mode, seed)
                assert np.array_equal(hits["draws"].astype(np.int64), want_draws[g].astype(np.int64)), (int(node), mode, seed)
                assert int(want_draws[g].sum()) > 0, (int(node), mode, seed)
            as_seven = _as_debug_records(renderer.query_hits(rays[groups[11]], seed=7, real_mode=mode))
            assert not _same_bits(as_seven, want[groups[11]]), (int(node), mode)


@pytest.mark.gpu
def test_the_known_answer_entry_points_refuse_an_unknown_mode(rt, renderer, scenes):
    """real_mode = 7 is RTK_ERR_INVALID from all four rtk_debug_* entry points, the function and the mode named; nothing is
    written.  (rtk_debug_closest_hit once ran the float kernel for any mode that was not F64.)"""
    lib = rt.hip_lib()
    scene = scenes("three_spheres")
    renderer.upload(scene)
    cam = scene.camera(8, 8, 1, 5)
    ray = np.array([[0.0, 0.0, 3.0, 0.0, 0.0, -1.0, 0.0, 0.001, np.inf]])
    keys, ids, ijs = np.array([[7, 0, 0]], np.uint32), np.zeros(1, np.int32), np.zeros((1, 3), np.int32)
    record, uvp = np.zeros((1, 11)), np.zeros((1, 5))
    out, draws = np.full(14, 123.0), np.full(2, 99, np.uint64)
    ptr = lambda a: a.ctypes.data  # noqa: E731
    calls = {"rtk_debug_closest_hit": lambda m: lib.rtk_debug_closest_hit(renderer._ctx, m, 1, ptr(ray), ptr(keys), ptr(out), ptr(draws)),
             "rtk_debug_scatter": lambda m: lib.rtk_debug_scatter(renderer._ctx, m, 1, ptr(ids), ptr(ray), ptr(record), ptr(keys), ptr(out), ptr(draws)),
             "rtk_debug_texture": lambda m: lib.rtk_debug_texture(renderer._ctx, m, 1, ptr(ids), ptr(uvp), ptr(out), ptr(draws)),
             "rtk_debug_get_ray": lambda m: lib.rtk_debug_get_ray(renderer._ctx, m, C.byref(cam), 7, 1, ptr(ijs), ptr(out), ptr(draws))}
    for name, call in calls.items():
        assert call(7) == -1, name                                # RTK_ERR_INVALID
        assert lib.rtk_last_error().decode() == f"{name}: unknown real_mode 7"
        assert np.all(out == 123.0) and np.all(draws == 99), name
    assert calls["rtk_debug_closest_hit"](rt.RTK_REAL_F32) == 0 and out[0] == 1.0     # (the ray is a good one: it hits the middle sphere)


def _box_quads(b, lo, hi, material):
    """box(a, b, mat) (quad.h:86-108): six quads, front first; returns (list node, index of the front quad)."""
    dx, dy, dz = (hi[0] - lo[0], 0, 0), (0, hi[1] - lo[1], 0), (0, 0, hi[2] - lo[2])
    neg = lambda v: tuple(-c for c in v)  # noqa: E731
    first = len(b.quads)
    sides = [b.quad((lo[0], lo[1], hi[2]), dx, dy, material), b.quad((hi[0], lo[1], hi[2]), neg(dz), dy, material),
             b.quad((hi[0], lo[1], lo[2]), neg(dx), dy, material), b.quad((lo[0], lo[1], lo[2]), dz, dy, material),
             b.quad((lo[0], hi[1], hi[2]), dx, neg(dz), material), b.quad((lo[0], lo[1], lo[2]), dx, dz, material)]
    return b.list(sides), first


def identity_scene():
    """Objects on a grid in the plane z = 0, one ray each from z = 10 down the z axis.  Returns (description, targets) with
    targets = [(x, y, prim_kind, prim_index, material)]."""
    b = DescBuilder()
    m = [b.lambertian((0.1 * k, 0.5, 0.5)) for k in range(8)]
    targets, members = [], []
    for k, x in enumerate((-6.0, -3.0)):                          # two spheres
        members.append(b.sphere((x, 0.0, 0.0), 1.0, m[k]))
        targets.append((x, 0.0, 1, len(b.spheres) - 1, m[k]))
    members.append(b.quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), m[2]))
    targets.append((0.0, 0.0, 2, len(b.quads) - 1, m[2]))
    members.append(b.triangle((2.0, -1.0, 0.0), (4.0, -1.0, 0.0), (3.0, 1.0, 0.0), m[3]))
    targets.append((3.0, -0.5, 3, len(b.triangles) - 1, m[3]))
    box, front = _box_quads(b, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), m[4])   # a box inside translate(rotate_y(...))
    members.append(b.translate(b.rotate_y(box, 15.0), (6.0, 0.0, 0.0)))
    targets.append((6.0, 0.0, 2, front, m[4]))
    shared = b.sphere((0.0, 0.0, 0.0), 0.5, m[5])                 # one sphere, two instances: the same index from both
    for x in (0.0, 3.0):
        members.append(b.translate(shared, (x, 4.0, 0.0)))
        targets.append((x, 4.0, 1, len(b.spheres) - 1, m[5]))
    members.append(b.medium(b.sphere((-6.0, 4.0, 0.0), 1.0, m[6]), 1e6, (0.9, 0.9, 0.9)))   # dense: the free path is ~1e-6
    targets.append((-6.0, 4.0, 8, len(b.media) - 1, b.media[-1].material))
    fog_box, _ = _box_quads(b, (-3.5, 3.5, -0.5), (-2.5, 4.5, 0.5), m[7])                    # ... and one whose boundary is not a sphere
    members.append(b.medium(fog_box, 1e6, (0.2, 0.9, 0.9)))
    targets.append((-3.0, 4.0, 8, len(b.media) - 1, b.media[-1].material))
    return b.finish(b.list(members)), targets


@pytest.mark.gpu
@MODES
def test_primitive_identity_in_both_orders(rt, renderer, real_mode):
    desc, targets = identity_scene()
    xy = np.array([(t[0], t[1]) for t in targets] + [(100.0, 100.0)])   # the last ray misses everything
    rays = rt.make_rays(np.column_stack([xy, np.full(len(xy), 10.0)]), (0.0, 0.0, -1.0), pixel=np.arange(len(xy), dtype=np.uint32))
    want = [(t[2], t[3], t[4]) for t in targets]
    assert len(set(want)) == len(want) - 1                        # nine targets, eight primitives: the shared sphere twice
    results = []
    for order in ORDERS:
        if order == "fast":
            renderer.upload_fast(desc, rt.Vec3(0.0, 0.0, 10.0))
        else:
            renderer.upload(desc)
        hits = renderer.query_hits(rays, seed=3, real_mode=real_mode)
        got = [(int(h["prim_kind"]), int(h["prim_index"]), int(h["material"])) for h in hits[:-1]]
        assert got == want, (order, got, want)
        assert np.all(hits["hit"][:-1] == 1) and np.all(np.abs(hits["p"][:-1, 2]) <= 1.0 + 1e-5)
        assert np.array_equal(hits["draws"][:-1] > 0, np.array([t[2] == 8 for t in targets]))   # only the media drew
        miss = hits[-1]
        assert (int(miss["hit"]), int(miss["prim_kind"]), int(miss["prim_index"]), int(miss["material"]), int(miss["draws"])) == (0, 0, -1, -1, 0)
        assert miss.tobytes()[:72] == bytes(72)                   # every real of a miss is +0
        results.append(hits)
    assert _same_bits(results[0], results[1])                     # the visiting order changes nothing a caller sees


# --- skip-ahead ---------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF
LCG_A, LCG_C = 747796405, 2891336453


def _pcg_hash(v):
    st = (v * LCG_A + LCG_C) & M32
    w = (((st >> ((st >> 28) + 4)) ^ st) * 277803737) & M32
    return (w >> 22) ^ w


def uniform_at(seed, pixel, sample, skip):
    """Uniform number `skip` of the stream (seed, pixel, sample): the seeding of the device's streams, the generator's step
    s <- a s + c composed `skip` times by squaring in numpy's uint32 arithmetic, then the generator's output function."""
    with np.errstate(over="ignore"):
        mult, plus, acc_mult, acc_plus = np.uint32(LCG_A), np.uint32(LCG_C), np.uint32(1), np.uint32(0)
        n = int(skip)
        while n:
            if n & 1:
                acc_mult, acc_plus = acc_mult * mult, acc_plus * mult + plus
            plus, mult = (mult + np.uint32(1)) * plus, mult * mult
            n >>= 1
        state = int(acc_mult * np.uint32(_pcg_hash((pixel + _pcg_hash((sample + _pcg_hash(seed)) & M32)) & M32)) + acc_plus)
    w = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return (((w >> 22) ^ w) >> 8) / 16777216.0


SKIPS = (0, 1, 2, 31, 65537, 2 ** 32 - 1)


@pytest.mark.gpu
def test_skip_continues_the_stream(rt, renderer, orc):
    """A sphere-bounded medium of density 50 and radius 1; rays through the centre enter at t = 2 exactly, and the hit lies a
    free path -log(u) / 50 further along: t = 2 + (-1 / 50) log(u) / |rd| shows which uniform the query drew."""
    seed, density = 11, 50.0
    b = DescBuilder()
    desc = b.finish(b.list([b.medium(b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian((0.5, 0.5, 0.5))), density, (0.8, 0.8, 0.8))]))
    renderer.upload(desc)
    keys = [(p, s) for p in (5, 1234567) for s in (0, 9)]
    for pixel, sample in keys:                                    # the numpy restatement against the oracle's generator
        stream = orc.rng_stream(seed, pixel, sample, 32)
        for k in (0, 1, 2, 31):
            assert uniform_at(seed, pixel, sample, k) == stream[k], (pixel, sample, k)
    cases = [(p, s, k) for p, s in keys for k in SKIPS]
    u = np.array([uniform_at(seed, p, s, k) for p, s, k in cases])
    assert np.all(u > 0) and len(set(u)) == len(u)                # keys whose uniforms are usable, and all different
    pixel, sample, skip = (np.array(c, dtype=np.uint32) for c in zip(*[(p, s, k) for p, s, k in cases]))
    rays = rt.make_rays((0.0, 0.0, -5.0), (0.0, 0.0, 2.0), tmin=0.001, tmax=np.inf, pixel=pixel, sample=sample, skip=skip)
    hits = renderer.query_hits(rays, seed=seed)
    want = 2.0 + (-1.0 / density) * np.log(u) / 2.0
    assert np.all(hits["hit"] == 1) and np.all(hits["draws"] == 1) and np.all(hits["prim_kind"] == 8)
    rel = np.abs(hits["t"] - want) / want
    print("skip-ahead: worst relative error of t %.3e" % rel.max())
    assert rel.max() <= 1e-13, rel
    assert np.array_equal(renderer.query_occluded(rays, seed=seed), hits["hit"])


# --- occlusion ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_spheres", "cornell_box", "mesh", "cornell_smoke"])
def test_occlusion_is_the_hit_flag(rt, renderer, scenes, name):
    """4096 segments between random point pairs, plus the camera rays.  The pairs are drawn inside the axis-aligned box of the
    points the case's camera rays hit and the eye: a box inside the scene's bounds that needs no table of them, and the part where
    segments meet both answers (the assertion on the occluded fraction below).  The occlusion
    flag equals query_hits' hit flag exactly, in both orders and both modes (each mode against itself: no tolerance).  The
    first three scenes take the early exit, cornell_smoke (media) the closest-hit walk."""
    _, w, h, _, depth = CASES[name]
    scene = scenes(name)
    cam = scene.camera(w, h, 1, depth)
    renderer.upload(scene)
    cam_rays = renderer.camera_rays(cam, RENDER_SEED, _pixel_samples(w, h, 0))
    seen = renderer.query_hits(cam_rays, seed=RENDER_SEED)
    points = np.vstack([seen["p"][seen["hit"] == 1], [[cam.center.x, cam.center.y, cam.center.z]]])
    lo, hi = points.min(0), points.max(0)
    rng = np.random.default_rng(2024)
    a, b = (lo + (hi - lo) * rng.random((4096, 3)) for _ in range(2))
    segments = rt.make_rays(a, b - a, tmin=0.001, tmax=1 - 0.001, pixel=np.arange(4096, dtype=np.uint32), sample=7)
    rays = np.concatenate([segments, cam_rays])
    flags = {}
    for order in ORDERS:
        _upload(renderer, scene, cam, order)
        for mode in (rt.RTK_REAL_F64, rt.RTK_REAL_F32):
            occluded = renderer.query_occluded(rays, seed=RENDER_SEED, real_mode=mode)
            hits = renderer.query_hits(rays, seed=RENDER_SEED, real_mode=mode)
            assert occluded.dtype == np.int32 and np.array_equal(occluded, hits["hit"]), (order, mode, int((occluded != hits["hit"]).sum()))
            flags[order, mode] = occluded
    f64 = flags["reference", rt.RTK_REAL_F64]
    assert np.array_equal(f64, flags["fast", rt.RTK_REAL_F64])
    frac = float(f64[:4096].mean())
    print(f"{name}: {frac:.3f} of the segments occluded")
    assert 0.02 < frac < 0.98                                     # the segments saw both answers


# --- radiance -----------------------------------------------------------------------------------------------------
ORACLE_CASES = ["three_spheres", "cornell_box", "material_zoo", "cornell_smoke", "obj_mesh", "book1_final"]


@pytest.fixture(scope="module")
def oracle_samples(orc, scenes):
    """(radiance [n][3], draws [n]) of the oracle's ray_color for every pixel's sample `sample` at `depth`, computed once."""
    cache = {}

    def get(name, depth, sample):
        key = (name, depth, sample)
        if key not in cache:
            _, w, h, _, _ = CASES[name]
            scene = scenes(name)
            cam = scene.camera(w, h, 1, max(depth, 1))
            cam.max_depth = depth                                 # (scene.camera reads 0 as "the scene's default")
            fn = orc.lib().orc_sample
            rgb, draws = np.zeros((w * h, 3)), np.zeros(w * h, np.uint64)
            for k in range(w * h):
                assert fn(scene.desc_ptr, C.addressof(cam), RENDER_SEED, k % w, k // w, sample, rgb[k].ctypes.data, draws[k:].ctypes.data) == 0
            cache[key] = (rgb, draws)
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_radiance_is_the_oracles_sample(rt, renderer, scenes, oracle_samples, name):
    """Every pixel of the case's size, samples 0 and 1, depths {0, 1, the case's} (book1_final: its depth and sample 0 only),
    both orders: |query - oracle| <= 1e-12 max(1, |oracle|) per channel, and the draws of get_ray plus the query's equal the
    oracle's exactly."""
    _, w, h, _, depth = CASES[name]
    scene = scenes(name)
    combos = [(depth, 0)] if name == "book1_final" else [(d, s) for d in (0, 1, depth) for s in (0, 1)]
    worst = 0.0
    for order in ORDERS:
        for d, s in combos:
            cam = scene.camera(w, h, 1, max(d, 1))
            cam.max_depth = d                                     # (scene.camera reads 0 as "the scene's default")
            _upload(renderer, scene, cam, order)
            rays = renderer.camera_rays(cam, RENDER_SEED, _pixel_samples(w, h, s))
            got, draws = renderer.query_radiance(rays, max_depth=d, background=cam.background, count=True, seed=RENDER_SEED)
            want, want_draws = oracle_samples(name, d, s)
            err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, float(err.max()))
            assert err.max() <= F64_BOUND, (order, d, s, float(err.max()))
            assert np.array_equal(draws.astype(np.uint64) + rays["skip"].astype(np.uint64), want_draws), (order, d, s)
            if d == 0:
                assert not got.any() and not draws.any()
            plain = renderer.query_radiance(rays, max_depth=d, background=cam.background, seed=RENDER_SEED)
            assert _same_bits(plain, got), (order, d, s)          # the counting build computes the same
    if name == "book1_final":
        assert len(set(rays["skip"].tolist())) > 1                # defocus: the lens rejection loop makes skip vary per ray
    print(f"{name}: worst |query - oracle| / max(1, |oracle|) = {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", IMAGE_CASES, ids=[c[0] for c in IMAGE_CASES])
def test_radiance_of_the_camera_rays_is_the_frame(rt, renderer, scenes, case):
    """A render_host frame at spp = 1 equals the radiance of its camera rays under the F64 bound; in F32 the query meets
    test_f32_parity's coherence rule against the F64 query (its constants, imported)."""
    name, w, h, _, depth = case
    scene = scenes(name)
    cam = scene.camera(w, h, 1, depth)
    ijs = _pixel_samples(w, h, 0)
    for order in ORDERS:
        _upload(renderer, scene, cam, order)
        frame, _, _ = renderer.render_host(cam, seed=RENDER_SEED)
        rays = renderer.camera_rays(cam, RENDER_SEED, ijs)
        f64 = renderer.query_radiance(rays, max_depth=depth, background=cam.background, seed=RENDER_SEED)
        err = np.abs(f64 - frame.reshape(-1, 3)) / np.maximum(1.0, np.abs(frame.reshape(-1, 3)))
        assert err.max() <= F64_BOUND, (order, float(err.max()))
        rays32 = renderer.camera_rays(cam, RENDER_SEED, ijs, real_mode=rt.RTK_REAL_F32)
        f32 = renderer.query_radiance(rays32, max_depth=depth, background=cam.background, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F32)
        assert np.isfinite(f32).all()
        rel = (np.abs(f32 - f64) / np.maximum(1.0, np.abs(f64))).max(axis=1)
        inco = rel > TAU
        frac, p99 = float(inco.mean()), float(np.percentile(rel[~inco], 99))
        print(f"{name} {order}: worst f64 error {err.max():.3e}; f32 incoherent fraction {frac:.4f}, coherent p99 {p99:.3e}")
        assert frac <= MAX_INCOHERENT[name][2], (order, frac)
        assert p99 <= COHERENT_P99_SCENE.get(name, COHERENT_P99), (order, p99)


@pytest.mark.gpu
@MODES
def test_samples_sum_in_sample_order(rt, renderer, scenes, real_mode):
    """samples = 5 is ((r0 + r1) + r2 + r3 + r4) / 5 of five single-sample queries with sample keys sample .. sample + 4,
    evaluated in the mode's own type: bit for bit."""
    name, w, h, _, depth = CASES["material_zoo"]
    scene = scenes(name)
    cam = scene.camera(w, h, 1, depth)
    renderer.upload(scene)
    rays = renderer.camera_rays(cam, RENDER_SEED, _pixel_samples(w, h, 3), real_mode=real_mode)
    real = np.float64 if real_mode == rt.RTK_REAL_F64 else np.float32
    query = lambda r, n: renderer.query_radiance(r, max_depth=depth, background=cam.background, samples=n, seed=RENDER_SEED, real_mode=real_mode)  # noqa: E731
    singles = []
    for s in range(5):
        r = rays.copy()
        r["sample"] += s
        singles.append(query(r, 1).astype(real))
    assert not _same_bits(singles[0], singles[1])
    total = singles[0] + singles[1]
    for s in singles[2:]:
        total = total + s
    want = total / real(5)
    assert want.dtype == real
    got = query(rays, 5).astype(real)
    assert _same_bits(got, want), float(np.abs(got - want).max())
    assert _same_bits(query(rays, 0).astype(real), singles[0])    # samples 0 = 1


# --- buffers and streams ------------------------------------------------------------------------------------------
POISON = 0xA5


def _arena_layout(n, real_bytes):
    """Byte offsets of (rays, hits, occluded, radiance, draws) in one allocation: each 8 past a 16-byte boundary (8-byte
    aligned, not 16), with at least 64 guard bytes behind it."""
    sizes = (88 * n, 96 * n, 4 * n, 3 * real_bytes * n, 4 * n)
    offsets, at = [], 8
    for size in sizes:
        offsets.append(at)
        at = (at + size + 64 + 15) // 16 * 16 + 8
    return offsets, sizes, at + 64


@pytest.mark.gpu
@MODES
@pytest.mark.parametrize("n", [1, 63, 64, 257])
def test_carved_buffers_guard_words_and_a_caller_stream(rt, renderer, scenes, real_mode, n):
    import torch

    name, w, h, _, depth = CASES["cornell_smoke"]                 # media: hits and occlusion draw, the closest-hit walk runs
    scene = scenes(name)
    cam = scene.camera(w, h, 1, depth)
    renderer.upload(scene)
    rng = np.random.default_rng(n)
    ijs = _pixel_samples(w, h, 0)[rng.choice(w * h, n, replace=False)]
    rays = renderer.camera_rays(cam, RENDER_SEED, ijs, real_mode=real_mode)
    bg = cam.background
    want_hits = renderer.query_hits(rays, seed=RENDER_SEED, real_mode=real_mode)
    want_occ = renderer.query_occluded(rays, seed=RENDER_SEED, real_mode=real_mode)
    want_rad, want_draws = renderer.query_radiance(rays, max_depth=depth, background=bg, count=True, seed=RENDER_SEED, real_mode=real_mode)
    real = np.float64 if real_mode == rt.RTK_REAL_F64 else np.float32
    (o_rays, o_hits, o_occ, o_rad, o_draws), sizes, total = _arena_layout(n, np.dtype(real).itemsize)
    dev = torch.device("cuda:0")
    source = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).to(dev)
    arena = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    assert base % 16 == 0 and all((base + o) % 16 == 8 for o in (o_rays, o_hits, o_occ, o_rad, o_draws))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        arena[o_rays:o_rays + 88 * n].copy_(source)               # the producer: until it has run the rays are poison
        s = stream.cuda_stream
        renderer.query_hits_device(n, base + o_rays, base + o_hits, seed=RENDER_SEED, real_mode=real_mode, stream=s)
        renderer.query_occluded_device(n, base + o_rays, base + o_occ, seed=RENDER_SEED, real_mode=real_mode, stream=s)
        renderer.query_radiance_device(n, base + o_rays, base + o_rad, base + o_draws, max_depth=depth, background=bg, seed=RENDER_SEED, real_mode=real_mode,
                                       stream=s)
        after = arena.clone()                                     # the consumer, same stream, no host synchronisation in between
    stream.synchronize()
    got = after.cpu().numpy()
    piece = lambda o, size: got[o:o + size].tobytes()  # noqa: E731
    assert piece(o_rays, sizes[0]) == rays.tobytes()
    assert piece(o_hits, sizes[1]) == want_hits.tobytes()
    assert piece(o_occ, sizes[2]) == want_occ.tobytes()
    assert piece(o_rad, sizes[3]) == want_rad.astype(real).tobytes()
    assert piece(o_draws, sizes[4]) == want_draws.tobytes()
    outside = np.ones(total, bool)
    for o, size in zip((o_rays, o_hits, o_occ, o_rad, o_draws), sizes):
        outside[o:o + size] = False
    assert np.all(got[outside] == POISON)                         # every guard byte before, between and behind the buffers
    # the plain (non-counting) radiance build and n = 0: RTK_OK, nothing written
    arena2 = arena.clone()
    base2 = arena2.data_ptr()
    renderer.query_radiance_device(n, base2 + o_rays, base2 + o_rad, max_depth=depth, background=bg, seed=RENDER_SEED, real_mode=real_mode)
    torch.cuda.synchronize()
    assert torch.equal(arena2, after)
    arena2.fill_(POISON)
    renderer.query_hits_device(0, base2 + o_rays, base2 + o_hits, real_mode=real_mode)
    renderer.query_occluded_device(0, base2 + o_rays, base2 + o_occ, real_mode=real_mode)
    renderer.query_radiance_device(0, base2 + o_rays, base2 + o_rad, base2 + o_draws, max_depth=depth, real_mode=real_mode)
    torch.cuda.synchronize()
    assert bool((arena2 == POISON).all())
    assert len(renderer.query_hits(rays[:0])) == 0 and renderer.query_radiance(rays[:0], max_depth=3).shape == (0, 3)


@pytest.mark.gpu
def test_misaligned_device_pointers_and_a_missing_scene_are_refused(rt):
    import torch

    r = rt.Renderer(0)
    buf = torch.full((4096,), POISON, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    with pytest.raises(rt.RtkError) as e:
        r.query_hits_device(4, p, p + 1024)
    assert e.value.code == -5 and "no scene" in str(e.value)      # RTK_ERR_NO_SCENE
    for call, word in ((lambda: r.query_hits_device(4, p + 4, p + 1024), "d_rays"), (lambda: r.query_hits_device(4, p, p + 1028), "d_hits"),
                       (lambda: r.query_occluded_device(4, p, p + 1026), "d_occluded"),
                       (lambda: r.query_radiance_device(4, p, p + 1028, max_depth=2), "d_radiance"),
                       (lambda: r.query_radiance_device(4, p, p + 1024, p + 2050, max_depth=2), "d_draws")):
        with pytest.raises(rt.RtkError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value) and "aligned" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())
    r.close()


# --- the host C++ API ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_api_ray_query(rt, renderer, scenes, tmp_path):
    """rtk::ray_query (host/rtk_ray_query.h) on a library scene built exactly as librtk_host.so builds it: hit, occluded and
    radiance -- single and batch forms -- agree bit for bit with what Python computes for the same scene and rays."""
    exe = str(tmp_path / "ray_query_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "helpers", "ray_query_check.cpp"),
                           "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lrtk_hip", "-Wl,-rpath," + PKG, "-o", exe])
    name, w, h, _, depth = CASES["material_zoo"]
    scene = scenes(name)
    cam = scene.camera(w, h, 1, depth)
    renderer.upload(scene)                                        # the reference order, as rtk::ray_query uploads
    rng = np.random.default_rng(5)
    view = renderer.camera_rays(cam, RENDER_SEED, _pixel_samples(w, h, 0)[rng.choice(w * h, 40, replace=False)])
    seen = renderer.query_hits(view, seed=1)
    assert seen["hit"].sum() >= 20
    # 40 rays with keys (0, 0, 0) -- what the single forms use: the camera's, and 24 segments between points the camera sees
    a, b = seen["p"][seen["hit"] == 1][:12], np.roll(seen["p"][seen["hit"] == 1][:12], 5, axis=0)
    a, b = np.vstack([a, b]), np.vstack([b, a + [0.0, 40.0, 0.0]])
    rays = np.concatenate([rt.make_rays(view["origin"][:16], view["direction"][:16], time=view["time"][:16]), rt.make_rays(a, b - a, tmin=0.001, tmax=1 - 0.001)])
    n, samples, bg = len(rays), 3, (0.25, 0.5, 0.75)
    hits = renderer.query_hits(rays, seed=1)
    occluded = renderer.query_occluded(rays, seed=1)
    radiance = renderer.query_radiance(rays, max_depth=depth, background=bg, samples=samples, seed=1)
    assert occluded.any() and radiance.any()
    case = tmp_path / "case.bin"
    case.write_bytes(struct.pack("<3i3d", n, depth, samples, *bg) + rays.tobytes() + hits.tobytes() + occluded.tobytes() + radiance.tobytes()
                     + np.ascontiguousarray(a).tobytes() + np.ascontiguousarray(b).tobytes())
    p = subprocess.run([exe, name, scene_file(name, GOLDEN), str(case)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "ray_query_check: ok" in p.stdout
