"""CPU tests: the C-ABI library loads and exports what include/rtk.h declares; host-side
logic (flattener, tiling arithmetic, byte model); the product refuses to run without a GPU."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.conftest import EARTH, GOLDEN, ROOT
from tests.kernel_matrix import kernel_static_lds
from tests.scene_cases import IMAGE_CASES, SCENE_SEED, scene_file


def test_hip_library_exports_every_declared_symbol(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtk_[a-z0-9_]+)\s*\(", body)))
    assert "rtk_render_device" in declared and "rtk_scene_upload" in declared and len(declared) >= 11
    lib = C.CDLL(rt.HIP_LIB_PATH)  # loading must work without a GPU
    missing = [name for name in declared if not hasattr(lib, name)]
    assert not missing, missing
    assert lib.rtk_abi_version() == rt.RTK_ABI_VERSION


def test_kernels_are_built_for_gfx950_only(rt):
    blob = open(rt.HIP_LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx90a", b"gfx942", b"sm_90"):
        assert other not in blob


def test_render_kernels_declare_no_static_lds(rt, tmp_path):
    """The lean MIXED kernel uses its byte program counters as LDS addresses (rtk_trace.hip rec_at): the staged program must
    start at LDS address 0, i.e. the kernels' static LDS size in the code object's metadata must be 0."""
    sizes = kernel_static_lds(rt.HIP_LIB_PATH, tmp_path)
    if sizes is None:
        pytest.skip("ROCm LLVM binary tools not present")
    render = {k: v for k, v in sizes.items() if "rtk_render_kernel" in k}
    assert len(render) >= 20, sorted(sizes)[:5]
    assert all(v == 0 for v in render.values()), {k: v for k, v in render.items() if v}


def test_every_compiled_render_kernel_is_accounted_for(rt, tmp_path):
    """The rtk_render_kernel instantiations in librtk_hip.so == the ones the rows of tests/kernel_matrix.py select (each launched and
    checked on the device by tests/test_kernel_matrix.py) + the ones listed there as unreachable, with the reason.  An instantiation
    added to rtk_trace.hip without a row fails here; so does a row taken away."""
    from tests import kernel_matrix as km

    sizes = kernel_static_lds(rt.HIP_LIB_PATH, tmp_path)
    if sizes is None:
        pytest.skip("ROCm LLVM binary tools not present")
    compiled = km.compiled_instantiations(sizes)
    assert len(compiled) == len(set(compiled)) == sum("rtk_render_kernel" in name for name in sizes)   # every symbol parsed
    expected = {}
    for row in km.ROWS:
        assert row.expect[0] == row.real and row.expect[2] == row.count, row
        if row.expect in expected:
            assert row.note, f"{km.row_id(row)} expects {row.expect} like {km.row_id(expected[row.expect])} and gives no reason"
        else:
            assert not row.note, f"{km.row_id(row)}: a reason for a duplicate on the first row that expects {row.expect}"
            expected[row.expect] = row
    for row in km.ROWS:   # an f32 F_LDS_BOXES row is checked against its all-in-memory twin: the twin (a duplicate tuple) must be there
        if row.real == km.F32 and row.expect[1] & 1024:
            twin = row._replace(variant=row.variant | km.V_NO_LDS_BOXES, expect=(row.real, row.expect[1] & ~1024, False, False))
            assert any(r[:6] == twin[:6] for r in km.ROWS), f"{km.row_id(row)} has no row at variant | V_NO_LDS_BOXES"
    assert all(isinstance(why, str) and why.strip() for why in km.UNREACHABLE.values())
    assert not set(expected) & set(km.UNREACHABLE), sorted(set(expected) & set(km.UNREACHABLE))
    accounted = set(expected) | set(km.UNREACHABLE)
    assert set(compiled) == accounted, {"compiled, in no row": sorted(set(compiled) - accounted), "in the table, not compiled": sorted(accounted - set(compiled))}
    assert len({km.row_id(r) for r in km.ROWS}) == len(km.ROWS)


def test_product_fails_loudly_without_a_device(rt):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(rt.RtkError) as err:
        rt.Renderer(0)
    assert err.value.code == -2  # RTK_ERR_NO_DEVICE: no CPU fallback exists


def test_multi_gpu_entry_points_fail_loudly_without_a_device(rt):
    """rtk_init_multi (several GPUs behind camera::render) has no CPU path either; argument errors come first."""
    import torch

    lib = rt.hip_lib()
    handle = C.c_void_p()
    devs = (C.c_int * 2)(0, 1)
    assert lib.rtk_init_multi(0, devs, 0, C.byref(handle)) == -1 and not handle.value          # RTK_ERR_INVALID: no devices
    assert lib.rtk_init_multi(2, devs, 7, C.byref(handle)) == -1                                # unknown gather mode
    assert lib.rtk_init_multi(2, None, 0, C.byref(handle)) == -1
    assert lib.rtk_multi_device_count(None) == 0 and lib.rtk_multi_destroy(None) == 0
    assert lib.rtk_set_progress_callback(None, C.cast(None, rt.PROGRESS_FN), None, 0) == -1
    if not torch.cuda.is_available():
        with pytest.raises(rt.RtkError) as err:
            rt.MultiRenderer([0, 1])
        assert err.value.code == -2 and "no CPU path" in str(err.value)


def test_multi_enqueue_buffer_sets_and_waits_follow_the_two_frames_in_flight_rule(rt):
    """rtk_render_multi_enqueue keeps two frames in flight: frame k renders into buffer set k % 2 while frame k - 1 is gathered
    and un-permuted out of the other one, and from frame 2 on the renders first wait (on the device) for the release of their
    set by frame k - 2.  rtk_multi_frame_plan IS the rule the enqueue follows (host-only); the ordering it implies is checked
    here on a model of the streams: no buffer set is ever written while an earlier frame still reads it."""
    lib = rt.hip_lib()
    out = (C.c_int32 * 2)()
    assert lib.rtk_multi_frame_plan(-1, out) == -1 and lib.rtk_multi_frame_plan(0, None) == -1
    released_at = {}          # buffer set -> index of the frame whose un-permute released it last
    for frame in range(9):
        assert lib.rtk_multi_frame_plan(frame, out) == 0
        slot, waits = out[0], out[1]
        assert slot == frame % 2
        # the set was last used by frame - 2: the renders of `frame` must wait for exactly that release, and only then
        assert waits == (1 if frame >= 2 else 0)
        if waits:
            assert released_at[slot] == frame - 2
        # frame - 1 lives in the OTHER set: its gather / un-permute overlap this frame's renders without a hazard
        if frame >= 1:
            assert released_at.get(1 - slot, frame - 1) == frame - 1
        released_at[slot] = frame
    # argument errors come before any device work; no device -> the usual loud failure, never a fallback
    assert lib.rtk_render_multi_enqueue(None, None, None, None, None) == -1 and lib.rtk_multi_wait(None) == -1


def test_frame_launches_follow_the_workspace_budget(rt):
    """rtk_frame_launches (host-only): the partial-sum workspace is a byte budget (1.095 GB per context = 22 planes of a 1920x1080
    f64 frame); a frame whose sample chunks need more planes than the budget holds is rendered in passes.  The BASELINE configs:
    C2 (13 chunks) one launch, C3 (63 chunks of an 800x800 frame: 0.97 GB) one, C4 (32 chunks at 1920x1080) two, C5 (63) three;
    an eighth of the tiles of any of them one; float planes are half the size."""
    lib = rt.hip_lib()

    def launches(w, h, spp, n_ranks=1, real=rt.RTK_REAL_F64, variant=0):
        cam = rt.Camera()
        cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, spp, 10
        opts = rt.RenderOpts(1, real, 0, n_ranks, 0, variant, None)
        return lib.rtk_frame_launches(C.byref(cam), C.byref(opts))

    assert launches(1920, 1080, 100) == 1 and launches(800, 800, 1000) == 1
    assert launches(1920, 1080, 256) == 2 and launches(1920, 1080, 1000) == 3
    assert launches(1920, 1080, 1000, n_ranks=8) == 1 and launches(1920, 1080, 1000, n_ranks=2) == 2
    assert launches(1920, 1080, 1000, real=rt.RTK_REAL_F32) == 2
    assert launches(1920, 1080, 1000, variant=1 << 24) == 1          # tests: one launch whatever the chunk count
    assert launches(7680, 4320, 512) == 8                            # a frame 16x as large: never fewer than 8 chunks per launch
    assert launches(0, 1080, 100) == -1 and launches(1920, 1080, 0) == -1 and lib.rtk_frame_launches(None, None) == -1


def test_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    offenders = []
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                text = open(os.path.join(base, f), errors="ignore").read()
                uses = (re.search(r'^\s*#\s*include\s*[<"][^>"]*oracle', text, re.M) or re.search(r"^\s*(from|import)\s+oracle", text, re.M)
                        or "liboracle" in text or "orc_render" in text or "ref_driver" in text.replace("oracle/ref_driver.cpp", ""))
                if uses:
                    offenders.append(f)
    assert not offenders, offenders


def test_camera_struct_layout_matches_c(rt):
    scene = rt.Scene.build("three_spheres")
    cam = scene.camera(400, 225, 10, 10)
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth) == (400, 225, 10, 10)
    assert cam.pixel_samples_scale == 1.0 / 10  # the LAST field of rtk_camera: the whole layout lines up
    assert (cam.background.x, cam.background.y, cam.background.z) == (0.7, 0.8, 1.0)
    assert cam.defocus_angle == 0.0
    full = rt.Scene.build("book1_final").camera()
    assert (full.image_width, full.image_height, full.samples_per_pixel, full.max_depth) == (1920, 1080, 100, 50)


def _initialize_literal(W, aspect, vfov, lookfrom, lookat, vup, defocus_angle, focus_dist):
    """Camera.txt:136-175 restated line by line in Python floats (IEEE double, same operation order; vec3 `/ t` is
    `(1/t) * v`, vec3.h:91-93; unit_vector(v) = v / v.length(), vec3.h:103-105; degrees_to_radians = d * pi / 180,
    rtweekend.h:22-24)."""
    import math

    def sub(a, b): return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    def add(a, b): return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]
    def mul(t, a): return [t * a[0], t * a[1], t * a[2]]
    def div(a, t): return mul(1 / t, a)
    def cross(a, b): return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    def unit(a): return div(a, math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))
    pi = 3.1415926535897932385
    image_height = int(W / aspect)                      # Camera.txt:137 (C++ int() truncates toward zero, as Python's)
    image_height = 1 if image_height < 1 else image_height   # Camera.txt:138
    theta = vfov * pi / 180.0
    h = math.tan(theta / 2)
    viewport_height = 2 * h * focus_dist
    viewport_width = viewport_height * (float(W) / image_height)
    w = unit(sub(lookfrom, lookat))
    u = unit(cross(vup, w))
    v = cross(w, u)
    viewport_u = mul(viewport_width, u)
    viewport_v = mul(viewport_height, [-v[0], -v[1], -v[2]])
    du, dv = div(viewport_u, W), div(viewport_v, image_height)
    upper_left = sub(sub(sub(lookfrom, mul(focus_dist, w)), div(viewport_u, 2)), div(viewport_v, 2))
    pixel00 = add(upper_left, mul(0.5, add(du, dv)))
    defocus_radius = focus_dist * math.tan((defocus_angle / 2) * pi / 180.0)
    return image_height, pixel00, du, dv, mul(defocus_radius, u), mul(defocus_radius, v)


def test_camera_derive_follows_initialize_over_odd_widths_and_aspects(rt):
    """camera::derive() vs Camera.txt:136-175: image_height = int(image_width / aspect_ratio) with the `< 1 -> 1` rule
    (Camera.txt:137-138) over widths and aspect ratios where the division does not come out whole, and the derived
    viewport vectors bit for bit.  (Camera.txt itself includes windows.h and cannot be compiled here; this is its text
    restated literally, not the build's own code.)"""
    rng = np.random.default_rng(20251004)
    cases = [(1024, 16.0 / 9.0), (1920, 16.0 / 9.0), (400, 16.0 / 9.0), (800, 1.0), (1, 1.0), (1, 16.0 / 9.0), (3, 7.0), (2, 2.5), (5, 1e6), (7, 0.013),
             (1279, 2.39), (1000, 3.0), (999, 3.0), (1001, 3.0), (854, 1.7777), (64, 64.0), (63, 64.0), (65, 64.0)]
    cases += [(int(rng.integers(1, 4000)), float(rng.uniform(0.05, 40.0))) for _ in range(200)]
    view = dict(vfov=37.5, lookfrom=(13.0, 2.0, 3.0), lookat=(0.25, -0.5, 0.125), vup=(0.1, 1.0, -0.05), defocus_angle=0.6, focus_dist=9.75)
    heights = set()
    for W, aspect in cases:
        cam = rt.derive_camera(W, aspect, spp=7, max_depth=3, **view)
        H, p00, du, dv, ddu, ddv = _initialize_literal(W, aspect, view["vfov"], list(view["lookfrom"]), list(view["lookat"]), list(view["vup"]),
                                                         view["defocus_angle"], view["focus_dist"])
        assert cam.image_width == W and cam.image_height == H == max(1, int(W / aspect)), (W, aspect)
        heights.add(H)
        for got, want in ((cam.pixel00_loc, p00), (cam.pixel_delta_u, du), (cam.pixel_delta_v, dv), (cam.defocus_disk_u, ddu), (cam.defocus_disk_v, ddv)):
            assert [got.x, got.y, got.z] == want, (W, aspect)          # same doubles, not merely close
        assert [cam.center.x, cam.center.y, cam.center.z] == list(view["lookfrom"]) and cam.pixel_samples_scale == 1.0 / 7
        assert cam.samples_per_pixel == 7 and cam.max_depth == 3 and cam.defocus_angle == 0.6
    assert 1 in heights and len(heights) > 100     # the clamp to 1 was exercised (W / aspect < 1) as well as many truncations


@pytest.mark.parametrize("case", IMAGE_CASES, ids=[c[0] for c in IMAGE_CASES])
def test_flattened_scene_is_byte_identical_to_the_reference_graph(rt, case):
    """The drop-in API + flattener against the description dumped from the reference's own
    objects (bvh topology from std::sort, perlin tables, texture bytes, random scenes)."""
    name = case[0]
    golden = json.load(open(os.path.join(GOLDEN, "desc_sha256.json")))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, name + ".rtks")
        rt.Scene.build(name, SCENE_SEED, scene_file(name, GOLDEN)).save(path)
        mine = open(path, "rb").read()
        assert hashlib.sha256(mine).hexdigest() == golden[name]
        from oracle import orc

        if os.path.exists(orc.REF_DRIVER):  # live check where the reference is available
            ref_path = os.path.join(tmp, name + "_ref.rtks")
            subprocess.check_call([orc.REF_DRIVER, "desc", name, str(SCENE_SEED), scene_file(name, GOLDEN), ref_path], stderr=subprocess.DEVNULL)
            assert open(ref_path, "rb").read() == mine


def test_scene_save_load_roundtrip(rt):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "a.rtks"), os.path.join(tmp, "b.rtks")
        rt.Scene.build("cornell_smoke").save(a)
        rt.Scene.load(a).save(b)
        assert open(a, "rb").read() == open(b, "rb").read()
    assert not os.path.exists("/nonexistent")
    with pytest.raises(ValueError):
        rt.Scene.build("no_such_scene")


def test_scene_construction_is_seeded(rt):
    with tempfile.TemporaryDirectory() as tmp:
        out = []
        for seed in (SCENE_SEED, SCENE_SEED, 7):
            p = os.path.join(tmp, f"s{len(out)}.rtks")
            rt.Scene.build("book1_final", seed).save(p)
            out.append(open(p, "rb").read())
        assert out[0] == out[1] and out[0] != out[2]


def test_tiling_roundtrip_and_counts(rt):
    from raytracingoneweekendapplication_amd import tiling

    rng = np.random.default_rng(0)
    for (w, h) in ((64, 36), (61, 35), (8, 8), (1, 1), (1920, 1080)):
        for n in (1, 2, 3, 8):
            tpr = tiling.tiles_per_rank(w, h, n)
            assert tpr == rt.tiles_per_rank(w, h, n)
            assert tpr * n >= ((w + 7) // 8) * ((h + 7) // 8) > (tpr - 1) * n
    img = rng.random((35, 61, 3))
    for n in (1, 2, 3, 5):
        parts = np.stack([tiling.compact_from_image(img, r, n) for r in range(n)])
        assert np.array_equal(tiling.image_from_gathered(parts, 61, 35, n), img)


def test_byte_model(rt):
    counters = dict.fromkeys(rt.COUNTER_FIELDS, 0)
    counters.update(samples=10, box_tests=1000, sphere_tests=100, surface_hits=20)
    f32 = rt.algorithmic_bytes_per_sample(counters, 100, rt.RTK_REAL_F32)
    f64 = rt.algorithmic_bytes_per_sample(counters, 100, rt.RTK_REAL_F64)
    assert f32 == pytest.approx((32 * 1000 + 32 * 100 + 32 * 20) / 10 + 12 / 100)
    assert f64 == pytest.approx((56 * 1000 + 60 * 100 + 48 * 20) / 10 + 24 / 100)


def test_synthetic_earth_texture_is_deterministic(rt):
    with tempfile.TemporaryDirectory() as tmp:
        a = open(rt.write_synthetic_earth(os.path.join(tmp, "a.ppm"), 64, 32), "rb").read()
        b = open(rt.write_synthetic_earth(os.path.join(tmp, "b.ppm"), 64, 32), "rb").read()
    assert a == b and a.startswith(b"P6\n64 32\n255\n") and len(a) == 13 + 64 * 32 * 3


def test_reference_style_program_compiles_and_links_against_the_drop_in_headers(rt, tmp_path):
    """Scene code in the reference's style (examples/) builds against host/ + include/ and links librtk_hip.so;
    without a GPU, camera::render reports the missing device instead of rendering on the host."""
    exe = tmp_path / "scene"
    pkg = os.path.dirname(rt.HIP_LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "examples", "reference_style_scene.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", str(exe)])
    import torch

    if not torch.cuda.is_available():
        out = subprocess.run([str(exe), "32", "1"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert "camera::render failed" in out.stderr and "no HIP device" in out.stderr
        assert not (tmp_path / "reference_style_scene.png").exists()


def test_obj_loader_matches_reference_on_its_own_asset(rt, tmp_path):
    """mesh::loadObj (host/mesh.h + the minimal GLM) against the reference's loader on the reference's monkey.obj
    (968 triangles, rotate/scale/translate transform), stored as tests/golden/monkey.obj with the sha256 of the description
    the reference's loader gives for it (make_goldens.py --assets); where oracle/_ref is built it is compared live as well."""
    from oracle import orc

    asset = os.path.join(GOLDEN, "monkey.obj")
    want = json.load(open(os.path.join(GOLDEN, "reference_assets.json")))["obj_desc_sha256"]["monkey.obj"]
    mine = tmp_path / "mine.rtks"
    rt.Scene.build("obj_mesh", SCENE_SEED, asset).save(str(mine))
    blob = mine.read_bytes()
    assert hashlib.sha256(blob).hexdigest() == want
    assert np.frombuffer(blob[8:8 + 64], np.int32)[5] == 968  # n_triangles
    if os.path.exists(orc.REF_DRIVER):
        ref = tmp_path / "ref.rtks"
        subprocess.check_call([orc.REF_DRIVER, "desc", "obj_mesh", str(SCENE_SEED), asset, str(ref)], stderr=subprocess.DEVNULL)
        assert blob == ref.read_bytes()


def test_the_library_is_loaded_after_torch_so_that_one_hip_runtime_serves_both():
    """A PyTorch-ROCm wheel carries its own libamdhip64; a process whose first HIP call came from /opt/rocm's copy (through
    librtk_hip.so) finds torch.cuda without devices afterwards.  The package therefore imports torch (where installed) before it
    loads its library -- checked in a fresh interpreter that never mentions torch itself."""
    code = ("import sys, raytracingoneweekendapplication_amd as rt\n"
            "assert 'torch' not in sys.modules\n"
            "rt.hip_lib()\n"
            "import importlib.util\n"
            "assert ('torch' in sys.modules) == (importlib.util.find_spec('torch') is not None)\n")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
