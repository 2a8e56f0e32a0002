"""GPU tests (-m gpu): the HIP kernels, called through the C ABI of include/rtk.h, against the CPU
oracle on the same seeded inputs, against the golden framebuffers rendered through the reference's
own classes, and -- at BASELINE.json's full sizes -- through size-independent properties.

Tolerances
  f64 kernels (the parity mode, the reference's arithmetic type): the north star's bar is a
      per-channel RMSE < 1e-4 against the CPU at matched seed.  The kernel evaluates the same
      double-precision operations in the same order as the oracle except for (a) the iterative
      radiance sum (Camera.txt:232-235 recursion unrolled) and (b) sample chunks added in chunk
      order, so the observed RMSE is ~1e-17; the tests assert < 1e-12 (and < 1e-4 is implied).
      Work counters (box/primitive tests, segments, RNG draws ...) are integers and must be EQUAL.
  f32 kernels (throughput mode): float rounding flips hit/miss branches, after which paths are
      unrelated (the reference's own code in float differs by RMSE 3-5e-3 at 16 spp).
      Here images are held to statistical agreement: image mean within 2 %, work-counter totals within 10 %.
      The f32 device functions (hit, scatter / emitted, texture::value, get_ray) are pinned case by case against
      the reference's known answers, and per-pixel coherence with the f64 kernel at 1 spp, in test_f32_parity.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import EARTH, GOLDEN, ROOT
from tests.scene_cases import IMAGE_CASES, RENDER_SEED, SCENE_SEED, scene_file

pytestmark = pytest.mark.gpu

F64_RMSE_BOUND = 1e-12   # observed ~1e-17; the north-star bar is 1e-4


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def _assert_culling_counters(got, exact, slack=0.03):
    """Work counters of a kernel that culls with CONSERVATIVE f32 boxes (the MIXED program) against the exact counters
    of the same hierarchy (oracle / f64-box kernel): everything a closest hit determines -- samples, segments, surface
    interactions, RNG draws -- is an equal integer; box and primitive tests can only be MORE (an enlarged box admits a
    superset of rays, and an extra primitive test never produces a hit), by about one per cent (C2 at full size: +0.66 %
    box tests, +1.03 % sphere tests -- the 2^-19 x extent margin is 1 % of a radius-0.2 sphere's box).  `slack`: scenes whose
    coordinates run into the hundreds (the Cornell box: extent 2 600, margin 0.005) need more -- there the margin exceeds the
    1e-4 thickness of a quad's own box (aabb.h:98-105) and the t_min = 0.001 that keeps a ray from re-hitting the surface it
    leaves (Camera.txt:211), so every ray leaving a wall enters that wall's box again (+7 % box tests, +15 % quad tests)."""
    for key in ("samples", "segments", "surface_hits", "rng_draws", "noise_calls", "texel_fetches"):
        assert got[key] == exact[key], key
    for key in ("box_tests", "sphere_tests", "quad_tests", "triangle_tests", "xform_enters", "medium_tests"):
        assert exact[key] <= got[key] <= exact[key] * (1.0 + slack) + 16, (key, got[key], exact[key])


@pytest.fixture(scope="module")
def scenes(rt):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rt.Scene.build(name, SCENE_SEED, scene_file(name, GOLDEN))
        return cache[name]
    return get


def test_extension_is_the_code_that_runs(rt, renderer):
    """The render path is librtk_hip.so on a gfx950 device -- nothing else can serve it."""
    import torch

    assert torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    # the library that serves the calls is the in-tree build, by its resolved path (a substitute named through RTK_HIP_LIB
    # would also contain "librtk_hip" in its name: compare paths, not substrings)
    assert os.path.realpath(rt.HIP_LIB_PATH) == os.path.realpath(rt.DEFAULT_HIP_LIB_PATH)
    loaded = {os.path.realpath(line.split()[-1]) for line in open("/proc/self/maps") if line.rstrip().endswith(".so") and "/" in line}
    assert os.path.realpath(rt.DEFAULT_HIP_LIB_PATH) in loaded


@pytest.mark.parametrize("case", IMAGE_CASES, ids=[c[0] for c in IMAGE_CASES])
def test_f64_kernel_matches_oracle_and_reference_goldens(rt, orc, renderer, scenes, case):
    name, W, H, spp, depth = case
    scene = scenes(name)
    cam = scene.camera(W, H, spp, depth)
    renderer.upload(scene)
    gpu, gpu8, counters = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, count=True)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, RENDER_SEED, 8)
    assert rmse(gpu, ref) < F64_RMSE_BOUND
    assert np.array_equal(gpu8, ref8)                      # Camera.txt:77-89 bytes
    assert counters == ocnt                                # identical traversal, shading and RNG consumption
    golden = np.load(os.path.join(GOLDEN, f"img_{name}.npz"), allow_pickle=False)
    assert rmse(gpu, golden["linear"]) < F64_RMSE_BOUND    # framebuffer from the reference's own classes
    assert np.array_equal(gpu8, golden["rgb8"])
    assert [counters["rng_draws"], counters["segments"], counters["surface_hits"]] == golden["counts"].tolist()
    # the fast (non-counting) instantiation computes the same image, with the program in LDS or in global memory
    fast, fast8, _ = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64)
    glob, _, _ = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, variant=1)
    assert np.array_equal(fast, gpu) and np.array_equal(fast8, gpu8) and np.array_equal(glob, gpu)


@pytest.mark.parametrize("name", ["three_spheres", "book1_final", "cornell_box", "material_zoo"])
def test_f32_kernel_agrees_statistically(rt, orc, renderer, scenes, name):
    scene = scenes(name)
    cam = scene.camera(96, 54, 32, 0)
    renderer.upload(scene)
    gpu, _, counters = renderer.render_host(cam, real_mode=rt.RTK_REAL_F32, count=True)
    ref, _, ocnt = orc.render(scene.desc_ptr, cam, RENDER_SEED, 8)
    assert abs(gpu.mean() - ref.mean()) < 0.02 * ref.mean()
    assert rmse(gpu, ref) < 0.1 * max(ref.std(), 1e-3) + 0.02
    # float self-intersections at t_min = 0.001 on the radius-1000 ground sphere add bounces (SURVEY.md 8(d):
    # "acne"), so the work totals agree only to several per cent
    for key in ("segments", "box_tests", "rng_draws"):
        assert abs(counters[key] - ocnt[key]) < 0.10 * ocnt[key], key
    assert counters["samples"] == ocnt["samples"]


def test_sample_chunking_changes_only_the_summation_order(rt, orc, renderer, scenes):
    scene = scenes("book1_final")
    cam = scene.camera(64, 40, 50, 50)          # 50 spp -> 6 chunks of 8 and one of 2
    renderer.upload(scene)
    chunked, _, c1 = renderer.render_host(cam, count=True)
    single, _, c2 = renderer.render_host(cam, count=True, variant=2)   # one lane per pixel for all samples
    ref, _, ocnt = orc.render(scene.desc_ptr, cam, RENDER_SEED, 8)
    assert c1 == c2 == ocnt
    assert rmse(single, ref) < F64_RMSE_BOUND and rmse(chunked, ref) < F64_RMSE_BOUND
    assert np.abs(chunked - single).max() < 1e-14


@pytest.mark.parametrize("shape", [(8, 8, 1, 1), (1, 1, 3, 5), (13, 7, 2, 50), (65, 9, 17, 3), (40, 24, 9, 1)])
def test_ragged_sizes_and_degenerate_settings(rt, orc, renderer, scenes, shape):
    """Images that are not a multiple of the 8x8 tile, a single pixel, spp not a multiple of the chunk, depth 1."""
    W, H, spp, depth = shape
    scene = scenes("three_spheres")
    cam = scene.camera(W, H, spp, depth)
    renderer.upload(scene)
    gpu, gpu8, counters = renderer.render_host(cam, count=True)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, RENDER_SEED, 2)
    assert gpu.shape == (H, W, 3)
    assert rmse(gpu, ref) < F64_RMSE_BOUND and np.array_equal(gpu8, ref8) and counters == ocnt


def test_max_depth_zero_renders_black_like_the_reference(rt, orc, renderer, scenes):
    """ray_color returns (0,0,0) before any hit test when depth <= 0 (Camera.txt:205-206)."""
    scene = scenes("three_spheres")
    cam = scene.camera(24, 16, 3, 1)
    cam.max_depth = 0
    renderer.upload(scene)
    gpu, gpu8, counters = renderer.render_host(cam, count=True)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, RENDER_SEED, 2)
    assert not gpu.any() and not ref.any() and not gpu8.any()
    assert counters == ocnt and counters["segments"] == 0 and counters["samples"] == 24 * 16 * 3


def test_seed_and_determinism(rt, renderer, scenes):
    scene = scenes("cornell_smoke")
    cam = scene.camera(48, 48, 8, 10)
    renderer.upload(scene)
    a, _, _ = renderer.render_host(cam, seed=5)
    b, _, _ = renderer.render_host(cam, seed=5)
    c, _, _ = renderer.render_host(cam, seed=6)
    assert np.array_equal(a, b)          # run-to-run bit-identical (RNG keyed by pixel and sample only)
    assert not np.array_equal(a, c)
    # `b` was rendered in the tile order learned from `a` (most expensive tiles first), `d` in fixed row-major order:
    # the order in which tiles are handed to waves must never show in the image
    d, _, _ = renderer.render_host(cam, seed=5, variant=4)
    assert np.array_equal(a, d)


@pytest.mark.parametrize("n_ranks,real", [(2, "f64"), (3, "f64"), (8, "f64"), (4, "f32")])
def test_tile_sharding_is_bit_identical_to_one_gpu(rt, renderer, scenes, n_ranks, real):
    """P4 of SURVEY.md 8(d): the image must not depend on the GPU count.  All ranks run on this one
    device into their compact buffers; the gather is emulated by stacking (the real one is
    torch.distributed.gather over RCCL, covered on CPU/gloo by test_distributed_cpu.py)."""
    import torch
    from raytracingoneweekendapplication_amd import tiling

    scene = scenes("book1_final")
    cam = scene.camera(100, 60, 8, 50)   # 13 x 8 = 104 tiles: not a multiple of 3 or 8 -> padded last tiles
    renderer.upload(scene)
    mode = rt.RTK_REAL_F64 if real == "f64" else rt.RTK_REAL_F32
    dtype = torch.float64 if real == "f64" else torch.float32
    whole, whole8, _ = renderer.render_host(cam, real_mode=mode)
    dev = torch.device("cuda", 0)
    tpr = tiling.tiles_per_rank(100, 60, n_ranks)
    parts = []
    for rank in range(n_ranks):
        buf = torch.full((tpr, 3, 64), float("nan"), dtype=dtype, device=dev)
        renderer.render_device(cam, buf.data_ptr(), 0, real_mode=mode, rank=rank, n_ranks=n_ranks)
        parts.append(buf)
    gathered = torch.stack(parts).contiguous()
    image = torch.empty((60, 100, 3), dtype=dtype, device=dev)
    rgb8 = torch.empty((60, 100, 3), dtype=torch.uint8, device=dev)
    renderer.unpermute(100, 60, n_ranks, mode, gathered.data_ptr(), image.data_ptr(), rgb8.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().astype(np.float64), whole)
    assert np.array_equal(rgb8.cpu().numpy(), whole8)
    # and the device layout is the one the CPU/gloo path assumes
    assert np.array_equal(tiling.image_from_gathered(gathered.cpu().numpy(), 100, 60, n_ranks).astype(np.float64), whole)


def test_error_behaviour(rt, renderer, scenes, tmp_path):
    fresh = rt.Renderer(0)
    cam = scenes("three_spheres").camera(16, 16, 1, 2)
    with pytest.raises(rt.RtkError) as e:
        fresh.render_host(cam)
    assert e.value.code == -5            # RTK_ERR_NO_SCENE
    # an empty world: the reference recurses forever (bvh.h:38-43); the ABI reports it
    empty = tmp_path / "empty.rtks"
    head = np.zeros(16, np.int32)
    head[0] = 0
    head[1] = 1                          # one node ...
    node = np.array([4, 0, 0, 0], np.int32)   # ... an empty hittable_list
    empty.write_bytes(b"RTKSCN1\0" + head.tobytes() + np.int64(0).tobytes() + node.tobytes())
    with pytest.raises(rt.RtkError) as e:
        fresh.upload(rt.Scene.load(str(empty)))
    assert e.value.code == -1            # RTK_ERR_INVALID
    bad = tmp_path / "bad.rtks"
    node = np.array([1, 5, 0, 0], np.int32)   # sphere index out of range
    bad.write_bytes(b"RTKSCN1\0" + head.tobytes() + np.int64(0).tobytes() + node.tobytes())
    with pytest.raises(rt.RtkError):
        fresh.upload(rt.Scene.load(str(bad)))
    fresh.upload(scenes("three_spheres"))
    with pytest.raises(rt.RtkError):
        fresh.render_device(cam, 0, 0, rank=3, n_ranks=2)


# ------------------------------------------------------------------ BASELINE sizes
def _full_size_checks(rt, orc, renderer, scene, cam, n_probe=48, probe_seed=1234):
    """Full-size render checked through properties that do not need a full CPU render:
    exact per-pixel agreement with the oracle on a random pixel subset (every pixel is an
    independent function of (scene, camera, seed, pixel)), exact sample count, and invariance
    under tile sharding."""
    import ctypes as C
    import torch

    W, H, spp = cam.image_width, cam.image_height, cam.samples_per_pixel
    dev = torch.device("cuda", 0)
    image = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
    renderer.render_device(cam, image.data_ptr(), 0)
    torch.cuda.synchronize()
    img = image.cpu().numpy()
    assert np.isfinite(img).all() and (img >= 0).all()
    rng = np.random.default_rng(probe_seed)
    rgb = (C.c_double * 3)()
    worst = 0.0
    for _ in range(n_probe):
        i, j = int(rng.integers(0, W)), int(rng.integers(0, H))
        acc = np.zeros(3)
        for s in range(spp):
            orc.lib().orc_sample(scene.desc_ptr, C.addressof(cam), RENDER_SEED, i, j, s, C.addressof(rgb), None)
            acc = acc + np.array(rgb[:])
        worst = max(worst, float(np.abs(acc * cam.pixel_samples_scale - img[j, i]).max()))
    assert worst < 1e-12, worst
    return img


def test_config2_full_size_properties(rt, orc, renderer, scenes):
    """BASELINE configs[1]: book-1 final scene 1920x1080x100, depth 50."""
    scene = scenes("book1_final")
    cam = scene.camera()
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth) == (1920, 1080, 100, 50)
    renderer.upload(scene)
    img = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=1024)
    # furnace bound: every albedo <= 1 and nothing emits, so no pixel can exceed the background colour
    assert (img <= np.array([0.7, 0.8, 1.0]) + 1e-12).all()
    assert 0.2 < img.mean() < 0.6
    # ... and THE KERNEL bench.py TIMES: fast order + MIXED program (rtk_render_kernel<double, 256u, false, true>) at
    # the headline size, probed against the oracle's per-sample values of the reference scene; same bytes as above
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"] and renderer.kernel_name() == "rtk_render_kernel<double, 256u, false, true>"
    timed = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=1024, probe_seed=99)
    assert np.array_equal(timed, img)
    # its counting build at full size against the exact counters of the same hierarchy (f64-box counting kernel)
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.empty((1080, 1920, 3), dtype=torch.float64, device=dev)
    got = []
    for variant in (0, 1 << 20):
        cnt = torch.zeros(12, dtype=torch.int64, device=dev)
        renderer.render_device(cam, buf.data_ptr(), 0, d_counters=cnt.data_ptr(), variant=variant)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), img)
        got.append(dict(zip(rt.COUNTER_FIELDS, cnt.tolist())))
    assert got[0]["samples"] == 1920 * 1080 * 100
    _assert_culling_counters(got[0], got[1])


def test_config1_and_config3_reduced_spp_properties(rt, orc, renderer, scenes):
    """configs[0] at full size; configs[2] (Cornell 800x800) at 16 of its 1000 spp (same kernel,
    same per-sample work; the full 640 M samples are a bench workload, not a test)."""
    scene = scenes("three_spheres")
    cam = scene.camera()
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (400, 225, 10)
    renderer.upload(scene)
    _full_size_checks(rt, orc, renderer, scene, cam, n_probe=64)
    scene = scenes("cornell_box")
    cam = scene.camera(800, 800, 16, 25)
    renderer.upload(scene)
    img = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=32)
    assert img.max() <= 15.0 + 1e-9     # nothing can be brighter than the light (emit 15)


def test_config4_and_config5_full_resolution_reduced_spp_properties(rt, orc, renderer, scenes):
    """configs[3] (triangle mesh, 1920x1080) and configs[4] (book-2 final: media, Perlin, motion blur, image texture,
    instances; 1920x1080) at full resolution and 8 of their 256 / 1000 spp, in the reference order (boxes-in-LDS kernels,
    the programs do not fit LDS) and in the fast order bench.py times: exact per-pixel agreement with the oracle on random
    pixels, finiteness, brightness bounds the scenes imply, and the same doubles from both orders."""
    scene = scenes("mesh")
    cam = scene.camera(0, 0, 8, 0)
    assert (cam.image_width, cam.image_height, cam.max_depth) == (1920, 1080, 10)
    renderer.upload(scene)
    assert "false, false" in renderer.kernel_name() and int(renderer.kernel_name().split(",")[1].strip(" u")) & 1024   # F_LDS_BOXES
    img = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=32)
    assert img.mean() > 0.01
    # the fast order renders the same bytes at this size too (not provable for triangles: float determinant, triangle.h:72,77)
    renderer.upload_fast(scene, cam.center)
    fast = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=8, probe_seed=5)
    assert np.array_equal(fast, img)
    scene = scenes("book2_final")
    cam = scene.camera(0, 0, 8, 0)
    assert (cam.image_width, cam.image_height, cam.max_depth) == (1920, 1080, 10)
    renderer.upload(scene)
    assert "1151u" in renderer.kernel_name()
    img = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=32)
    assert img.max() <= 7.0 + 1e-9 and img.mean() > 0.005    # nothing is brighter than the light (emit 7, main.cpp:292)
    # ... and as bench.py times it: the fast order with the two media at their positions in the reference's visiting order
    # (the hot part of the COMPACT program in LDS, the 2 400 quads in memory: F_LDS_BOXES | F_F32_BOX | full feature set) -- the
    # very same doubles, 2 M pixels x 8 samples
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"] and info["has_media"] and info["n_ordered_items"] == 2 and "3455u" in renderer.kernel_name()   # hot/cold COMPACT, sphere media only
    # ... as does the slot program with its boxes in LDS (variant bit 20: f64 boxes, fused slab test)
    assert "1279u" in renderer.kernel_name(variant=1 << 20)
    import torch
    slot = torch.empty((1080, 1920, 3), dtype=torch.float64, device=torch.device("cuda", 0))
    renderer.render_device(cam, slot.data_ptr(), 0, variant=1 << 20)
    torch.cuda.synchronize()
    assert np.array_equal(slot.cpu().numpy(), img)
    fast = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=8, probe_seed=5)
    assert np.array_equal(fast, img)


def test_frames_with_many_sample_chunks_are_rendered_in_passes_with_the_same_sums(rt, orc, renderer, scenes):
    """More sample chunks than the partial-sum workspace (budget: 1.095 GB per context = 22 planes of a 1920x1080 f64 frame) holds
    planes for: the frame is rendered in passes over the chunks, the resolve kernel carrying every pixel's running sum from
    pass to pass (1000 spp at 1920x1080 used to take 63 planes, 3.1 GB).  The additions are those of one pass over all chunks,
    in the same order: the image must be the one-launch image (variant bit 24) bit for bit -- whole and sharded over ranks
    (a rank's share fits the budget: one launch) -- and the oracle's on probed pixels; progress reports of a blocking render
    add the passes up monotonically.  A frame of 1024x704 with 64 chunks of 2 samples (variant bits 3-4) is 1.107 GB of
    planes: 62 + 2."""
    import ctypes as C

    import torch

    scene = scenes("book1_final")
    W, H, spp = 1024, 704, 128
    cam = scene.camera(W, H, spp, 6)
    CH2 = 2 << 3                                     # chunks of 2 samples: 64 chunks
    opts = rt.RenderOpts(RENDER_SEED, rt.RTK_REAL_F64, 0, 1, 0, CH2, None)
    assert rt.hip_lib().rtk_frame_launches(C.byref(cam), C.byref(opts)) == 2
    opts.variant = CH2 | (1 << 24)
    assert rt.hip_lib().rtk_frame_launches(C.byref(cam), C.byref(opts)) == 1
    opts.variant, opts.n_ranks = CH2, 3
    assert rt.hip_lib().rtk_frame_launches(C.byref(cam), C.byref(opts)) == 1           # a third of the tiles: everything fits
    full = scene.camera(1920, 1080, 1000, 10)
    opts = rt.RenderOpts(RENDER_SEED, rt.RTK_REAL_F64, 0, 1, 0, 0, None)
    assert rt.hip_lib().rtk_frame_launches(C.byref(full), C.byref(opts)) == 3          # C5's size: 21 + 21 + 21 of 63 chunks
    opts.n_ranks = 8
    assert rt.hip_lib().rtk_frame_launches(C.byref(full), C.byref(opts)) == 1          # ... and one launch on an eighth of it
    renderer.upload_fast(scene, cam.center)
    dev = torch.device("cuda", 0)
    image = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    bytes8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    renderer.render_device(cam, image.data_ptr(), bytes8.data_ptr(), variant=CH2)
    torch.cuda.synchronize()
    passes, passes8 = image.cpu().numpy().copy(), bytes8.cpu().numpy().copy()
    renderer.render_device(cam, image.data_ptr(), bytes8.data_ptr(), variant=CH2 | (1 << 24))
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy(), passes) and np.array_equal(bytes8.cpu().numpy(), passes8)
    rng = np.random.default_rng(5)
    rgb = (C.c_double * 3)()
    for _ in range(12):                              # the oracle's per-sample values of random pixels, summed in chunk order
        i, j = int(rng.integers(0, W)), int(rng.integers(0, H))
        total = np.zeros(3)
        for c0 in range(0, spp, 2):
            part = np.zeros(3)
            for s_ in range(c0, c0 + 2):
                orc.lib().orc_sample(scene.desc_ptr, C.addressof(cam), RENDER_SEED, i, j, s_, C.addressof(rgb), None)
                part = part + np.array(rgb[:])
            total = part if c0 == 0 else total + part
        assert np.abs(total * cam.pixel_samples_scale - passes[j, i]).max() < 1e-12, (i, j)   # (the oracle multiplies attenuations recursively, the kernel iteratively: ~1e-17)
    tpr = rt.tiles_per_rank(W, H, 3)
    gathered = torch.zeros((3, tpr, 3, 64), dtype=torch.float64, device=dev)
    for rank in range(3):
        renderer.render_device(cam, gathered[rank].data_ptr(), 0, rank=rank, n_ranks=3, variant=CH2)
    renderer.unpermute(W, H, 3, rt.RTK_REAL_F64, gathered.data_ptr(), image.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy(), passes)
    small = scene.camera(128, 64, 16, 6)             # a blocking render of a small frame forced into passes: progress adds them up
    seen = []
    renderer.set_progress(lambda done, total: seen.append((done, total)), interval_ms=1)
    a_img, a8, _ = renderer.render_host(small, variant=CH2)
    renderer.set_progress(None)
    n_items = (128 // 8) * (64 // 8) * 8
    assert seen and seen[-1] == (n_items, n_items) and all(0 <= a[0] <= b[0] <= b[1] for a, b in zip(seen, seen[1:]))


FULL_SIZE_CONFIGS = [
    # config, scene, (W, H, spp, depth), substring of the timed kernel's name
    ("c3", "cornell_box", (800, 800, 1000, 25), "837u"),
    ("c4", "mesh", (1920, 1080, 256, 10), "834u"),
    ("c5", "book2_final", (1920, 1080, 1000, 10), "3455u"),   # full feature | F_F32_BOX | F_LDS_BOXES | F_SPHERE_MEDIA_ONLY
]


@pytest.mark.parametrize("case", FULL_SIZE_CONFIGS, ids=[c[0] for c in FULL_SIZE_CONFIGS])
def test_configs_3_4_5_at_their_stated_sizes(rt, orc, renderer, tmp_path, case):
    """BASELINE configs[2..4] at the sizes BASELINE.json states -- Cornell box 800x800x1000, mesh 1920x1080x256, book-2 final
    1920x1080x1000 -- in the order and with the kernels bench.py times: 512 random pixels checked against the oracle over ALL
    of their samples (orc_sample on the reference's own hierarchy), the whole frame equal to the reference-order render of
    the same size, double for double, and its SHA-256 equal to the constant bench.py also checks (bench.PINNED_SHA256)."""
    import hashlib
    import json

    import bench
    from tests.conftest import ROOT

    cfg, name, (W, H, spp, depth), kernel_tag = case
    # the scene exactly as bench.py builds it (its procedural 1024x512 earth texture, not the small golden one)
    scene = rt.Scene.build(name, rt.SCENE_SEED, rt.write_synthetic_earth(str(tmp_path / "earth_synth.ppm")))
    cam = scene.camera()
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth) == (W, H, spp, depth)
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"] and kernel_tag in renderer.kernel_name(), renderer.kernel_name()
    assert info["proven"] == (name != "mesh")   # triangles: identical by measurement (this test), not by proof
    fast = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=512, probe_seed=2026)
    renderer.upload(scene)
    ref = _full_size_checks(rt, orc, renderer, scene, cam, n_probe=4, probe_seed=7)
    assert np.array_equal(fast, ref)
    sha = hashlib.sha256(fast.tobytes()).hexdigest()[:16]
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"full_size_sha_{cfg}.json"), "w") as f:
        json.dump({"config": cfg, "scene": name, "size": [W, H, spp, depth], "framebuffer_sha256": sha}, f)
    assert bench.PINNED_SHA256.get(cfg) == sha, (cfg, sha, bench.PINNED_SHA256.get(cfg))


def test_device_hit_records_match_reference_known_answers(rt, renderer, tmp_path):
    """Function-level parity ON THE DEVICE: hittable::hit of every object kind (static/moving/huge spheres,
    quads, triangles with UVs, boxes, rotate_y/translate instances, constant media incl. the span-1 double
    test, a 37-sphere bvh) for ~3000 reference-generated rays with arbitrary (tmin, tmax) -- including rays
    with a zero direction component and origins on slab planes (1/0 = inf, 0*inf = NaN in aabb::hit) --
    through the same device traversal and deferred hit-record code the render kernel uses.
    Expected values come from the reference's own classes (tests/golden/kat_hit_*.npy)."""
    inp = np.load(os.path.join(GOLDEN, "kat_hit_in.npy"))
    out = np.load(os.path.join(GOLDEN, "kat_hit_out.npy"))
    meta = np.load(os.path.join(GOLDEN, "kat_hit_meta.npy"))
    blob = bytearray(open(os.path.join(GOLDEN, "kat_scene.rtks"), "rb").read())
    n_exact = n_hits = 0
    for node in np.unique(meta[:, 0]):
        rows = np.nonzero(meta[:, 0] == node)[0]
        blob[8:12] = np.int32(node).tobytes()          # make this object the scene root
        path = tmp_path / f"obj_{int(node)}.rtks"
        path.write_bytes(bytes(blob))
        renderer.upload(rt.Scene.load(str(path)))
        rays = inp[rows]                                # o(3) d(3) time tmin tmax
        keys = np.stack([np.full(len(rows), 7), meta[rows, 1], meta[rows, 2]], 1)
        got, draws = renderer.closest_hit(rays, keys)
        expect = out[rows]
        assert np.array_equal(got[:, 0], expect[:, 0]), int(node)              # hit / miss decisions
        assert np.array_equal(draws.astype(np.int64), meta[rows, 3]), int(node)  # RNG draws inside hit()
        hit = expect[:, 0] == 1
        g, e = got[hit, 1:], expect[hit, 1:]
        assert np.array_equal(g[:, 7], e[:, 7]) and np.array_equal(g[:, 10], e[:, 10])   # front_face, material
        scale = np.maximum(1.0, np.abs(e[:, :7]))
        assert (np.abs(g[:, :7] - e[:, :7]) <= 1e-13 * scale).all(), int(node)             # t, p, normal
        assert (np.abs(g[:, 8:10] - e[:, 8:10]) <= 1e-13).all(), int(node)                 # u, v (acos/atan2: libm vs ocml ulps)
        n_exact += int((g[:, :7] == e[:, :7]).all(axis=1).sum())
        n_hits += int(hit.sum())
    assert n_hits > 800
    assert n_exact >= 0.95 * n_hits   # nearly all records are bit-identical; the rest differ by log()/ulps in media


# ---- function-level known answers for the shading side (rtk_debug_scatter / _texture / _get_ray) ----------------
def _load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def _close(got, want, tol=1e-13):
    """Equal, or within `tol` relative to the larger magnitude (libm vs device ulps of sin / pow / acos / atan2); NaN == NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        ok = (got == want) | both_nan | (np.abs(got - want) <= tol * np.maximum(np.maximum(np.abs(got), np.abs(want)), 1.0))
    return ok


def test_device_scatter_matches_reference_known_answers(rt, renderer):
    """Function-level parity ON THE DEVICE for material::scatter / emitted (material.h:22-172): the reference-generated vectors
    of tests/golden/kat_scatter_* (all seven material kinds, textured and not; made from the reference's own classes by
    make_goldens.py) through rtk_debug_scatter, i.e. through shade_surface -- the function the render kernel executes after it
    has built a hit record.  Scattered / absorbed decisions and RNG-draw counts equal; scattered ray, attenuation and emission
    within 1e-13 (bit-identical except where sin / pow / Perlin's floor differ from libm by an ulp -- counted below)."""
    scene = rt.Scene.load(os.path.join(GOLDEN, "kat_scene.rtks"))
    renderer.upload(scene)
    inp, out, meta = _load_golden("kat_scatter_in.npy"), _load_golden("kat_scatter_out.npy"), _load_golden("kat_scatter_meta.npy")
    keys = np.stack([np.full(len(meta), 7), meta[:, 1], meta[:, 2]], 1)     # KAT_SEED, pixel, sample
    got, draws = renderer.debug_scatter(meta[:, 0], inp[:, 0:7], inp[:, 7:18], keys)
    assert np.array_equal(got[:, 0], out[:, 0])                            # scattered or not, every case
    assert np.array_equal(draws.astype(np.int64), meta[:, 3].astype(np.int64))   # random_double() calls inside scatter()
    assert _close(got[:, 11:14], out[:, 11:14]).all()                      # emitted(u, v, p)
    sc = out[:, 0] == 1
    assert sc.sum() > len(out) // 3 and (~sc).sum() > 10                   # both outcomes are exercised
    assert _close(got[sc, 1:11], out[sc, 1:11]).all()                      # scattered ray (origin, direction), attenuation, time
    exact = (got[sc, 1:11] == out[sc, 1:11]) | (np.isnan(got[sc, 1:11]) & np.isnan(out[sc, 1:11]))
    assert exact.all(axis=1).mean() > 0.9, exact.all(axis=1).mean()        # nearly all cases bit for bit
    kinds = set(int(k) for k in meta[:, 0])
    assert len(kinds) >= 7                                                 # every material of the KAT scene took part


def test_device_texture_matches_reference_known_answers(rt, renderer):
    """texture::value (texture.h:20-120: solid, checker, checker for triangle UVs, image, Perlin noise with turbulence,
    perlin.h:14-50) on the device against the reference's values for the same (u, v, p)."""
    scene = rt.Scene.load(os.path.join(GOLDEN, "kat_scene.rtks"))
    renderer.upload(scene)
    inp, out, meta = _load_golden("kat_texture_in.npy"), _load_golden("kat_texture_out.npy"), _load_golden("kat_texture_meta.npy")
    got, work = renderer.debug_texture(meta[:, 0], inp[:, 0:5])
    assert _close(got, out).all(), np.abs(got - out).max()
    assert (got == out).all(axis=1).mean() > 0.9
    assert len(set(int(t) for t in meta[:, 0])) >= 5 and work[:, 0].max() >= 7 and work[:, 1].max() >= 1   # noise (7 octaves) and image lookups took part


def test_device_get_ray_matches_reference_known_answers(rt, renderer):
    """camera::get_ray (Camera.txt:177-200: sample_square, defocus_disk_sample's rejection loop, the ray time) on the device
    -- begin_sample, the function that starts every sample in the render kernel -- against the vectors generated from the
    restated Camera.txt on the reference side: origin, direction, time and draw counts, bit for bit."""
    out, meta, cams = _load_golden("kat_getray_out.npy"), _load_golden("kat_getray_meta.npy"), _load_golden("kat_getray_cams.npy")
    import ctypes as C
    for variant in sorted(set(int(v) for v in meta[:, 0])):
        rows = meta[:, 0] == variant
        cam = rt.Camera()
        raw = cams[variant]
        cam.image_width, cam.image_height = int(raw[0]), int(raw[1])
        cam.samples_per_pixel, cam.max_depth = 1, 1
        C.memmove(C.addressof(cam) + 16, raw[2:].astype(np.float64).tobytes(), C.sizeof(rt.Camera) - 16)
        got, draws = renderer.debug_get_ray(cam, 7, meta[rows][:, 1:4])
        assert np.array_equal(got, out[rows])
        assert np.array_equal(draws.astype(np.int64), meta[rows][:, 4].astype(np.int64))


# ---- the fast visiting order (rtk_scene_optimize) --------------------------------------
@pytest.mark.parametrize("case", IMAGE_CASES, ids=[c[0] for c in IMAGE_CASES])
def test_fast_order_on_the_device(rt, orc, renderer, scenes, case):
    """The re-grouped hierarchy through the same kernels: the device agrees with the oracle executing that
    hierarchy (image, bytes, every work counter), and -- where the pass claims exactness, and on the triangle
    scenes at these sizes -- with the reference-order image bit for bit."""
    name, W, H, spp, depth = case
    scene = scenes(name)
    cam = scene.camera(W, H, spp, depth)
    fast = scene.fast_order(cam.center)
    renderer.upload(fast)
    gpu, gpu8, counters = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, count=True)
    ref, ref8, ocnt = orc.render(fast.desc_ptr, cam, RENDER_SEED, 8)
    assert rmse(gpu, ref) < F64_RMSE_BOUND and np.array_equal(gpu8, ref8) and counters == ocnt
    # rtk_scene_upload_fast = the same hierarchy + the fused slab test (F_FMA_BOX kernels): conservative on the grown
    # boxes, so the same image; the slab decisions themselves coincide at these sizes, hence equal counters
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"] == fast.exact
    feat = int(renderer.kernel_name().split(",")[1].strip().rstrip("u"))
    # every f64 kernel of the fast order culls with f32 boxes (F_F32_BOX = 256): the MIXED program of sphere-only scenes
    # (feat == 256) or the COMPACT program of the other families; variant bit 20 keeps the f64 boxes of the slot program
    has_media = fast.info["has_media"]
    assert (feat & 256) or name == "book2_final"     # (a full-feature scene whose COMPACT program does not fit LDS stays on the slot program)
    slot_feat = int(renderer.kernel_name(variant=1 << 20).split(",")[1].strip().rstrip("u"))
    assert not (slot_feat & 256) and ((slot_feat & 128) or (slot_feat & ~(512 | 1024)) == 69)
    fused, fused8, fcnt = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, count=True)
    fused_fast, _, _ = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64)
    assert np.array_equal(fused, gpu) and np.array_equal(fused8, gpu8) and np.array_equal(fused_fast, gpu)
    # `count=True` ran a counting build on the f32-box program (the MIXED kernel's own; the full-feature kernel on a COMPACT
    # program): conservative culling -> a tight superset of the oracle's tests, equal closest-hit counters
    _assert_culling_counters(fcnt, counters, slack=0.25 if name.startswith("cornell") or name == "material_zoo" else (0.12 if "mesh" in name else 0.03))
    slot, slot8, exact_cnt = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, count=True, variant=1 << 20)   # f64 boxes
    assert exact_cnt == counters and np.array_equal(slot, gpu) and np.array_equal(slot8, gpu8)
    slot_fast, _, _ = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, variant=1 << 20)
    in_global, _, _ = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, variant=1)
    assert np.array_equal(slot_fast, gpu) and np.array_equal(in_global, gpu)
    # the hot/cold form of the COMPACT program (what programs larger than LDS run from: quads and triangles -- in runs, also
    # inside a medium's boundary and under instance transforms -- in memory, everything else in LDS): forced by variant bit
    # 23 on the scenes of the full-feature kernel family, which is the only one that has it
    cold_name = renderer.kernel_name(variant=1 << 23)
    if int(cold_name.split(",")[1].strip().rstrip("u")) & ~(2048 | 1024 | 256 | 128) == 127:
        # 1407 = full feature | F_F32_BOX | F_LDS_BOXES; + 2048 (F_SPHERE_MEDIA_ONLY) where every medium is sphere-bounded (book 2,
        # single_fog): the variant without the generic OP_MED_BEGIN / MID / END bracket and its parked query state
        assert ("3455u" in cold_name) == (name == "book2_final") and ("1407u" in cold_name) == (name != "book2_final")
        cold_img, cold8, _ = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, variant=1 << 23)
        assert np.array_equal(cold_img, gpu) and np.array_equal(cold8, gpu8)
    else:
        assert name in ("three_spheres", "book1_final", "cornell_box", "mesh", "obj_mesh")
    assert fast.exact   # media included: they keep their position in the reference's visiting order
    renderer.upload(scene)
    base, base8, bcnt = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64, count=True)
    assert np.array_equal(gpu, base) and np.array_equal(gpu8, base8)
    golden = np.load(os.path.join(GOLDEN, f"img_{name}.npz"), allow_pickle=False)
    assert rmse(gpu, golden["linear"]) < F64_RMSE_BOUND and np.array_equal(gpu8, golden["rgb8"])
    for key in ("samples", "segments", "surface_hits", "rng_draws"):
        assert counters[key] == bcnt[key], key
    if has_media:   # opts.free_media_order: media re-grouped like any other object -- another sample of the same estimator
        info = renderer.upload_fast(scene, cam.center, free_media_order=True)
        assert not info["exact"]
        free, _, _ = renderer.render_host(cam, seed=RENDER_SEED, real_mode=rt.RTK_REAL_F64)
        assert abs(free.mean() - gpu.mean()) < 0.08 * gpu.mean() + 1e-3
        assert name == "single_fog" or not np.array_equal(free, gpu)   # (a world of one medium has only one order)


def test_fast_order_full_resolution_book1_is_bit_identical_and_cheaper(rt, renderer, scenes):
    """BASELINE configs[1] at full resolution (reduced spp): same bytes from both orders, about half the slab tests."""
    import torch

    scene = scenes("book1_final")
    cam = scene.camera(1920, 1080, 8, 50)
    dev = torch.device("cuda", 0)
    out = []
    for use_fast in (False, True):
        if use_fast:
            renderer.upload_fast(scene, cam.center)
        else:
            renderer.upload(scene)
        img = torch.empty((1080, 1920, 3), dtype=torch.float64, device=dev)
        u8 = torch.empty((1080, 1920, 3), dtype=torch.uint8, device=dev)
        cnt = torch.zeros(12, dtype=torch.int64, device=dev)
        renderer.render_device(cam, img.data_ptr(), u8.data_ptr(), d_counters=cnt.data_ptr())
        torch.cuda.synchronize()
        out.append((img, u8, dict(zip(rt.COUNTER_FIELDS, cnt.tolist()))))
    (a, a8, ca), (b, b8, cb) = out
    assert torch.equal(a, b) and torch.equal(a8, b8)
    assert ca["rng_draws"] == cb["rng_draws"] and ca["segments"] == cb["segments"] and ca["surface_hits"] == cb["surface_hits"]
    assert cb["box_tests"] < 0.6 * ca["box_tests"] and cb["sphere_tests"] < ca["sphere_tests"]


# ---- the MIXED program: f32 culling boxes + exact f64 spheres (F_F32_BOX kernels) ---------------------------------
class _SphereRec(__import__("ctypes").Structure):
    import ctypes as _C
    _fields_ = [("center0", _C.c_double * 3), ("center_dir", _C.c_double * 3), ("radius", _C.c_double), ("material", _C.c_int32), ("_pad", _C.c_int32)]


def _spheres_of(scene):
    """The rtk_sphere table of a flattened scene (include/rtk.h), writable: tests poke motion into it."""
    import ctypes as C

    from tests.test_fast_order import DescHead

    head = DescHead.from_address(scene.desc_ptr)
    base = scene.desc_ptr + DescHead.list_children.offset + C.sizeof(C.c_void_p)   # `spheres` follows `list_children`
    ptr = C.c_void_p.from_address(base).value
    return (_SphereRec * head.n_spheres).from_address(ptr)


def test_mixed_program_kernel_is_used_and_bit_identical(rt, orc, renderer, scenes):
    """Sphere-only scenes in the fast order run the F_F32_BOX kernel (feature word 256): conservative f32 boxes must
    not change a single bit of the image; variant bit 20 falls back to the f64 fused boxes with the same result."""
    scene = scenes("book1_final")
    cam = scene.camera(256, 144, 16, 50)
    renderer.upload(scene)
    base, base8, _ = renderer.render_host(cam)
    renderer.upload_fast(scene, cam.center)
    assert "double, 256u" in renderer.kernel_name() and "double, 128u" in renderer.kernel_name(variant=1 << 20)
    mixed, mixed8, _ = renderer.render_host(cam)
    fused, fused8, _ = renderer.render_host(cam, variant=1 << 20)
    in_global, _, _ = renderer.render_host(cam, variant=1)
    assert np.array_equal(mixed, base) and np.array_equal(mixed8, base8)
    assert np.array_equal(fused, base) and np.array_equal(in_global, base)
    ref, ref8, _ = orc.render(scene.desc_ptr, cam, RENDER_SEED, 8)
    assert rmse(mixed, ref) < F64_RMSE_BOUND and np.array_equal(mixed8, ref8)
    # the counting build of the MIXED kernel (rtk_render_kernel<double, 256u, true, true>) against the oracle executing
    # the same re-grouped hierarchy: same image, closest-hit counters equal, culling counters a tight superset
    fast = scene.fast_order(cam.center)
    _, _, ocnt = orc.render(fast.desc_ptr, cam, RENDER_SEED, 8)
    counted, counted8, mcnt = renderer.render_host(cam, count=True)
    assert np.array_equal(counted, base) and np.array_equal(counted8, base8)
    _assert_culling_counters(mcnt, ocnt)
    in_global_counted, _, gcnt = renderer.render_host(cam, count=True, variant=1)
    assert np.array_equal(in_global_counted, base) and gcnt == mcnt


def test_mixed_program_moving_spheres_and_far_cameras(rt, orc, renderer):
    """Moving spheres (3-unit records) and rays the f32 test must not judge: a camera far outside the coordinate bound
    the box margin was sized for sends every primary ray through the exact f64 test on the f32 bounds."""
    scene = rt.Scene.build("three_spheres", SCENE_SEED)
    spheres = _spheres_of(scene)
    spheres[1].center_dir[0], spheres[1].center_dir[1] = 0.3, 0.2        # the centre sphere now moves (sphere.h:20-28)
    spheres[3].center_dir[2] = -0.25
    cam = scene.camera(96, 54, 8, 10)
    # The motion was poked in after the reference's bvh_node boxes were computed, so the reference order is not the
    # yardstick here: the optimiser recomputes every box from the primitives (sphere.h:24-26), and the oracle and the
    # exact-slab kernels run on that hierarchy.
    fast = scene.fast_order(cam.center)
    ref, ref8, _ = orc.render(fast.desc_ptr, cam, RENDER_SEED, 4)
    renderer.upload(fast)
    base, base8, _ = renderer.render_host(cam)
    assert rmse(base, ref) < F64_RMSE_BOUND and np.array_equal(base8, ref8)
    renderer.upload_fast(scene, cam.center)
    assert "double, 256u" in renderer.kernel_name()
    mixed, mixed8, _ = renderer.render_host(cam)
    assert np.array_equal(mixed, base) and np.array_equal(mixed8, base8)
    # a camera 700 units away along +z (the scene spans ~200): no eye passed, so the margin ignores it
    far = scene.camera(96, 54, 8, 10)
    for v in (far.center, far.pixel00_loc):
        v.z += 700.0
    ref_far, _, _ = orc.render(fast.desc_ptr, far, RENDER_SEED, 4)
    renderer.upload_fast(scene, None)
    got_far, _, _ = renderer.render_host(far)
    assert rmse(got_far, ref_far) < F64_RMSE_BOUND
    assert got_far.std() > 0.01   # the far camera still sees the scene


@pytest.mark.parametrize("seed,triangles", [(s, False) for s in range(6)] + [(s, True) for s in range(6)])
def test_random_soups_on_the_device(rt, orc, renderer, seed, triangles):
    """Random sphere/quad(/triangle) soups with instances (tests/test_fast_order_random.py): the kernels on the flat list
    agree with the oracle, and rtk_scene_upload_fast (COMPACT program: f32 culling boxes also under the instance transforms,
    ties by reference rank) renders the same bytes."""
    from tests.test_fast_order_random import look_at_camera, random_scene

    scene = random_scene(2000 + seed, triangles=triangles)
    cam = look_at_camera(rt)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, 7, 4)
    renderer.upload(scene)
    gpu, gpu8, cnt = renderer.render_host(cam, seed=7, count=True)
    assert rmse(gpu, ref) < F64_RMSE_BOUND and np.array_equal(gpu8, ref8) and cnt == ocnt
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"] and int(renderer.kernel_name().split(",")[1].strip(" u")) & 256
    fast, fast8, _ = renderer.render_host(cam, seed=7)
    assert np.array_equal(fast, gpu) and np.array_equal(fast8, gpu8)
    fast_global, _, fcnt = renderer.render_host(cam, seed=7, variant=1, count=True)
    assert np.array_equal(fast_global, gpu)
    for key in ("samples", "segments", "surface_hits", "rng_draws"):
        assert fcnt[key] == cnt[key], key


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_random_zoo_scenes_on_the_device(rt, orc, renderer, seed):
    """Random scenes with every feature at once (tests/test_fast_order_random.py::random_zoo_scene: seven materials, five textures,
    a textured medium, point lights, triangles and quads under instances): the full-feature kernels agree with the oracle in the
    reference order, work counters included, and the fast order renders the same doubles."""
    from tests.test_fast_order_random import look_at_camera, random_zoo_scene

    scene = random_zoo_scene(8000 + seed)
    cam = look_at_camera(rt)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, 7, 4)
    renderer.upload(scene)
    gpu, gpu8, cnt = renderer.render_host(cam, seed=7, count=True)
    assert rmse(gpu, ref) < F64_RMSE_BOUND and np.array_equal(gpu8, ref8) and cnt == ocnt
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"]
    fast, fast8, _ = renderer.render_host(cam, seed=7)
    assert np.array_equal(fast, gpu) and np.array_equal(fast8, gpu8)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_sphere_scenes_on_the_device(rt, orc, renderer, seed):
    """Random sphere-only scenes (tests/test_fast_order_random.py::random_sphere_scene: 5-700 spheres, radii over four orders of
    magnitude, a cluster far from the origin, moving spheres, a glass ball around everything): the headline kernel -- the lean
    MIXED program with f32 centre / half-extent boxes -- against the oracle, and equal to the reference order double for double."""
    from tests.test_fast_order_random import look_at_camera, random_sphere_scene

    scene = random_sphere_scene(12100 + seed)
    cam = look_at_camera(rt)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, 7, 4)
    renderer.upload(scene)
    gpu, gpu8, cnt = renderer.render_host(cam, seed=7, count=True)
    assert rmse(gpu, ref) < F64_RMSE_BOUND and np.array_equal(gpu8, ref8) and cnt == ocnt
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"] and info["proven"] and "256u" in renderer.kernel_name()
    fast, fast8, _ = renderer.render_host(cam, seed=7)
    assert np.array_equal(fast, gpu) and np.array_equal(fast8, gpu8)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_degenerate_scenes_on_the_device(rt, orc, renderer, seed):
    """Exact ties (the same primitive twice, coplanar overlaps), radius 0 and below, zero-area primitives, a sphere around the
    camera (tests/test_fast_order_random.py::random_degenerate_scene): the device resolves them as the reference does, in both
    orders."""
    from tests.test_fast_order_random import look_at_camera, random_degenerate_scene

    scene = random_degenerate_scene(11100 + seed)
    cam = look_at_camera(rt)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, 7, 4)
    renderer.upload(scene)
    gpu, gpu8, cnt = renderer.render_host(cam, seed=7, count=True)
    assert rmse(gpu, ref) < F64_RMSE_BOUND and np.array_equal(gpu8, ref8) and cnt == ocnt
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"]
    fast, fast8, _ = renderer.render_host(cam, seed=7)
    assert np.array_equal(fast, gpu) and np.array_equal(fast8, gpu8)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
def test_random_big_scenes_on_the_device(rt, orc, renderer, seed):
    """Random scenes of a few thousand primitives (tests/test_fast_order_random.py::random_big_scene): the traversal program is
    larger than LDS, so these run the kernels that keep only a part of it there -- against the oracle in the reference order,
    and bit-identical in the fast order."""
    from tests.test_fast_order_random import look_at_camera, random_big_scene

    scene = random_big_scene(9100 + seed)
    cam = look_at_camera(rt)
    ref, ref8, ocnt = orc.render(scene.desc_ptr, cam, 7, 4)
    renderer.upload(scene)
    assert renderer.kernel_name().rstrip(">").endswith("false")        # not the all-in-LDS instantiation
    gpu, gpu8, cnt = renderer.render_host(cam, seed=7, count=True)
    assert rmse(gpu, ref) < F64_RMSE_BOUND and np.array_equal(gpu8, ref8) and cnt == ocnt
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"]
    fast, fast8, _ = renderer.render_host(cam, seed=7)
    assert np.array_equal(fast, gpu) and np.array_equal(fast8, gpu8)


@pytest.mark.gpu
def test_rendering_before_importing_torch_leaves_torch_its_devices():
    """One HIP runtime per process (raytracingoneweekendapplication_amd._one_hip_runtime): a script that renders first and only
    then imports torch still gets torch.cuda, and a torch tensor is a valid render target."""
    code = ("import raytracingoneweekendapplication_amd as rt\n"
            "scene = rt.Scene.build('three_spheres'); cam = scene.camera(32, 18, 2, 4)\n"
            "r = rt.Renderer(0); r.upload(scene)\n"
            "a, _, _ = r.render_host(cam)\n"
            "import torch\n"
            "assert torch.cuda.is_available() and torch.cuda.device_count() >= 1\n"
            "img = torch.empty((18, 32, 3), dtype=torch.float64, device='cuda:0')\n"
            "r.render_device(cam, img.data_ptr(), 0); torch.cuda.synchronize()\n"
            "import numpy as np\n"
            "assert np.array_equal(img.cpu().numpy(), a)\n")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]


def test_cpp_camera_render_through_the_drop_in_api(rt, tmp_path):
    """The C++ side of the boundary end to end (host/rtk_camera.h): a reference-style program builds its scene with the
    drop-in classes and calls camera::render_to.  auto_order must pick the fast order exactly when it is bit-identical
    and then give the very same doubles as reference_order -- with a constant_medium in the scene as well; only with
    camera::free_media_order it must stay on the reference order (identical again), while the forced fast order is
    statistically the same image."""
    import json
    import subprocess

    from tests.conftest import ROOT

    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "camera_render_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "camera_render_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    verdict = json.loads(out.strip().splitlines()[-1])
    clear, fog = verdict["fog0"], verdict["fog1"]
    assert clear["rc"] == [0, 0, 0] and fog["rc"] == [0, 0, 0]
    for v in (clear, fog):   # with a medium too: it keeps its place in the reference's order (rtk_optimize_opts.free_media_order = 0)
        assert v["exact"] and v["auto_used_fast"] and v["auto_identical"] and v["fast_identical"]
    # camera::free_media_order: nothing changes without a medium; with one the pass no longer claims exactness, auto_order
    # stays on the reference order, and the forced fast order is another image of the same estimator
    assert clear["free_exact"] and clear["free_auto_used_fast"] and clear["free_auto_identical"] and clear["free_fast_identical"]
    assert not fog["free_exact"] and not fog["free_auto_used_fast"] and fog["free_auto_identical"] and not fog["free_fast_identical"]
    assert abs(fog["mean_free"] - fog["mean_ref"]) < 0.03 * fog["mean_ref"]
    assert clear["mean_ref"] > 0.05
    # camera::devices = {0, 0} / {0, 0, 0}: render() splits the image itself (rtk_render_multi) -- same doubles, same bytes;
    # camera::progress is fed from the work-item counters and ends at the total (Camera.txt:102-106 prints a percentage)
    for verdict in (clear, fog):
        assert verdict["two_devices_identical"] and verdict["three_devices_identical"] and verdict["bytes_identical"]
        assert verdict["progress_calls"] >= 1 and verdict["progress_monotone"] and verdict["progress_reached_total"]


@pytest.mark.parametrize("devices,gather,real", [([0, 0], "auto", "f64"), ([0, 0, 0, 0, 0], "peer", "f64"), ([0, 0, 0], "auto", "f32"), ([0], "rccl", "f64"), ([0], "auto", "f64")])
def test_render_multi_behind_the_c_abi_reproduces_the_one_gpu_bytes(rt, renderer, scenes, devices, gather, real):
    """rtk_init_multi / rtk_render_multi (one host thread, one stream per device slot, replicated upload -- the SAH pass
    once --, compact tile buffers, ONE gather to the first device, rtk_tiles_unpermute there).  On this one-GPU box the
    device is listed several times (peer-copy gather; RCCL refuses duplicate devices) and, for the RCCL transport, once
    with the gather forced through a 1-rank ncclGather.  The image must not depend on any of it."""
    scene = scenes("book1_final")
    cam = scene.camera(100, 60, 10, 50)      # 104 tiles: ragged against 2, 3 and 5 ranks; 10 spp: two sample chunks
    mode = rt.RTK_REAL_F64 if real == "f64" else rt.RTK_REAL_F32
    for fast in (False, True):
        renderer.upload_fast(scene, cam.center) if fast else renderer.upload(scene)
        whole, whole8, _ = renderer.render_host(cam, real_mode=mode)
        multi = rt.MultiRenderer(devices, {"auto": rt.GATHER_AUTO, "peer": rt.GATHER_PEER, "rccl": rt.GATHER_RCCL}[gather])
        assert multi.uses_rccl == (gather == "rccl")
        info = multi.upload_fast(scene, cam.center) if fast else multi.upload(scene)
        assert multi.kernel_name(mode) == renderer.kernel_name(mode) and (not fast or info["exact"])
        seen = []
        multi.set_progress(lambda done, total: seen.append((done, total)), interval_ms=1)
        image, image8 = multi.render_host(cam, real_mode=mode)
        first, seen = seen, []
        multi.set_progress(lambda done, total: seen.append((done, total)), interval_ms=1)
        again, _ = multi.render_host(cam, real_mode=mode)       # buffers and the learned tile order are reused
        assert np.array_equal(image, whole) and np.array_equal(image8, whole8) and np.array_equal(again, whole)
        for reports in (first, seen):     # per render: monotone, within [0, total], ending at the total (work items = tiles x sample chunks)
            assert reports and reports[-1][0] == reports[-1][1] == -(-104 // len(devices)) * len(devices) * 2   # tiles per rank x ranks x 2 chunks
            assert all(0 <= a[0] <= b[0] <= b[1] for a, b in zip(reports, reports[1:]))
        multi.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]], ids=["2", "4"])
def test_render_multi_enqueue_keeps_two_frames_in_flight_and_the_same_bytes(rt, renderer, scenes, devices):
    """rtk_render_multi_enqueue / rtk_multi_wait: a sequence of frames alternating between two cameras and two pairs of output
    buffers, enqueued back to back and waited for once -- frame k's gather and un-permute overlap frame k + 1's renders, frame
    k + 2 re-uses frame k's tile buffers.  Every frame must be the one-device image of its camera, in both arithmetic types
    and both orders; the blocking form (enqueue + wait) afterwards gives the same bytes again."""
    import torch

    scene = scenes("book1_final")
    cams = [scene.camera(100, 60, 10, 50), scene.camera(100, 60, 3, 50)]      # 104 tiles, ragged against 2 and 4 ranks; two sample chunks / one
    dev = torch.device("cuda", 0)
    for mode, dtype in ((rt.RTK_REAL_F64, torch.float64), (rt.RTK_REAL_F32, torch.float32)):
        for fast in (False, True):
            renderer.upload_fast(scene, cams[0].center) if fast else renderer.upload(scene)
            want = []
            for cam in cams:
                whole, whole8, _ = renderer.render_host(cam, real_mode=mode)
                want.append((whole, whole8))
            multi = rt.MultiRenderer(devices)
            multi.upload_fast(scene, cams[0].center) if fast else multi.upload(scene)
            frames = 7
            images = [torch.zeros((60, 100, 3), dtype=dtype, device=dev) for _ in range(frames)]
            bytes8 = [torch.zeros((60, 100, 3), dtype=torch.uint8, device=dev) for _ in range(frames)]
            for k in range(frames):
                multi.enqueue_device(cams[k % 2], images[k].data_ptr(), bytes8[k].data_ptr(), real_mode=mode)
            multi.wait()
            torch.cuda.synchronize()
            for k in range(frames):
                assert np.array_equal(images[k].cpu().numpy().astype(np.float64), want[k % 2][0]), (k, mode, fast)
                assert np.array_equal(bytes8[k].cpu().numpy(), want[k % 2][1]), (k, mode, fast)
            images[0].zero_()
            multi.render_device(cams[1], images[0].data_ptr(), bytes8[0].data_ptr(), real_mode=mode)
            assert np.array_equal(images[0].cpu().numpy().astype(np.float64), want[1][0])
            multi.close()


def test_render_multi_error_behaviour(rt):
    with pytest.raises(rt.RtkError) as e:
        rt.MultiRenderer([0, 99])
    assert e.value.code == -1                 # device out of range
    with pytest.raises(rt.RtkError) as e:
        rt.MultiRenderer([0, 0], rt.GATHER_RCCL)
    assert e.value.code == -4 and "more than once" in str(e.value)     # RCCL cannot run two ranks on one device
    multi = rt.MultiRenderer([0, 0])
    cam = rt.Scene.build("three_spheres").camera(16, 16, 1, 2)
    with pytest.raises(rt.RtkError) as e:
        multi.render_host(cam)
    assert e.value.code == -5                 # RTK_ERR_NO_SCENE


def test_boxes_in_lds_kernel_for_programs_larger_than_lds(rt, orc, renderer, scenes):
    """F_LDS_BOXES: a program that cannot be staged in LDS whole keeps its box slots, kind nibbles and rank table there;
    the image is the one the all-in-memory kernel and the counting kernel compute (variant bit 21 switches it off)."""
    scene = scenes("mesh")                       # 1280 triangles: 295 KB of f64 program, 99 KB of boxes
    cam = scene.camera(64, 36, 4, 10)
    for fast in (False, True):
        renderer.upload_fast(scene, cam.center) if fast else renderer.upload(scene)
        # fast order: the COMPACT program (151 KB) fits LDS whole; its slot program (variant bit 20) does not
        slot = (1 << 20) if fast else 0
        if fast:
            assert renderer.kernel_name().endswith("false, true>") and int(renderer.kernel_name().split(",")[1].strip(" u")) & 256
        with_boxes, plain = renderer.kernel_name(variant=slot), renderer.kernel_name(variant=slot | (1 << 21))
        assert "false, false" in with_boxes and int(with_boxes.split(",")[1].strip(" u")) == int(plain.split(",")[1].strip(" u")) | 1024
        a, a8, _ = renderer.render_host(cam, variant=slot)
        b, b8, _ = renderer.render_host(cam, variant=slot | (1 << 21))
        c, c8, _ = renderer.render_host(cam, count=True)
        d, d8, _ = renderer.render_host(cam)
        assert np.array_equal(a, b) and np.array_equal(a8, b8) and np.array_equal(a, c) and np.array_equal(a, d)
    renderer.upload(scene)
    ref, ref8, _ = orc.render(scene.desc_ptr, cam, RENDER_SEED, 8)
    a, a8, _ = renderer.render_host(cam)
    assert rmse(a, ref) < F64_RMSE_BOUND and np.array_equal(a8, ref8)
    # the book-2 scene (887 KB of f64 program, 2 570 boxes in 56-byte records): same arithmetic with and without the LDS copies
    scene = scenes("book2_final")
    cam = scene.camera(64, 36, 4, 10)
    renderer.upload(scene)
    for real in (rt.RTK_REAL_F64, rt.RTK_REAL_F32):
        assert "1151u" in renderer.kernel_name(real) and "127u" in renderer.kernel_name(real, 1 << 21)
        a, a8, _ = renderer.render_host(cam, real_mode=real)
        b, b8, _ = renderer.render_host(cam, real_mode=real, variant=1 << 21)
        assert np.array_equal(a, b) and np.array_equal(a8, b8)
