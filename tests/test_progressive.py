"""Progressive, resumable rendering (rtk_progressive_*): a frame rendered in steps of whole sample chunks into a session's own
running sums is the one-shot frame bit for bit; previews equal short one-shot renders; checkpoints resume to the same image and
are refused when anything the image depends on differs; the batch-means noise estimate matches a numpy restatement.

CPU tests: the checkpoint format (parsed from a blob built field by field here), the exported entry points and the tile-to-image
helper of the numpy checks.
GPU tests (-m gpu): everything that renders."""
import ctypes as C
import hashlib
import os
import re
import struct

import numpy as np
import pytest

from tests.conftest import EARTH, ROOT

ENTRY_POINTS = ("rtk_progressive_create", "rtk_progressive_step", "rtk_progressive_step_host", "rtk_progressive_samples_done",
                "rtk_progressive_chunk_size", "rtk_progressive_noise", "rtk_progressive_checkpoint_bytes", "rtk_progressive_save",
                "rtk_progressive_resume", "rtk_checkpoint_read_info", "rtk_progressive_destroy")


def _fnv64(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _tiles(w, h, n_ranks):
    return (((w + 7) // 8) * ((h + 7) // 8) + n_ranks - 1) // n_ranks


def _blob(rt, *, version=1, w=20, h=12, rank=0, n_ranks=1, real_mode=0, target=48, chunk=8, done=16, seed=7, digest=0x1122334455667788,
          payload_tiles=None, magic=b"RTKPROG\0", fix_checksum=True):
    """A checkpoint assembled field by field as include/rtk.h documents it."""
    cam = rt.Camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, target, 5
    cam.pixel_samples_scale = 1.0 / target
    head = magic + struct.pack("<9iIQ", version, w, h, rank, n_ranks, real_mode, target, chunk, done, seed, digest) + bytes(cam)
    assert len(head) == 256
    tiles = _tiles(w, h, n_ranks) if payload_tiles is None else payload_tiles
    elem = 8 if real_mode == 0 else 4
    rng = np.random.default_rng(3)
    body = rng.random(tiles * 192 * elem // 8 + 1).tobytes()[: tiles * 192 * elem] + rng.random(tiles * 64).tobytes() + rng.random(tiles * 64).tobytes()
    data = head + body
    return data + struct.pack("<Q", _fnv64(data) if fix_checksum else 0)


# ----------------------------------------------------------------------------------------------------------------- CPU --
def test_header_declares_and_library_exports_the_progressive_api(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, body), name
    for typ in ("rtk_progressive", "rtk_noise_stats", "rtk_checkpoint_info"):
        assert re.search(r"typedef struct %s\b" % typ, body), typ
    assert "#define RTK_ABI_VERSION 2" in body           # added functions only
    lib = C.CDLL(rt.HIP_LIB_PATH)                         # loads without a GPU
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing


def test_checkpoint_info_parses_a_blob_built_field_by_field(rt):
    info = rt.checkpoint_info(_blob(rt))
    assert info == {"version": 1, "width": 20, "height": 12, "rank": 0, "n_ranks": 1, "real_mode": 0, "target_spp": 48, "chunk_size": 8,
                    "samples_done": 16, "seed": 7, "scene_digest": 0x1122334455667788}
    # f32 sums are 4-byte reals; a rank of several owns fewer tiles; chunk size 16 for a 1000-spp target
    info = rt.checkpoint_info(_blob(rt, real_mode=1, w=100, h=30, rank=1, n_ranks=3, target=1000, chunk=16, done=1000, seed=1))
    assert (info["real_mode"], info["rank"], info["n_ranks"], info["chunk_size"], info["samples_done"]) == (1, 1, 3, 16, 1000)


@pytest.mark.parametrize("what", ["magic", "version", "truncated", "size_vs_ranks", "size_vs_dims", "checksum", "chunk", "done"])
def test_checkpoint_info_rejects_malformed_blobs(rt, what):
    good = _blob(rt)
    bad = {
        "magic": lambda: _blob(rt, magic=b"RTKPROGX"),
        "version": lambda: _blob(rt, version=2),
        "truncated": lambda: good[:-100],
        "size_vs_ranks": lambda: _blob(rt, n_ranks=2, payload_tiles=_tiles(20, 12, 1)),   # header says 2 ranks, payload is one rank's
        "size_vs_dims": lambda: _blob(rt, w=40, payload_tiles=_tiles(20, 12, 1)),
        "checksum": lambda: good[:300] + bytes([good[300] ^ 1]) + good[301:],
        "chunk": lambda: _blob(rt, chunk=16),                                              # 48 spp: chunks of 8
        "done": lambda: _blob(rt, done=56),                                                # beyond the target
    }[what]()
    with pytest.raises(rt.RtkError) as e:
        rt.checkpoint_info(bad)
    assert e.value.code == -1
    with pytest.raises(rt.RtkError):
        rt.checkpoint_info(good[:8])


# ----------------------------------------------------------------------------------------------------------------- GPU --
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _full_size(rt, renderer, tmp_path, name):
    """The scene, camera and upload of bench.py / test_configs_3_4_5_at_their_stated_sizes (fast order)."""
    scene = rt.Scene.build(name, rt.SCENE_SEED, rt.write_synthetic_earth(str(tmp_path / "earth_synth.ppm")))
    cam = scene.camera()
    info = renderer.upload_fast(scene, cam.center)
    assert info["exact"]
    return scene, cam


def _run_steps(renderer, cam, steps, **kw):
    p = renderer.progressive(cam, **kw)
    for n in steps:
        linear, _, _ = p.step(n)
    assert p.samples_done == cam.samples_per_pixel
    p.close()
    return linear


@pytest.mark.gpu
def test_c2_full_size_in_steps_has_the_pinned_digest(rt, renderer, tmp_path):
    import bench

    scene, cam = _full_size(rt, renderer, tmp_path, "book1_final")
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (1920, 1080, 100)
    assert _sha(_run_steps(renderer, cam, [8] * 12 + [4])) == bench.PINNED_SHA256["c2"] == "02cec6778ff20839"
    assert _sha(_run_steps(renderer, cam, [24, 40, 36])) == bench.PINNED_SHA256["c2"]


@pytest.mark.gpu
def test_c3_larger_chunks_and_refused_steps(rt, renderer, tmp_path):
    import bench

    scene, cam = _full_size(rt, renderer, tmp_path, "cornell_box")
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (800, 800, 1000)
    p = renderer.progressive(cam)
    assert p.chunk_size == 16
    for n in (100, 0, -16):                               # not a multiple of 16 / not positive
        with pytest.raises(rt.RtkError) as e:
            p.step(n)
        assert e.value.code == -1 and p.samples_done == 0
    for _ in range(6):
        linear, _, _ = p.step(160)
    with pytest.raises(rt.RtkError):
        p.step(100)                                       # 960 + 100 passes the target
    with pytest.raises(rt.RtkError):
        p.step(48)                                        # a multiple of 16, still past the target
    linear, _, _ = p.step(40)                             # ends exactly at the target: a partial last chunk (8 samples)
    assert p.samples_done == 1000
    with pytest.raises(rt.RtkError):
        p.step(16)                                        # finished
    assert _sha(linear) == bench.PINNED_SHA256["c3"] == "626eb89c5adf83ce"


@pytest.mark.gpu
def test_c5_multi_launch_steps(rt, renderer, tmp_path):
    import bench

    scene, cam = _full_size(rt, renderer, tmp_path, "book2_final")
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (1920, 1080, 1000)
    assert rt.hip_lib().rtk_frame_launches(C.byref(cam), C.byref(rt.RenderOpts(rt.RENDER_SEED, 0, 0, 1, 0, 0, None))) == 3  # 21 chunks per launch
    # chunks of 16: a step of 400 samples is 25 chunks, two launches
    assert _sha(_run_steps(renderer, cam, [400, 400, 200])) == bench.PINNED_SHA256["c5"] == "5f3398426c23599e"


def _small_scenes(rt):
    return [("book1_final", 96, 56, 48, 8), ("cornell_box", 64, 64, 40, 6), ("material_zoo", 96, 54, 48, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1])
def test_previews_equal_short_one_shot_renders(rt, renderer, real_mode):
    for name, w, h, target, depth in _small_scenes(rt):
        scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
        renderer.upload(scene)
        cam = scene.camera(w, h, target, depth)
        p = renderer.progressive(cam, real_mode=real_mode)
        while p.samples_done < target:
            linear, rgb8, noise = p.step(8)
            ref, ref8, _ = renderer.render_host(scene.camera(w, h, p.samples_done, depth), real_mode=real_mode)
            assert np.array_equal(linear, ref), (name, p.samples_done)
            assert np.array_equal(rgb8, ref8), (name, p.samples_done)
            assert noise.shape == (h, w) and np.all(noise >= 0)
        p.close()
        # work counters per step (the counting kernels): their sum is the one-shot frame's
        p = renderer.progressive(cam, real_mode=real_mode)
        total = None
        for n in (8, 16, target - 24):
            _, _, _, cnt = p.step(n, count=True)
            total = cnt if total is None else {k: total[k] + cnt[k] for k in cnt}
        _, _, one = renderer.render_host(cam, real_mode=real_mode, count=True)
        assert total == one, name
        p.close()


@pytest.mark.gpu
def test_resume_in_a_fresh_context(rt, tmp_path):
    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    cam = scene.camera(120, 64, 96, 8)
    r = rt.Renderer(0)
    r.upload_fast(scene, cam.center)
    one, one8, _ = r.render_host(cam)
    p = r.progressive(cam)
    for _ in range(3):
        p.step(16)
    blob = p.save()
    info = rt.checkpoint_info(blob)
    assert (info["samples_done"], info["target_spp"], info["chunk_size"], info["width"]) == (48, 96, 8, 120)
    p.close()
    r.close()

    r2 = rt.Renderer(0)
    r2.upload_fast(scene, cam.center)
    q = r2.resume(cam, blob)
    assert q.samples_done == 48
    linear, rgb8, _ = q.step(48)
    assert np.array_equal(linear, one) and np.array_equal(rgb8, one8)
    q.close()

    refusals = {
        "seed": lambda: r2.resume(cam, blob, seed=rt.RENDER_SEED + 1),
        "camera": lambda: r2.resume(scene.camera(120, 64, 96, 9), blob),
        "target": lambda: r2.resume(scene.camera(120, 64, 104, 8), blob),
        "real_mode": lambda: r2.resume(cam, blob, real_mode=rt.RTK_REAL_F32),
        "ranks": lambda: r2.resume(cam, blob, rank=0, n_ranks=2),
    }
    for what, call in refusals.items():
        with pytest.raises(rt.RtkError) as e:
            call()
        assert e.value.code == -1 and r2._lib.rtk_last_error(), what
    r2.upload(scene)                                      # the same scene in the reference order: another program
    with pytest.raises(rt.RtkError, match="another scene"):
        r2.resume(cam, blob)
    r2.upload_fast(rt.Scene.build("cornell_box", rt.SCENE_SEED), cam.center)
    with pytest.raises(rt.RtkError, match="another scene"):
        r2.resume(cam, blob)
    r2.upload_fast(scene, cam.center)                     # back to the checkpoint's scene: accepted again
    r2.resume(cam, blob).close()
    r2.close()


@pytest.mark.gpu
def test_scene_change_fails_later_steps_and_one_shots_do_not_disturb(rt, renderer):
    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    cam = scene.camera(64, 40, 32, 6)
    renderer.upload(scene)
    one, _, _ = renderer.render_host(cam)
    p = renderer.progressive(cam)
    p.step(8)
    renderer.render_host(scene.camera(96, 56, 24, 6))   # a one-shot on the same context between steps
    p.step(16)
    renderer.upload(rt.Scene.build("three_spheres", rt.SCENE_SEED))
    with pytest.raises(rt.RtkError, match="scene changed"):
        p.step(8)
    renderer.upload(scene)
    linear, _, _ = p.step(8)
    assert np.array_equal(linear, one)
    p.close()


@pytest.mark.gpu
def test_two_ranks_on_one_device_equal_one_rank(rt, renderer):
    from raytracingoneweekendapplication_amd.tiling import image_from_gathered

    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    w, h = 84, 50                                         # partial tiles at the right and bottom edges
    cam = scene.camera(w, h, 40, 6)
    renderer.upload(scene)
    whole = renderer.progressive(cam)
    ranks = [renderer.progressive(cam, rank=k, n_ranks=2) for k in range(2)]
    for n in (8, 16, 16):
        ref, _, ref_noise = whole.step(n)
        parts = [r.step(n) for r in ranks]
        gathered = np.stack([lin for lin, _, _ in parts])
        assert np.array_equal(image_from_gathered(gathered, w, h, 2), ref)
        noise = image_from_gathered(np.stack([nz[:, None, :].repeat(3, 1) for _, _, nz in parts]), w, h, 2)[..., 0]
        assert np.array_equal(noise, ref_noise)
    for r in ranks + [whole]:
        r.close()


def _sums_from_blob(blob, tiles, elem=8):
    """(running sums [tiles, 3, 64] as float64, S1, S2) of a checkpoint: `elem`-byte running sums (4 in f32 sessions), then the
    f64 S1 and S2 planes."""
    body = np.frombuffer(blob, np.uint8, offset=256)
    n_acc = tiles * 192 * elem
    acc = np.frombuffer(body[:n_acc].tobytes(), np.float64 if elem == 8 else np.float32).astype(np.float64).reshape(tiles, 3, 64)
    s1 = np.frombuffer(body[n_acc: n_acc + tiles * 64 * 8].tobytes(), np.float64).reshape(tiles, 64)
    s2 = np.frombuffer(body[n_acc + tiles * 64 * 8: n_acc + tiles * 128 * 8].tobytes(), np.float64).reshape(tiles, 64)
    return acc, s1, s2


def _tile_image(a, w, h):
    """[tiles, 64] of one rank of one -> (h, w): tile t = (row ty, column tx), lane = 8 * pixel row + pixel column."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    a = np.asarray(a)
    return np.ascontiguousarray(a[: tx * ty].reshape(ty, tx, 8, 8).transpose(0, 2, 1, 3).reshape(ty * 8, tx * 8)[:h, :w])


def _tile_image_loop(a, w, h):
    """_tile_image written out pixel by pixel (the CPU test's yardstick)."""
    tx = (w + 7) // 8
    out = np.zeros((h, w), a.dtype)
    for t in range(a.shape[0]):
        for lane in range(64):
            i, j = (t % tx) * 8 + (lane & 7), (t // tx) * 8 + (lane >> 3)
            if i < w and j < h:
                out[j, i] = a[t, lane]
    return out


def test_tile_image_equals_the_pixel_loop():
    rng = np.random.default_rng(2)
    for w, h in ((128, 128), (16, 16), (96, 56), (64, 64), (96, 54), (64, 40), (84, 50), (120, 64), (1, 1), (13, 7), (1, 37), (37, 1), (65, 9)):
        a = rng.random((_tiles(w, h, 1), 64))
        got = _tile_image(a, w, h)
        assert got.shape == (h, w) and got.dtype == a.dtype
        assert np.array_equal(got, _tile_image_loop(a, w, h)), (w, h)
        f = a.astype(np.float32)
        assert np.array_equal(_tile_image(f, w, h), _tile_image_loop(f, w, h)) and _tile_image(f, w, h).dtype == np.float32


@pytest.mark.gpu
def test_noise_estimate_matches_numpy(rt, renderer):
    # the Cornell box: a light (real noise) and a black background -- the camera's view is a little wider than the box, so the
    # outermost columns see nothing, and a pixel whose every sample is background has se == 0 exactly
    scene = rt.Scene.build("cornell_box", rt.SCENE_SEED)
    w, h, target = 128, 128, 64
    cam = scene.camera(w, h, target, 6)
    renderer.upload(scene)
    tiles = _tiles(w, h, 1)

    def run():
        p = renderer.progressive(cam)
        assert p.chunk_size == 8
        stats, chunks, prev = [], [], None
        for k in range(target // 8):
            linear, _, noise = p.step(8)
            st = p.noise()
            assert st["samples_done"] == 8 * (k + 1) and st["full_chunks"] == k + 1 and st["valid"] == (1 if k >= 1 else 0)
            stats.append(st)
            acc, s1, s2 = _sums_from_blob(p.save(), tiles)
            chunks.append(acc.copy() if prev is None else acc - prev)
            prev = acc.copy()
        p.close()
        return linear, noise, stats, chunks, s1, s2

    linear, noise, stats, chunks, s1, s2 = run()
    # numpy restatement: y_k per chunk, S1 / S2, se, frame statistics
    y = np.stack([(c[:, 0, :] + c[:, 1, :] + c[:, 2, :]) / (3.0 * 8) for c in chunks])
    K = y.shape[0]
    np.testing.assert_allclose(s1, y.sum(0), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(s2, (y * y).sum(0), rtol=1e-9, atol=1e-12)

    def se_of(a1, a2):
        m = a1 / K
        return np.sqrt(np.maximum(0.0, (a2 - K * m * m) / (K - 1)) / K), m

    se_dev, m = se_of(s1, s2)                             # from the device's own sums: the per-pixel plane and the statistics
    se_img = _tile_image(se_dev, w, h)
    np.testing.assert_allclose(noise, se_img.astype(np.float32), rtol=1e-6, atol=0)
    inside = _tile_image(np.ones_like(se_dev), w, h) > 0
    rel_img = _tile_image(se_dev / np.maximum(m, 1e-3), w, h)
    st = stats[-1]
    assert st["valid"] == 1 and st["full_chunks"] == K and st["samples_done"] == target
    np.testing.assert_allclose(st["mean_se"], se_img[inside].mean(), rtol=1e-9)
    np.testing.assert_allclose(st["max_se"], se_img[inside].max(), rtol=1e-12)
    np.testing.assert_allclose(st["mean_rel_se"], rel_img[inside].mean(), rtol=1e-9)
    se_np, _ = se_of(y.sum(0), (y * y).sum(0))            # from the chunk sums restated in numpy
    np.testing.assert_allclose(se_img, _tile_image(se_np, w, h), rtol=1e-6, atol=1e-9)
    black = np.all(linear == 0.0, axis=2)
    assert black.sum() > 0 and np.all(noise[black] == 0.0)
    assert stats[0]["valid"] == 0 and stats[0]["mean_se"] == 0.0
    # a second identical run: bit-identical statistics
    _, noise2, stats2, _, _, _ = run()
    assert stats2 == stats and np.array_equal(noise2, noise)


def _check_noise_against_the_sums(p, noise, w, h):
    """The step's per-pixel se plane and p.noise() against numpy from the checkpoint's own S1 / S2 (one rank, K full chunks)."""
    k = p.samples_done // p.chunk_size
    _, s1, s2 = _sums_from_blob(p.save(), _tiles(w, h, 1), 8 if p.real_mode == 0 else 4)
    m = s1 / k
    se = np.sqrt(np.maximum(0.0, (s2 - k * m * m) / (k - 1)) / k)
    se_img = _tile_image(se, w, h)
    rel_img = _tile_image(se / np.maximum(m, 1e-3), w, h)
    np.testing.assert_allclose(noise, se_img.astype(np.float32), rtol=1e-6, atol=0)
    st = p.noise()
    assert st["valid"] == 1 and st["full_chunks"] == k and st["samples_done"] == p.samples_done
    np.testing.assert_allclose(st["mean_se"], se_img.mean(), rtol=1e-9)
    np.testing.assert_allclose(st["max_se"], se_img.max(), rtol=1e-12)
    np.testing.assert_allclose(st["mean_rel_se"], rel_img.mean(), rtol=1e-9)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("book1_final", 48, 16, 0), ("book1_final", 48, 16, 1), ("cornell_box", 1000, 160, 0)],
                         ids=["c2-f64", "c2-f32", "c3-f64"])
def test_noise_estimate_at_full_size_matches_numpy(rt, renderer, tmp_path, case):
    """Full-size frames: 1920x1080 is 32 400 tiles, 8 100 block partials of the noise statistics (8-sample chunks); 800x800 is
    2 500 partials of 16-sample chunks.  rtk_noise_final_kernel reduces them in strided slices of 256."""
    name, target, step, real_mode = case
    scene, cam = _full_size(rt, renderer, tmp_path, name)
    cam = scene.camera(cam.image_width, cam.image_height, target, cam.max_depth)
    w, h = cam.image_width, cam.image_height
    partials = (_tiles(w, h, 1) * 64 + 255) // 256
    assert partials > 2 * 256, partials
    p = renderer.progressive(cam, real_mode=real_mode)
    assert p.chunk_size == (8 if target <= 512 else 16)
    means = []
    for _ in range(2 if name == "cornell_box" else 3):
        _, _, noise = p.step(step)
        means.append(_check_noise_against_the_sums(p, noise, w, h)["mean_se"])
    assert means == sorted(means, reverse=True) and means[-1] > 0    # more chunks, less noise
    p.close()


@pytest.mark.gpu
def test_cpp_camera_progressive_render(rt, tmp_path):
    """camera::render() of the drop-in C++ API (host/rtk_camera.h): progressive_step = 8 writes the one-shot PNG's bytes; a
    checkpoint written at 48 spp through the Python API is resumed (target - 48 samples rendered, same bytes); noise_target
    stops at the first chunk boundary where the frame's mean relative standard error is low enough."""
    import json
    import subprocess

    w, h, target, depth, noise_target = 128, 64, 96, 8, 1.0
    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    cam = scene.camera(w, h, target, depth)
    r = rt.Renderer(0)
    r.upload_fast(scene, cam.center)                     # camera::order = auto_order takes the (proven) fast order here
    p = r.progressive(cam)
    p.step(24)
    p.step(24)
    ckpt = tmp_path / "frame.ckpt"
    ckpt.write_bytes(p.save())
    p.close()
    r.close()

    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "progressive_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "progressive_camera_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.check_output([exe, str(tmp_path), str(ckpt), str(w), str(h), str(target), str(depth), str(noise_target)], timeout=300).decode()
    v = json.loads(out.strip().splitlines()[-1])
    one = (tmp_path / "one.png").read_bytes()
    assert (tmp_path / "prog.png").read_bytes() == one
    assert (v["prog_rendered"], v["prog_done"], v["prog_valid"]) == (target, target, 1)
    assert (tmp_path / "resumed.png").read_bytes() == one
    assert (v["resumed_rendered"], v["resumed_done"]) == (target - 48, target)
    assert rt.checkpoint_info(ckpt.read_bytes())["samples_done"] == target   # saved after every step
    assert v["noise_valid"] == 1 and v["noise_mean_rel_se"] <= noise_target
    assert v["noise_done"] < target and v["noise_done"] % 8 == 0 and v["noise_rendered"] == v["noise_done"]
    assert v["noise_full_chunks"] == v["noise_done"] // 8
