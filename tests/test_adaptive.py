"""Tile-adaptive sampling of progressive sessions (rtk_progressive_set_adaptive): a tile retires once the largest relative standard
error of its pixels is low enough; every pixel of a tile then equals a one-shot render at that tile's own sample count, bit for bit.

CPU tests: the API's declarations and exports, version-2 checkpoints (built field by field here), argument checks and the
rel_target picker of the large cases.
GPU tests (-m gpu): everything that renders."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from tests.conftest import EARTH, ROOT
from tests.test_progressive import _tile_image

ENTRY_POINTS = ("rtk_progressive_set_adaptive", "rtk_adaptive_status", "rtk_adaptive_tile_samples", "rtk_checkpoint_read_adaptive")


def _fnv64(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _tiles(w, h, n_ranks):
    return (((w + 7) // 8) * ((h + 7) // 8) + n_ranks - 1) // n_ranks


def _blob(rt, *, version=2, w=20, h=12, rank=0, n_ranks=1, target=48, chunk=8, done=32, seed=7, digest=0x1122334455667788,
          rel_target=0.05, min_samples=16, pad=0, tile_spp=None, adaptive_block=True, fix_checksum=True):
    """A checkpoint assembled field by field as include/rtk.h documents it (f64 sums); version 2 appends the adaptive block."""
    cam = rt.Camera()
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, target, 5
    cam.pixel_samples_scale = 1.0 / target
    head = b"RTKPROG\0" + struct.pack("<9iIQ", version, w, h, rank, n_ranks, 0, target, chunk, done, seed, digest) + bytes(cam)
    assert len(head) == 256
    tiles = _tiles(w, h, n_ranks)
    rng = np.random.default_rng(5)
    data = head + rng.random(tiles * 192).tobytes() + rng.random(tiles * 64).tobytes() + rng.random(tiles * 64).tobytes()
    if adaptive_block:
        if tile_spp is None:
            tile_spp = [done] * tiles
        data += struct.pack("<dii", rel_target, min_samples, pad) + np.asarray(tile_spp, np.int32).tobytes()
    return data + struct.pack("<Q", _fnv64(data) if fix_checksum else 0)


# ----------------------------------------------------------------------------------------------------------------- CPU --
def test_header_declares_and_library_exports_the_adaptive_api(rt):
    header = open(os.path.join(ROOT, "include", "rtk.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, body), name
    for typ in ("rtk_adaptive_opts", "rtk_adaptive_state"):
        assert re.search(r"typedef struct %s\b" % typ, body), typ
    assert "#define RTK_ABI_VERSION 2" in body
    lib = C.CDLL(rt.HIP_LIB_PATH)
    missing = [n for n in ENTRY_POINTS if not hasattr(lib, n)]
    assert not missing, missing
    assert C.sizeof(rt.AdaptiveOpts) == 16 and C.sizeof(rt.AdaptiveState) == 24


def test_version2_checkpoint_parses(rt):
    # 20 x 12: 3 x 2 tiles; two retired at 16 and 24, the others active at 32
    info = rt.checkpoint_info(_blob(rt, tile_spp=[16, 32, 24, 32, 32, 32]))
    spp = info.pop("tile_spp")
    assert info == {"version": 2, "width": 20, "height": 12, "rank": 0, "n_ranks": 1, "real_mode": 0, "target_spp": 48, "chunk_size": 8,
                    "samples_done": 32, "seed": 7, "scene_digest": 0x1122334455667788, "rel_target": 0.05, "min_samples": 16}
    assert spp.dtype == np.int32 and spp.tolist() == [16, 32, 24, 32, 32, 32]
    # a rank of several: its padding tile (past the last tile) holds 0 samples; a finished frame holds the target
    info = rt.checkpoint_info(_blob(rt, w=20, h=20, rank=1, n_ranks=2, target=40, done=40, min_samples=40, tile_spp=[40, 40, 40, 40, 0]))
    assert info["tile_spp"].tolist() == [40, 40, 40, 40, 0] and info["min_samples"] == 40
    # the raw entry point: a version-1 checkpoint has no adaptive part
    lib = rt.hip_lib()
    v1 = _blob(rt, version=1, adaptive_block=False)
    ad = rt.AdaptiveOpts(1.0, 5, 5)
    assert lib.rtk_checkpoint_read_adaptive(v1, len(v1), C.byref(ad), None) == 0
    assert (ad.rel_target, ad.min_samples, ad.reserved) == (0.0, 0, 0)


def test_version1_checkpoint_still_parses_to_the_same_dict(rt):
    info = rt.checkpoint_info(_blob(rt, version=1, adaptive_block=False, done=16))
    assert info == {"version": 1, "width": 20, "height": 12, "rank": 0, "n_ranks": 1, "real_mode": 0, "target_spp": 48, "chunk_size": 8,
                    "samples_done": 16, "seed": 7, "scene_digest": 0x1122334455667788}


@pytest.mark.parametrize("what", ["min_samples_not_chunk", "min_samples_one_chunk", "min_samples_over_target", "rel_target_zero", "rel_target_negative",
                                  "pad", "spp_over_target", "spp_over_done", "spp_not_chunk", "spp_under_min", "padding_tile_rendered", "truncated",
                                  "checksum", "v2_with_v1_size", "v1_with_v2_size"])
def test_version2_checkpoint_rejects_malformed_blobs(rt, what):
    good = _blob(rt)
    bad = {
        "min_samples_not_chunk": lambda: _blob(rt, min_samples=20),
        "min_samples_one_chunk": lambda: _blob(rt, min_samples=8),
        "min_samples_over_target": lambda: _blob(rt, min_samples=56),
        "rel_target_zero": lambda: _blob(rt, rel_target=0.0),
        "rel_target_negative": lambda: _blob(rt, rel_target=-0.1),
        "pad": lambda: _blob(rt, pad=1),
        "spp_over_target": lambda: _blob(rt, tile_spp=[56, 32, 32, 32, 32, 32]),
        "spp_over_done": lambda: _blob(rt, tile_spp=[40, 32, 32, 32, 32, 32]),
        "spp_not_chunk": lambda: _blob(rt, tile_spp=[20, 32, 32, 32, 32, 32]),
        "spp_under_min": lambda: _blob(rt, tile_spp=[8, 32, 32, 32, 32, 32]),
        "padding_tile_rendered": lambda: _blob(rt, w=20, h=20, rank=1, n_ranks=2, tile_spp=[32, 32, 32, 32, 32]),
        "truncated": lambda: good[:-40],
        "checksum": lambda: good[:300] + bytes([good[300] ^ 1]) + good[301:],
        "v2_with_v1_size": lambda: _blob(rt, version=2, adaptive_block=False),
        "v1_with_v2_size": lambda: _blob(rt, version=1),
    }[what]()
    with pytest.raises(rt.RtkError) as e:
        rt.checkpoint_info(bad)
    assert e.value.code == -1
    lib = rt.hip_lib()
    ad = rt.AdaptiveOpts()
    assert lib.rtk_checkpoint_read_adaptive(bad, len(bad), C.byref(ad), None) == -1


def test_argument_checks_without_a_device(rt):
    lib = rt.hip_lib()
    opts = rt.AdaptiveOpts(0.05, 16, 0)
    st = rt.AdaptiveState()
    out = (C.c_int32 * 4)()
    assert lib.rtk_progressive_set_adaptive(None, C.byref(opts)) == -1
    assert "null session" in lib.rtk_last_error().decode()
    assert lib.rtk_adaptive_status(None, C.byref(st)) == -1
    assert lib.rtk_adaptive_tile_samples(None, out) == -1
    assert lib.rtk_checkpoint_read_adaptive(None, 0, C.byref(opts), None) == -1
    good = _blob(rt)
    assert lib.rtk_checkpoint_read_adaptive(good, len(good), None, None) == -1
    # the option rules are the checkpoint reader's too: rel_target <= 0 and a bad min_samples are refused there without a device
    for rel, ms in ((0.0, 16), (-1.0, 16), (float("nan"), 16), (0.05, 12), (0.05, 8), (0.05, 0), (0.05, 64)):
        blob = _blob(rt, rel_target=rel, min_samples=ms)
        assert lib.rtk_checkpoint_read_adaptive(blob, len(blob), C.byref(opts), None) == -1, (rel, ms)


# ----------------------------------------------------------------------------------------------------------------- GPU --
def _sums_from_blob(blob, tiles, real_mode):
    elem = 8 if real_mode == 0 else 4
    body = np.frombuffer(blob, np.uint8, offset=256)
    s1 = np.frombuffer(body[tiles * 192 * elem: tiles * 192 * elem + tiles * 512].tobytes(), np.float64).reshape(tiles, 64)
    s2 = np.frombuffer(body[tiles * 192 * elem + tiles * 512: tiles * 192 * elem + tiles * 1024].tobytes(), np.float64).reshape(tiles, 64)
    return s1, s2


def _inside(w, h, tiles, n_ranks=1, rank=0):
    """[tiles, 64] bool: the slot is an in-image pixel."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    t = np.arange(tiles)[:, None] * n_ranks + rank
    lane = np.arange(64)[None, :]
    i, j = (t % tx) * 8 + (lane & 7), (t // tx) * 8 + (lane >> 3)
    return (t < tx * ty) & (i < w) & (j < h)


def _rel(s1, s2, k):
    """The noise estimate of include/rtk.h in numpy: (se, se / max(m, 1e-3)) over k full chunks."""
    m = s1 / k
    se = np.sqrt(np.maximum(0.0, (s2 - k * m * m) / (k - 1)) / k)
    return se, se / np.maximum(m, 1e-3)


def _tile_map(per_tile, w, h):
    """[tiles] of one rank of one -> (h, w)."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    return np.repeat(np.repeat(np.asarray(per_tile).reshape(ty, tx), 8, 0), 8, 1)[:h, :w]


def _small_scenes():
    # (scene, width, height, target, depth): 8-sample chunks.  (Not the Cornell box: at these sizes every tile has a pixel lit
    # in a single chunk, so every tile's metric is 1 at every step and no rel_target retires some tiles but not others.)
    return [("book1_final", 96, 56, 64, 8), ("material_zoo", 96, 54, 48, 8), ("three_spheres", 64, 40, 64, 8)]


def _uniform_metrics(renderer, cam, real_mode, step):
    """A non-adaptive session stepped to the target in steps of `step` (the last one may be shorter): per step end s, every tile's
    retire metric from the checkpoint's exact S1 / S2."""
    w, h, target = cam.image_width, cam.image_height, cam.samples_per_pixel
    tiles = _tiles(w, h, 1)
    inside = _inside(w, h, tiles)
    p = renderer.progressive(cam, real_mode=real_mode)
    metrics = {}
    while p.samples_done < target:
        p.step(min(step, target - p.samples_done))
        s = p.samples_done
        if s // 8 >= 2:
            s1, s2 = _sums_from_blob(p.save(), tiles, real_mode)
            _, rel = _rel(s1, s2, s // 8)
            metrics[s] = np.where(inside, rel, 0.0).max(1)
    p.close()
    return metrics


def _expected_spp(metrics, rel_target, min_samples, target):
    """The retire rule replayed: (expected tile_spp, tiles whose metric is within 1e-9 relative of rel_target somewhere)."""
    tiles = len(next(iter(metrics.values())))
    spp = np.full(tiles, target, np.int32)
    near = np.zeros(tiles, bool)
    for s in sorted(metrics):
        if not (min_samples <= s < target):
            continue
        live = spp == target
        near |= live & (np.abs(metrics[s] - rel_target) <= 1e-9 * rel_target)
        spp[live & (metrics[s] <= rel_target)] = s
    return spp, near


def _run_adaptive(renderer, cam, real_mode, rel_target, min_samples, step, count=False, **kw):
    p = renderer.progressive(cam, real_mode=real_mode, rel_target=rel_target, min_samples=min_samples, **kw)
    total, actives = None, []
    while p.samples_done < cam.samples_per_pixel:
        out = p.step(min(step, cam.samples_per_pixel - p.samples_done), count=count)
        if count:
            total = out[3] if total is None else {k: total[k] + out[3][k] for k in out[3]}
        actives.append(p.adaptive_status()["active_tiles"])
    linear, rgb8, noise = out[:3]
    return p, linear, rgb8, noise, total, actives


def _pick_rel_target(metrics, min_samples, target):
    """A rel_target under which, by the rule replayed on a uniform session, some tiles retire early and some reach the target:
    the midpoint between two distinct metrics at min_samples that splits the tiles most evenly.  (The metric of a tile is a
    maximum over 64 pixels: where one pixel saw light in a single chunk only, se / m is exactly 1, and in a dim scene such as
    the Cornell box every lit tile then sits at 1.)"""
    values = np.unique(metrics[min_samples])
    best, best_split = None, 0
    for lo, hi in zip(values[:-1], values[1:]):
        if hi - lo <= 1e-6 * hi:
            continue
        rel_target = float(lo + hi) / 2
        spp, _ = _expected_spp(metrics, rel_target, min_samples, target)
        split = min(int((spp < target).sum()), int((spp == target).sum()))
        if split > best_split:
            best, best_split = rel_target, split
    assert best_split >= 2, ("no rel_target splits the tiles", {s: np.quantile(v, [0, 0.25, 0.5, 0.75, 1]).tolist() for s, v in metrics.items()})
    return best


def _median_rel_target(metrics, min_samples, target, share=0.1):
    """_pick_rel_target for thousands of tiles, one replay per try: the midpoint between the two adjacent distinct metrics at
    min_samples nearest their median.  At least `share` of the tiles must retire early and as many reach the target; tiles
    above the median may still retire at a later step, so where too few would reach the target the next tries take lower
    quantiles instead of the median."""
    values = np.unique(metrics[min_samples])
    assert len(values) >= 2, "every tile has the same metric"
    tries = []
    for q in (0.5, 0.4, 0.3, 0.2):
        k = int(np.clip(np.searchsorted(values, np.quantile(metrics[min_samples], q)), 1, len(values) - 1))
        lo, hi = values[k - 1], values[k]
        if hi - lo <= 1e-6 * hi:
            continue
        rel_target = float(lo + hi) / 2
        spp, _ = _expected_spp(metrics, rel_target, min_samples, target)
        early, full = int((spp < target).sum()), int((spp == target).sum())
        if min(early, full) >= share * len(spp):
            return rel_target
        tries.append((q, rel_target, early, full))
    raise AssertionError(("no rel_target near the median splits the tiles", tries))


def test_median_rel_target_on_synthetic_metrics():
    rng = np.random.default_rng(9)
    n = 5001
    m16 = rng.random(n)
    metrics = {16: m16, 24: m16 * 0.95, 32: m16 * 0.9, 40: m16 * 0.85}
    rel = _median_rel_target(metrics, 16, 48)
    below = np.sort(m16)[n // 2 - 1:n // 2 + 2]
    assert below[0] < rel < below[2] and np.sum(m16 <= rel) in (n // 2, n // 2 + 1)
    spp, near = _expected_spp(metrics, rel, 16, 48)
    # the replay: a tile retires at the first step end whose metric meets rel_target
    want = np.full(n, 48)
    for s in (40, 32, 24, 16):
        want[metrics[s] <= rel] = s
    assert np.array_equal(spp, want) and not near.any()
    # the slow picker agrees with the rule on a small draw; a constant metric is refused; so is a split under the share
    small = {16: m16[:40], 24: m16[:40] * 0.8}
    assert 0 < np.sum(_expected_spp(small, _pick_rel_target(small, 16, 32), 16, 32)[0] < 32) < 40
    with pytest.raises(AssertionError):
        _median_rel_target({16: np.full(100, 0.5), 24: np.full(100, 0.4)}, 16, 32)
    skew = np.where(np.arange(100) < 95, 0.0, 1.0) + np.arange(100) * 1e-3
    with pytest.raises(AssertionError):
        _median_rel_target({16: skew, 24: skew * 0.99}, 16, 32, share=0.6)


def _unreachable(rt, renderer, real_mode=0):
    """A small scene whose every tile's metric stays above 0 (a flat background tile -- every sample alike -- has metric 0 and
    retires under any rel_target), and half its smallest metric: (scene, cam, name, w, h, target, depth, rel_target).  The
    Cornell box qualifies: every tile's metric is 1."""
    for name, w, h, target, depth in [("cornell_box", 64, 64, 96, 6)] + _small_scenes():
        scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
        renderer.upload(scene)
        cam = scene.camera(w, h, target, depth)
        metrics = _uniform_metrics(renderer, cam, real_mode, 8)
        low = min(v.min() for s, v in metrics.items() if 16 <= s < target)
        if low > 1e-6:
            return scene, cam, name, w, h, target, depth, low / 2
    raise AssertionError("every small scene has a flat tile")


def _adaptive_cases(case):
    """(scene, width, height, target, depth, min_samples, step) of test_every_tile_equals_a_one_shot_render_at_its_own_count.
    ragged: 43 x 33 = 1 419 tiles -- two 1 024-position windows of the compaction kernel, a partial last row and column and
    n_tiles % 4 == 3.  full_hd: 32 400 tiles, target 512 in 8-sample chunks, so a 192-sample step is 24 chunk planes, two launches
    (21 per launch); tiles retire at 192 and 384, and the second step renders the active tiles only, in two launches."""
    if case == "small":
        return [(name, w, h, target, depth, 16, 8) for name, w, h, target, depth in _small_scenes()]
    if case == "ragged":
        return [("book1_final", 340, 260, 64, 8, 16, 8)]
    assert case == "full_hd"
    return [("book1_final", 1920, 1080, 512, 8, 192, 192)]


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode,case", [(0, "small"), (1, "small"), (0, "ragged"), (1, "ragged"), (0, "full_hd")],
                         ids=["0", "1", "ragged-f64", "ragged-f32", "full_hd-f64"])
def test_every_tile_equals_a_one_shot_render_at_its_own_count(rt, renderer, real_mode, case):
    """The invariant, plus: retire decisions agree with the rule replayed in numpy on a uniform session's exact noise sums, the step
    work counters add up to the tile map, and the noise statistics use each tile's own K."""
    for name, w, h, target, depth, min_samples, step in _adaptive_cases(case):
        scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
        renderer.upload(scene)
        cam = scene.camera(w, h, target, depth)
        if case == "full_hd":
            launches = rt.hip_lib().rtk_frame_launches(C.byref(scene.camera(w, h, step, depth)), C.byref(rt.RenderOpts(rt.RENDER_SEED, 0, 0, 1, 0, 0, None)))
            probe = renderer.progressive(cam)
            assert launches >= 2 and probe.chunk_size == 8, launches
            probe.close()
        metrics = _uniform_metrics(renderer, cam, real_mode, step)
        if case == "small":
            rel_target = _pick_rel_target(metrics, min_samples, target)
        else:
            assert _tiles(w, h, 1) > 1024
            rel_target = _median_rel_target(metrics, min_samples, target)
        p, linear, rgb8, noise, counters, actives = _run_adaptive(renderer, cam, real_mode, rel_target, min_samples, step, count=True)
        spp = p.tile_samples()
        expected, near = _expected_spp(metrics, rel_target, min_samples, target)
        assert np.array_equal(spp[~near], expected[~near]), name
        assert (spp < target).any() and (spp == target).any(), (name, np.unique(spp))
        assert actives == sorted(actives, reverse=True)             # retired tiles never come back
        smap = p.sample_map()
        assert np.array_equal(smap, _tile_map(spp, w, h))
        for s in np.unique(spp):
            ref, ref8, _ = renderer.render_host(scene.camera(w, h, int(s), depth), real_mode=real_mode)
            sel = smap == s
            assert np.array_equal(linear[sel], ref[sel]), (name, s)
            assert np.array_equal(rgb8[sel], ref8[sel]), (name, s)
        # work: the counting kernels rendered exactly the tile map's samples
        px = _inside(w, h, len(spp)).sum(1)
        assert counters["samples"] == int((px * spp).sum()), name
        st = p.adaptive_status()
        assert st["pixel_samples"] == int((px * spp).sum()) and st["retired_tiles"] == int((spp < target).sum())
        assert st["active_tiles"] + st["retired_tiles"] == len(spp)
        np.testing.assert_allclose(st["mean_spp"], (px * spp).sum() / (w * h), rtol=1e-12)
        # the per-pixel se of the last preview and the frame statistics: per-tile K from the session's own sums
        s1, s2 = _sums_from_blob(p.save(), len(spp), real_mode)
        k = (spp // 8)[:, None].astype(np.float64)
        se, rel = _rel(s1, s2, k)
        inside = _inside(w, h, len(spp))
        np.testing.assert_allclose(noise, _tile_image(se, w, h).astype(np.float32), rtol=1e-6, atol=0)
        stats = p.noise()
        np.testing.assert_allclose(stats["mean_se"], se[inside].mean(), rtol=1e-9)
        np.testing.assert_allclose(stats["max_se"], se[inside].max(), rtol=1e-12)
        np.testing.assert_allclose(stats["mean_rel_se"], rel[inside].mean(), rtol=1e-9)
        p.close()


@pytest.mark.gpu
def test_identical_runs_and_an_unreachable_target(rt, renderer):
    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    w, h, target = 80, 48, 64
    cam = scene.camera(w, h, target, 6)
    renderer.upload(scene)
    rel_target = _pick_rel_target(_uniform_metrics(renderer, cam, 0, 8), 24, target)
    runs = []
    for _ in range(2):
        p, linear, rgb8, noise, _, actives = _run_adaptive(renderer, cam, 0, rel_target, 24, 8)
        runs.append((linear, rgb8, noise, p.tile_samples(), actives, p.save()))
        p.close()
    a, b = runs
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] and a[5] == b[5]
    assert 0 < a[4][-1] < (w // 8) * (h // 8)
    # nothing retires: the finished frame is the one-shot frame
    flat, flat_cam, _, _, _, flat_target, _, low = _unreachable(rt, renderer)
    one, one8, _ = renderer.render_host(flat_cam)
    p, linear, rgb8, _, _, actives = _run_adaptive(renderer, flat_cam, 0, low, 16, 16)
    assert np.array_equal(linear, one) and np.array_equal(rgb8, one8)
    assert (p.tile_samples() == flat_target).all() and p.adaptive_status()["retired_tiles"] == 0
    p.close()
    renderer.upload(scene)
    # everything retires at min_samples: a later step is valid, changes no pixel, and renders nothing
    p = renderer.progressive(cam, rel_target=1e9, min_samples=16)
    p.step(16)
    st = p.adaptive_status()
    assert st["active_tiles"] == 0 and st["pixel_samples"] == w * h * 16
    before, before8, _ = p.step(8)
    after, after8, _, cnt = p.step(8, count=True)
    ref, ref8, _ = renderer.render_host(scene.camera(w, h, 16, 6))
    assert np.array_equal(before, ref) and np.array_equal(after, ref) and np.array_equal(after8, ref8)
    assert cnt["samples"] == 0 and p.samples_done == 32
    p.close()


@pytest.mark.gpu
def test_set_adaptive_rules(rt, renderer):
    scene = rt.Scene.build("three_spheres", rt.SCENE_SEED)
    renderer.upload(scene)
    cam = scene.camera(32, 24, 48, 4)
    for rel, ms in ((0.0, 16), (-0.5, 16), (0.1, 12), (0.1, 8), (0.1, 56)):
        with pytest.raises(rt.RtkError) as e:
            renderer.progressive(cam, rel_target=rel, min_samples=ms)
        assert e.value.code == -1, (rel, ms)
    p = renderer.progressive(cam)
    p.step(8)
    rc = p._lib.rtk_progressive_set_adaptive(p._h, C.byref(rt.AdaptiveOpts(0.1, 16, 0)))
    assert rc == -1 and "before the first step" in p._lib.rtk_last_error().decode()
    st = p.adaptive_status()                          # a plain session: every tile active at samples_done
    assert st == {"active_tiles": 12, "retired_tiles": 0, "pixel_samples": 32 * 24 * 8, "mean_spp": 8.0}
    assert (p.tile_samples() == 8).all()
    p.close()


@pytest.mark.gpu
def test_resume_in_a_fresh_context_equals_an_uninterrupted_run(rt, tmp_path):
    scene = rt.Scene.build("material_zoo", rt.SCENE_SEED, EARTH)
    w, h, target = 96, 54, 64
    cam = scene.camera(w, h, target, 8)
    r = rt.Renderer(0)
    r.upload_fast(scene, cam.center)
    rel_target = _pick_rel_target(_uniform_metrics(r, cam, 1, 8), 16, target)
    p, whole, whole8, whole_noise, _, _ = _run_adaptive(r, cam, 1, rel_target, 16, 8)
    whole_spp = p.tile_samples()
    p.close()
    p = r.progressive(cam, real_mode=1, rel_target=rel_target, min_samples=16)
    for _ in range(4):
        p.step(8)
    mid_spp = p.tile_samples()
    assert (mid_spp < 32).any()                      # some tiles retired before the checkpoint
    blob = p.save()
    info = rt.checkpoint_info(blob)
    assert info["version"] == 2 and info["samples_done"] == 32 and info["rel_target"] == rel_target and info["min_samples"] == 16
    assert np.array_equal(info["tile_spp"], mid_spp)
    p.close()
    r.close()

    r2 = rt.Renderer(0)
    r2.upload_fast(scene, cam.center)
    q = r2.resume(cam, blob, real_mode=1)
    assert np.array_equal(q.tile_samples(), mid_spp) and q.samples_done == 32
    while q.samples_done < target:
        linear, rgb8, noise = q.step(8)
    assert np.array_equal(linear, whole) and np.array_equal(rgb8, whole8) and np.array_equal(noise, whole_noise)
    assert np.array_equal(q.tile_samples(), whole_spp)
    q.close()
    r2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_resume_above_1024_tiles_equals_an_uninterrupted_run(rt, real_mode):
    """Case "ragged" of test_every_tile_equals_a_one_shot_render_at_its_own_count, saved at 32 samples: the resumed session
    recomputes its retired tiles (rtk_adaptive_restore_kernel) and compacts 1 419 tiles in two windows with no learned order."""
    name, w, h, target, depth, min_samples, step = _adaptive_cases("ragged")[0]
    scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
    cam = scene.camera(w, h, target, depth)
    r = rt.Renderer(0)
    r.upload(scene)
    rel_target = _median_rel_target(_uniform_metrics(r, cam, real_mode, step), min_samples, target)
    p, whole, whole8, whole_noise, _, _ = _run_adaptive(r, cam, real_mode, rel_target, min_samples, step)
    whole_spp, whole_blob, whole_stats = p.tile_samples(), p.save(), p.noise()
    p.close()
    p = r.progressive(cam, real_mode=real_mode, rel_target=rel_target, min_samples=min_samples)
    while p.samples_done < 32:
        p.step(step)
    mid_spp = p.tile_samples()
    active = p.adaptive_status()["active_tiles"]
    # retired tiles, and tiles still at 32 samples in both 1 024-tile windows (a resumed session compacts in tile order)
    assert (mid_spp < 32).any() and (mid_spp[:1024] == 32).any() and (mid_spp[1024:] == 32).any() and active > 0, (np.unique(mid_spp), active)
    blob = p.save()
    p.close()
    r.close()

    r2 = rt.Renderer(0)
    r2.upload(scene)
    q = r2.resume(cam, blob, real_mode=real_mode)
    assert np.array_equal(q.tile_samples(), mid_spp) and q.adaptive_status()["active_tiles"] == active
    while q.samples_done < target:
        linear, rgb8, noise = q.step(step)
    assert np.array_equal(linear, whole) and np.array_equal(rgb8, whole8) and np.array_equal(noise, whole_noise)
    assert np.array_equal(q.tile_samples(), whole_spp) and q.noise() == whole_stats
    assert q.save() == whole_blob
    q.close()
    r2.close()


@pytest.mark.gpu
def test_two_ranks_on_one_device_equal_one_rank(rt, renderer):
    from raytracingoneweekendapplication_amd.tiling import image_from_gathered

    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    w, h = 84, 50                                         # partial tiles at the right and bottom edges; rank 1 has a padding tile
    cam = scene.camera(w, h, 48, 6)
    renderer.upload(scene)
    rel_target = _pick_rel_target(_uniform_metrics(renderer, cam, 0, 8), 16, 48)
    whole = renderer.progressive(cam, rel_target=rel_target, min_samples=16)
    ranks = [renderer.progressive(cam, rank=k, n_ranks=2, rel_target=rel_target, min_samples=16) for k in range(2)]
    for n in (8, 8, 16, 8, 8):
        ref, _, ref_noise = whole.step(n)
        parts = [r.step(n) for r in ranks]
        assert np.array_equal(image_from_gathered(np.stack([lin for lin, _, _ in parts]), w, h, 2), ref)
        noise = image_from_gathered(np.stack([nz[:, None, :].repeat(3, 1) for _, _, nz in parts]), w, h, 2)[..., 0]
        assert np.array_equal(noise, ref_noise)
        maps = [r.sample_map() for r in ranks]
        assert np.array_equal(maps[0] + maps[1], whole.sample_map())
    assert (whole.tile_samples() < 48).any()
    assert sum(r.adaptive_status()["pixel_samples"] for r in ranks) == whole.adaptive_status()["pixel_samples"]
    assert ranks[1].tile_samples()[-1] == 0              # the padding tile
    for r in ranks + [whole]:
        r.close()


@pytest.mark.gpu
def test_scene_change_fails_later_steps(rt, renderer):
    scene = rt.Scene.build("book1_final", rt.SCENE_SEED)
    cam = scene.camera(64, 40, 48, 6)
    renderer.upload(scene)
    p = renderer.progressive(cam, rel_target=0.1, min_samples=16)
    p.step(16)
    renderer.upload(rt.Scene.build("three_spheres", rt.SCENE_SEED))
    with pytest.raises(rt.RtkError, match="scene changed"):
        p.step(8)
    assert p.samples_done == 16
    p.close()


@pytest.mark.gpu
def test_cpp_camera_adaptive_render(rt, tmp_path):
    """camera::render() with progressive_step and adaptive_target: stops at the target or when no tile is active and reports
    last_adaptive; a target no tile reaches writes the one-shot PNG's bytes.  (The helper builds the library scene as
    librtk_host.so does; camera::order = auto_order takes the fast order only where it is bit-identical.)"""
    import json
    import subprocess

    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "adaptive_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "adaptive_camera_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])

    def run(out, name, w, h, target, depth, never, mid):
        out.mkdir()
        text = subprocess.check_output([exe, str(out), name, EARTH, str(w), str(h), str(target), str(depth), repr(never), repr(mid)],
                                       timeout=300).decode()
        return json.loads(text.strip().splitlines()[-1])

    r = rt.Renderer(0)
    _, _, name, w, h, target, depth, low = _unreachable(rt, r)
    name2, w2, h2, target2, depth2 = _small_scenes()[0]
    scene2 = rt.Scene.build(name2, rt.SCENE_SEED, EARTH)
    r.upload(scene2)
    rel_target = _pick_rel_target(_uniform_metrics(r, scene2.camera(w2, h2, target2, depth2), 0, 8), 16, target2)
    r.close()

    v = run(tmp_path / "a", name, w, h, target, depth, low, low)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert (tmp_path / "a" / "never.png").read_bytes() == (tmp_path / "a" / "one.png").read_bytes()
    assert (v["never_done"], v["never_rendered"], v["never_active"], v["never_retired"], v["never_pixel_samples"]) == (target, target, tiles, 0, w * h * target)
    # a target every tile meets at once: render() stops when no tile is active
    assert (v["all_done"], v["all_active"], v["all_retired"], v["all_pixel_samples"], v["all_rendered"]) == (16, 0, tiles, 16 * w * h, 16)

    # a middling target: some tiles retire, the rest reach the target
    v = run(tmp_path / "b", name2, w2, h2, target2, depth2, rel_target, rel_target)
    tiles = ((w2 + 7) // 8) * ((h2 + 7) // 8)
    assert v["mid_done"] == target2 and v["mid_active"] + v["mid_retired"] == tiles and 0 < v["mid_retired"] < tiles
    assert 16 * w2 * h2 < v["mid_pixel_samples"] < target2 * w2 * h2
    assert abs(v["mid_mean_spp"] - v["mid_pixel_samples"] / (w2 * h2)) < 1e-9
