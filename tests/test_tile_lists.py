"""Tile lists (include/rtk.h, "Tile lists"): rtk_tiles_select against the numpy restatement of its rule (tests/tile_rules.py),
rtk_render_tiles against the frame rtk_render_host renders and the noise a one-step progressive session writes, and what is
built on the two: Renderer.upsample_refined and camera::refine_support.

CPU tests: declarations, the option struct's layout, every refusal that needs no device, the restatement's own properties.
GPU tests (-m gpu): flag for flag, bit for bit and byte for byte; pixels of unflagged tiles keep the sentinel they held.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_matrix as km
from tests import tile_rules as tr
from tests.conftest import EARTH, ROOT
from tests.scene_cases import RENDER_SEED

ENTRY_POINTS = ("rtk_tiles_select", "rtk_tiles_select_host", "rtk_render_tiles", "rtk_render_tiles_host")
W, H = 37, 23                          # 5 x 3 tiles, partial on the right and bottom edges
SPPS = (1, 8, 9, 20)                   # one chunk, one full chunk, a full and a partial one, three chunks with the last partial
SENTINEL = {"linear": -7.25, "rgb8": 0xA5, "noise": -3.0, "support": -5.0}     # (exact in float32: the F32 host form rounds and widens)


def _header():
    with open(os.path.join(ROOT, "include", "rtk.h")) as f:
        return f.read()


def _err(rt):
    return rt.hip_lib().rtk_last_error().decode()


def sentinels(w, h):
    return {"linear": np.full((h, w, 3), SENTINEL["linear"]), "rgb8": np.full((h, w, 3), SENTINEL["rgb8"], np.uint8),
            "noise": np.full((h, w), SENTINEL["noise"], np.float32), "support": np.full((h, w), SENTINEL["support"], np.float32)}


def assert_tiles(got, flags, w, h, want):
    """got = (linear, rgb8, noise, support): `want[name]` (where given) at the pixels of flagged tiles, the sentinel elsewhere."""
    m = tr.pixel_mask(flags, w, h)
    for name, img in zip(("linear", "rgb8", "noise", "support"), got):
        assert (img[~m] == SENTINEL[name]).all(), name
        if name in want:
            assert np.array_equal(img[m], want[name][m]), name


# ------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_and_exported_and_the_abi_version_stays(rt):
    header = _header()
    lib = rt.hip_lib()
    assert "Tile lists ---" in header
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert getattr(lib, name) is not None
    assert re.search(r"^#define RTK_ABI_VERSION 2$", header, re.M) and lib.rtk_abi_version() == 2
    for name in ("tiles_select", "tiles_select_device", "render_tiles", "render_tiles_device", "upsample_refined"):
        assert callable(getattr(rt.Renderer, name)), name
    assert callable(rt.tile_flags_from_mask)


def test_option_struct_layout_matches_the_header(rt, tmp_path):
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rtk.h"\nint main(void) {\n'
                '    printf("%zu %zu %zu %zu %zu\\n", sizeof(rtk_tile_select_opts), offsetof(rtk_tile_select_opts, below), offsetof(rtk_tile_select_opts, above),\n'
                '           offsetof(rtk_tile_select_opts, dilate), offsetof(rtk_tile_select_opts, reserved));\n    return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    T = rt.TileSelectOpts
    assert got == [16, 0, 4, 8, 12]
    assert got == [C.sizeof(T), T.below.offset, T.above.offset, T.dilate.offset, T.reserved.offset]
    assert "sizeof(rtk_tile_select_opts) = 16" in _header()


def test_new_sources_are_built_into_the_library():
    import __graft_entry__ as g

    assert "rtk_tiles.hip" in g.HIP_SOURCES and "rtk_frame.hip" in g.HIP_SOURCES
    assert all(os.path.exists(p) for p in g.hip_dependencies())


def test_select_refusals_need_no_device_and_write_nothing(rt):
    lib = rt.hip_lib()
    T = rt.TileSelectOpts
    w, h = 16, 16
    m = np.zeros((h, w), np.float32)
    flags = np.full(4, -9, np.int32)
    ok = T(0.5, 0.5, 1, 0)
    mp, fp = m.ctypes.data, flags.ctypes.data
    nan, inf = float("nan"), float("inf")
    cases = [((None, 0, h, mp, None, ok, fp), "image size"), ((None, w, 65537, mp, None, ok, fp), "image size"), ((None, w, h, None, None, ok, fp), "both null"),
             ((None, w, h, mp, None, ok, None), "d_tile_flags"), ((None, w, h, mp, None, None, fp), "opts"), ((None, w, h, mp, None, T(0.5, 0.5, -1, 0), fp), "dilate"),
             ((None, w, h, mp, None, T(0.5, 0.5, 9, 0), fp), "dilate"), ((None, w, h, mp, None, T(nan, 0.5, 0, 0), fp), "below"),
             ((None, w, h, None, mp, T(0.5, inf, 0, 0), fp), "above"), ((None, w, h, mp, mp, T(0.5, -inf, 0, 0), fp), "above"),
             ((None, w, h, mp, None, T(0.5, 0.5, 0, 1), fp), "reserved"), ((None, w, h, mp + 2, None, ok, fp), "d_below_map"),
             ((None, w, h, None, mp + 1, ok, fp), "d_above_map"), ((None, w, h, mp, None, ok, fp + 2), "d_tile_flags"), ((None, w, h, mp, None, ok, fp), "null context")]
    for args, word in cases:
        ctx, ww, hh, b, a, o, f = args
        for name in ("rtk_tiles_select", "rtk_tiles_select_host"):
            extra = (None,) if name == "rtk_tiles_select" else ()
            rc = getattr(lib, name)(ctx, ww, hh, b, a, C.byref(o) if o is not None else None, f, *extra)
            assert rc == -1 and name + ":" in _err(rt) and word in _err(rt), (name, word, _err(rt))
    # a non-finite threshold of a map that is not given is not read
    assert lib.rtk_tiles_select(None, w, h, mp, None, C.byref(T(0.5, nan, 0, 0)), fp, None) == -1 and "null context" in _err(rt)
    assert (flags == -9).all()


def test_render_tiles_refusals_that_need_no_device(rt):
    lib = rt.hip_lib()
    cam = rt.derive_camera(W, W / H, spp=8, max_depth=5)
    assert (cam.image_width, cam.image_height) == (W, H)
    n = rt.tiles_per_rank(W, H, 1)
    flags = np.ones(n, np.int32)
    lin, rgb8 = np.full((H, W, 3), -7.25), np.full((H, W, 3), 0xA5, np.uint8)
    noise, support, info = np.full((H, W), -3.0, np.float32), np.full((H, W), -5.0, np.float32), np.full(2, -9, np.int32)
    outs = (lin.ctypes.data, rgb8.ctypes.data, noise.ctypes.data, support.ctypes.data, info.ctypes.data)
    opts = lambda mode=0, rank=0, ranks=1, variant=0: rt.RenderOpts(RENDER_SEED, mode, rank, ranks, 0, variant, None)  # noqa: E731

    def changed(**kw):
        c = rt.Camera.from_buffer_copy(bytes(cam))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    big = rt.derive_camera(1920, 16.0 / 9.0, spp=176, max_depth=5)
    assert lib.rtk_frame_launches(C.byref(big), C.byref(opts())) == 2 and lib.rtk_frame_launches(C.byref(big), C.byref(opts(1))) == 1
    fp = flags.ctypes.data
    cases = [(changed(image_width=0), opts(), fp, 0, outs, "camera"), (changed(samples_per_pixel=0), opts(), fp, 0, outs, "camera"),
             (changed(samples_per_pixel=40000), opts(), fp, 0, outs, "camera"), (changed(max_depth=-1), opts(), fp, 0, outs, "camera"),
             (cam, opts(ranks=2), fp, 0, outs, "n_ranks"), (cam, opts(rank=1, ranks=2), fp, 0, outs, "n_ranks"), (cam, opts(mode=2), fp, 0, outs, "real_mode"),
             (cam, opts(variant=1 << 22), fp, 0, outs, "variant"), (cam, opts(), None, 0, outs, "flags"), (cam, opts(), fp, -1, outs, "max_tiles"),
             (cam, opts(), fp, 0, (None, None, None, None, outs[4]), "no output"), (cam, opts(), fp + 2, 0, outs, "d_tile_flags"),
             (cam, opts(), fp, 0, (outs[0] + 4,) + outs[1:], "d_linear"), (cam, opts(), fp, 0, outs[:2] + (outs[2] + 2,) + outs[3:], "d_noise"),
             (cam, opts(), fp, 0, outs[:3] + (outs[3] + 1, outs[4]), "d_support"), (cam, opts(), fp, 0, outs[:4] + (outs[4] + 2,), "d_info"),
             (big, opts(), fp, 0, outs, "launches"), (cam, opts(), fp, 0, outs, "null context")]
    for c, o, f, max_tiles, out, word in cases:
        assert lib.rtk_render_tiles(None, C.byref(c), C.byref(o), f, max_tiles, *out) == -1, word
        assert "rtk_render_tiles:" in _err(rt) and word in _err(rt), (word, _err(rt))
    assert lib.rtk_render_tiles(None, C.byref(cam), C.byref(opts(1)), fp, 0, outs[0] + 4, *outs[1:]) == -1 and "null context" in _err(rt)   # floats: 4 bytes
    assert lib.rtk_render_tiles(None, None, C.byref(opts()), fp, 0, *outs) == -1 and lib.rtk_render_tiles(None, C.byref(cam), None, fp, 0, *outs) == -1
    # the host form: its own null checks, then the device form's
    host = lambda c, o, f, mt, out: lib.rtk_render_tiles_host(None, C.byref(c), C.byref(o), f, mt, *out)  # noqa: E731
    assert host(cam, opts(), None, 0, outs) == -1 and "h_tile_flags" in _err(rt)
    assert host(cam, opts(), fp, 0, (None, None, None, None, outs[4])) == -1 and "no output" in _err(rt)
    assert host(cam, opts(), fp, -1, outs) == -1 and "max_tiles" in _err(rt)
    assert host(cam, opts(ranks=2), fp, 0, outs) == -1 and "n_ranks" in _err(rt)
    assert host(big, opts(), fp, 0, outs) == -1 and "launches" in _err(rt)
    assert host(cam, opts(), fp, 0, outs) == -1 and "null context" in _err(rt)
    assert (lin == -7.25).all() and (rgb8 == 0xA5).all() and (noise == -3.0).all() and (support == -5.0).all() and (info == -9).all()


def test_the_restatement_has_the_rules_properties(rt):
    nan = np.float32("nan")
    one = lambda v: np.full((1, 1), v, np.float32)  # noqa: E731
    assert tr.select(below_map=one(nan), below=0.5)[0] == 1 and tr.select(above_map=one(nan), above=0.5)[0] == 1          # a NaN flags
    assert tr.select(below_map=one(0.5), below=0.5)[0] == 0 and tr.select(above_map=one(0.5), above=0.5)[0] == 0          # equality does not
    assert tr.select(below_map=one(np.nextafter(np.float32(0.5), np.float32(0))), below=0.5)[0] == 1
    assert tr.select(above_map=one(np.nextafter(np.float32(0.5), np.float32(1))), above=0.5)[0] == 1
    assert tr.select(below_map=one(1.0), above_map=one(1.0), below=0.5, above=0.5)[0] == 1                                # OR of the two
    assert tr.select(below_map=one(np.float32("inf")), below=0.5)[0] == 0 and tr.select(below_map=one(-np.float32("inf")), below=0.5)[0] == 1
    rng = np.random.default_rng(3)
    m = rng.random((23, 37)).astype(np.float32)
    prev = tr.select(below_map=m, below=0.01, dilate=0)
    assert 0 < prev.sum() < prev.size
    for r in range(1, 9):                                          # dilation is monotone in r
        cur = tr.select(below_map=m, below=0.01, dilate=r)
        assert (cur >= prev).all()
        prev = cur
    raw = np.zeros((8, 40), bool)
    raw[3, 7] = True                                               # x = 7 of tile 0: r = 8 reaches x = 15, the last column of tile 1, not tile 2
    assert list(tr.dilate_to_tiles(raw, 8)) == [1, 1, 0, 0, 0] and list(tr.dilate_to_tiles(raw, 0)) == [1, 0, 0, 0, 0]
    assert list(tr.dilate_to_tiles(raw, 1)) == [1, 1, 0, 0, 0]
    raw[:] = False
    raw[3, 6] = True
    assert list(tr.dilate_to_tiles(raw, 1)) == [1, 0, 0, 0, 0] and list(tr.dilate_to_tiles(raw, 2)) == [1, 1, 0, 0, 0]
    edge = np.zeros((9, 9), bool)
    edge[8, 8] = True                                              # the corner tile of a 9 x 9 image is one pixel
    assert list(tr.dilate_to_tiles(edge, 0)) == [0, 0, 0, 1] and list(tr.dilate_to_tiles(edge, 1)) == [1, 1, 1, 1]


def test_tile_flags_from_mask_is_the_rule_without_dilation(rt):
    rng = np.random.default_rng(11)
    for w, h in ((1, 1), (5, 1), (8, 8), (9, 9), (37, 23), (64, 48)):
        for density in (0.0, 0.02, 1.0):
            mask = rng.random((h, w)) < density
            flags = rt.tile_flags_from_mask(mask)
            assert flags.dtype == np.int32 and flags.shape == (rt.tiles_per_rank(w, h, 1),)
            assert np.array_equal(flags, tr.dilate_to_tiles(mask, 0)), (w, h, density)
    with pytest.raises(ValueError):
        rt.tile_flags_from_mask(np.zeros(5, bool))


# ------------------------------------------------------------------------------------------------ GPU: select
def select_maps(w, h, seed):
    """{name: (below map, above map)}; thresholds 0.02 / 0.98 flag about 2 % of the random pixels each."""
    rng = np.random.default_rng(seed)
    below, above = np.float32(0.02), np.float32(0.98)
    random = (rng.random((h, w)).astype(np.float32), rng.random((h, w)).astype(np.float32))
    nans = (np.full((h, w), np.nan, np.float32),) * 2
    inf = tuple(rng.choice(np.array([np.inf, -np.inf, 0.5], np.float32), (h, w), p=[0.02, 0.02, 0.96]) for _ in range(2))
    eq_b, eq_a = np.full((h, w), below, np.float32), np.full((h, w), above, np.float32)
    few = rng.random((h, w)) < 0.01
    eq_b[few] = np.nextafter(below, np.float32(0))
    eq_a[few] = np.nextafter(above, np.float32(1))
    return {"random": random, "nan": nans, "inf": inf, "equal": (eq_b, eq_a), "exactly equal": (np.full((h, w), below, np.float32), np.full((h, w), above, np.float32))}


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (5, 1), (8, 8), (9, 9), (37, 23), (64, 48), (264, 264)], ids=lambda s: "%dx%d" % s)
def test_select_equals_the_restatement_flag_for_flag(rt, renderer, size):
    import torch

    w, h = size
    n = rt.tiles_per_rank(w, h, 1)
    seen = set()
    for name, (mb, ma) in select_maps(w, h, 100 * w + h).items():
        db, da = torch.from_numpy(mb).to("cuda:0"), torch.from_numpy(ma).to("cuda:0")
        for mode in ("below", "above", "both"):
            b, a = (mb if mode != "above" else None), (ma if mode != "below" else None)
            for dilate in (0, 1, 3, 8):
                want = tr.select(b, a, 0.02, 0.98, dilate)
                buf = torch.full((n + 8,), -77, dtype=torch.int32, device="cuda:0")       # sentinel words around the flags
                renderer.tiles_select_device(w, h, db.data_ptr() if b is not None else 0, da.data_ptr() if a is not None else 0, buf.data_ptr() + 16,
                                             below=0.02, above=0.98, dilate=dilate)
                got = buf.cpu().numpy()
                assert (got[:4] == -77).all() and (got[4 + n:] == -77).all(), (name, mode, dilate)
                assert np.array_equal(got[4:4 + n], want), (name, mode, dilate, int(want.sum()))
                if dilate in (0, 8) or w < 37:
                    assert np.array_equal(renderer.tiles_select(b, a, below=0.02, above=0.98, dilate=dilate), want), (name, mode, dilate)   # the host form
                seen.add((name, int(want.sum()) in (0, n)))
    if n > 4:
        assert ("random", False) in seen and ("equal", False) in seen     # some tiles flagged, not all: the cases tell tiles apart
    assert ("nan", True) in seen and ("exactly equal", True) in seen


# ------------------------------------------------------------------------------------------------ GPU: render_tiles
class _State:
    """One upload per (scene, order) run of rows (tests/test_kernel_matrix.py's pattern), on a context of this module's own."""

    def __init__(self, rt):
        self.rt, self.renderer = rt, rt.Renderer(0)
        self.scenes, self.uploaded = {}, None

    def ensure(self, name, order):
        if name not in self.scenes:
            self.scenes[name] = km.MatrixScene(self.rt, name)
        scene = self.scenes[name]
        if self.uploaded != (name, order):
            self.uploaded = None
            info = km.upload(self.renderer, scene, scene.camera(W, H, 1), order)
            assert info is None or info["exact"], info
            self.uploaded = (name, order)
        return scene


@pytest.fixture(scope="module")
def state(rt):
    s = _State(rt)
    yield s
    s.renderer.close()


# rtk_render_tiles takes no counters: one row per instantiation compiled without them
ROWS = []
for _r in km.ROWS:
    if not _r.count and _r.expect not in {x.expect for x in ROWS}:      # (a few rows are twins: the first of each)
        ROWS.append(_r)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[km.row_id(r) for r in ROWS])
def test_render_tiles_is_the_frame_at_flagged_tiles_and_silence_elsewhere(rt, state, row):
    """Every compiled render-kernel instantiation, both orders and real modes among them: linear bits and rgb8 bytes of
    render_host at the flagged tiles, the sentinel everywhere else, for one to three chunks and five flag patterns."""
    scene = state.ensure(row.scene, row.order)
    real_mode = rt.RTK_REAL_F64 if row.real == km.F64 else rt.RTK_REAL_F32
    r = state.renderer
    assert r.kernel_name(real_mode, row.variant) == km.kernel_name(row.expect)
    patterns = tr.flag_patterns(W, H)
    n = rt.tiles_per_rank(W, H, 1)
    for spp in SPPS:
        cam = scene.camera(W, H, spp)
        full, full8, _ = r.render_host(cam, seed=RENDER_SEED, real_mode=real_mode, variant=row.variant)
        assert np.isfinite(full).all()
        for name, flags in patterns.items():
            *got, info = r.render_tiles(cam, flags, **sentinels(W, H), seed=RENDER_SEED, real_mode=real_mode, variant=row.variant)
            flagged = int((flags != 0).sum())
            assert info == {"flagged": flagged, "rendered": flagged}, (name, spp, info)
            assert_tiles(got, flags, W, H, {"linear": full, "rgb8": full8, "support": np.ones((H, W), np.float32)})
            if name == "all":
                assert np.array_equal(got[0], full) and np.array_equal(got[1], full8)
            if name == "none":
                assert flagged == 0
            assert 0 < int((patterns["random"] != 0).sum()) < n and int(patterns["checker"].sum()) == n // 2


@pytest.mark.gpu
def test_render_tiles_of_a_list_longer_than_one_compaction_round(rt, state):
    """264 x 264: 1 089 tiles, so the compaction's loop runs twice and list positions cross a block of 1 024 tiles' waves."""
    scene = state.ensure("three_spheres", km.REFERENCE)
    w = 264
    cam = scene.camera(w, w, 1)
    flags = tr.flag_patterns(w, w)["checker"]
    assert flags.size == 1089 and flags[1088] == 0 and flags[1087] == 1 and flags[:1024].sum() == 512
    full, full8, _ = state.renderer.render_host(cam, seed=RENDER_SEED)
    *got, info = state.renderer.render_tiles(cam, flags, **sentinels(w, w), seed=RENDER_SEED)
    assert info == {"flagged": 544, "rendered": 544}
    assert_tiles(got, flags, w, w, {"linear": full, "rgb8": full8, "support": np.ones((w, w), np.float32)})
    inverse = (1 - flags).astype(np.int32)                          # ... and the last tile, the one-pixel-wide corner, in the other half
    *got, info = state.renderer.render_tiles(cam, inverse, **sentinels(w, w), seed=RENDER_SEED)
    assert info == {"flagged": 545, "rendered": 545}
    assert_tiles(got, inverse, w, w, {"linear": full, "rgb8": full8})


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("order", [km.REFERENCE, km.FAST])
def test_noise_is_the_one_step_sessions_and_support_is_one(rt, state, real_mode, order):
    scene = state.ensure("cornell_box", order)
    r = state.renderer
    flags = tr.flag_patterns(W, H)["random"]
    m = tr.pixel_mask(flags, W, H)
    for spp in (16, 20, 8):
        cam = scene.camera(W, H, spp)
        p = r.progressive(cam, seed=RENDER_SEED, real_mode=real_mode)
        assert p.chunk_size == 8
        linear, rgb8, noise = p.step(spp)
        p.close()
        *got, _ = r.render_tiles(cam, flags, **sentinels(W, H), seed=RENDER_SEED, real_mode=real_mode)
        assert_tiles(got, flags, W, H, {"linear": linear, "rgb8": rgb8, "noise": noise, "support": np.ones((H, W), np.float32)})
        if spp == 8:
            assert (got[2][m] == 0).all()                           # fewer than two full chunks
        else:
            assert (got[2][m] > 0).sum() >= 16                           # the comparison is not one of zeros


@pytest.mark.gpu
def test_max_tiles_is_decided_on_the_device(rt, state):
    scene = state.ensure("three_spheres", km.REFERENCE)
    r = state.renderer
    cam = scene.camera(W, H, 8)
    flags = tr.flag_patterns(W, H)["checker"]
    flagged = int(flags.sum())
    full, full8, _ = r.render_host(cam, seed=RENDER_SEED)
    *got, info = r.render_tiles(cam, flags, **sentinels(W, H), max_tiles=flagged, seed=RENDER_SEED)
    assert info == {"flagged": flagged, "rendered": flagged}
    assert_tiles(got, flags, W, H, {"linear": full, "rgb8": full8})
    more = flags.copy()
    more[0 if flags[0] == 0 else 1] = 1
    assert int(more.sum()) == flagged + 1
    *got, info = r.render_tiles(cam, more, **sentinels(W, H), max_tiles=flagged, seed=RENDER_SEED)
    assert info == {"flagged": flagged + 1, "rendered": 0}
    assert_tiles(got, np.zeros_like(flags), W, H, {})               # nothing written anywhere
    *got, info = r.render_tiles(cam, more, **sentinels(W, H), max_tiles=0, seed=RENDER_SEED)    # 0: no limit
    assert info == {"flagged": flagged + 1, "rendered": flagged + 1}
    assert_tiles(got, more, W, H, {"linear": full, "rgb8": full8})


@pytest.mark.gpu
def test_the_context_is_left_as_found(rt, state):
    """A tile render between two full frames, and between two steps of a session on the same stream, changes neither."""
    scene = state.ensure("cornell_box", km.FAST)
    r = state.renderer
    cam = scene.camera(W, H, 24)
    flags = tr.flag_patterns(W, H)["random"]
    before = r.render_host(cam, seed=RENDER_SEED)
    again = r.render_host(cam, seed=RENDER_SEED)                     # (the second frame is handed out in the learned order)
    r.render_tiles(cam, flags, seed=RENDER_SEED + 1)
    r.render_tiles(scene.camera(64, 48, 9), tr.flag_patterns(64, 48)["checker"], real_mode=rt.RTK_REAL_F32)   # another shape, mode and camera slot
    after = r.render_host(cam, seed=RENDER_SEED)
    for x, y, z in zip(before[:2], again[:2], after[:2]):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    p = r.progressive(cam, seed=RENDER_SEED)
    p.step(8)
    *got, _ = r.render_tiles(cam, flags, **sentinels(W, H), seed=RENDER_SEED)
    linear, rgb8, _ = p.step(16)
    assert p.samples_done == 24
    p.close()
    assert np.array_equal(linear, before[0]) and np.array_equal(rgb8, before[1])
    assert_tiles(got, flags, W, H, {"linear": before[0], "rgb8": before[1]})


@pytest.fixture(scope="module")
def blocker(rt):
    from tests.test_streams import Blocker

    b = Blocker(rt, rt.Scene.build("book1_final", rt.SCENE_SEED, EARTH))
    yield b
    b.r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
def test_entry_point_forms_agree_on_the_callers_stream_and_carved_buffers(rt, state, blocker, real_mode):
    """Select and render on a caller stream behind a blocker (tests/test_streams.py's pattern), the map made on that stream, every
    buffer carved out of one allocation at an offset that has its element's alignment and no more: the outputs equal the _host
    forms', and an output given as NULL does not change the others."""
    import torch

    from tests.test_streams import _behind_blocker

    scene = state.ensure("cornell_box", km.REFERENCE)
    r = state.renderer
    cam = scene.camera(W, H, 16)
    n = rt.tiles_per_rank(W, H, 1)
    rng = np.random.default_rng(5)
    support = rng.random((H, W)).astype(np.float32)
    want_flags = r.tiles_select(support, below=0.004, dilate=2)
    assert 0 < want_flags.sum() < n and np.array_equal(want_flags, tr.select(support, None, 0.004, 0.0, 2))
    *want, want_info = r.render_tiles(cam, want_flags, **sentinels(W, H), seed=RENDER_SEED, real_mode=real_mode)
    dt, esz = (torch.float64, 8) if real_mode == 0 else (torch.float32, 4)
    names = ("linear", "rgb8", "noise", "support")
    sizes = {"map": H * W * 4, "flags": n * 4, "linear": H * W * 3 * esz, "rgb8": H * W * 3, "noise": H * W * 4, "support": H * W * 4, "info": 8}
    dtypes = {"map": torch.float32, "flags": torch.int32, "linear": dt, "rgb8": torch.uint8, "noise": torch.float32, "support": torch.float32, "info": torch.int32}
    dev_map = torch.from_numpy(support).to("cuda:0").reshape(-1)
    torch.cuda.synchronize()

    def body(streams, keep):
        s = streams[0]
        result = {}
        with torch.cuda.stream(s):
            for skip in (None, 0, 1, 2, 3):
                arena = torch.zeros(sum(sizes.values()) + 16 * len(sizes) + 64, dtype=torch.uint8, device="cuda:0")
                at, piece = 8 if real_mode == 0 else 4, {}                   # never 16-byte aligned
                for key, size in sizes.items():
                    assert at % 16 != 0
                    piece[key] = arena[at:at + size].view(dtypes[key])
                    at += (size + 15) // 16 * 16
                piece["map"].copy_(dev_map)                              # the map is made on the stream
                for key in names:
                    piece[key].fill_(SENTINEL[key])
                piece["flags"].fill_(-77)
                ptr = {k: v.data_ptr() for k, v in piece.items()}
                r.tiles_select_device(W, H, ptr["map"], 0, ptr["flags"], below=0.004, dilate=2, stream=s.cuda_stream)
                outs = [0 if k == skip else ptr[key] for k, key in enumerate(names)]
                r.render_tiles_device(cam, ptr["flags"], *outs, ptr["info"], seed=RENDER_SEED, real_mode=real_mode, stream=s.cuda_stream)
                tag = "nothing" if skip is None else names[skip]
                result.update({"%s without %s" % (key, tag): piece[key] for key in names + ("flags", "info")})   # (views: they keep the arena)
        return result

    got = _behind_blocker("tile lists f%d" % (64 if real_mode == 0 else 32), blocker, 1, body)
    shapes = {"linear": (H, W, 3), "rgb8": (H, W, 3), "noise": (H, W), "support": (H, W)}
    for key, value in got.items():
        name, skipped = key.split(" without ")
        if name == "flags":
            assert np.array_equal(value, want_flags), key
        elif name == "info":
            assert list(value) == [want_info["flagged"], want_info["rendered"]], key
        elif name == skipped:
            assert (value == SENTINEL[name]).all(), key              # the output that was not given: never written
        else:
            assert np.array_equal(value.reshape(shapes[name]).astype(want[names.index(name)].dtype), want[names.index(name)]), key


@pytest.mark.gpu
def test_refusals_launch_and_write_nothing(rt, state):
    import torch

    scene = state.ensure("three_spheres", km.REFERENCE)
    r, lib = state.renderer, rt.hip_lib()
    cam = scene.camera(W, H, 8)
    n = rt.tiles_per_rank(W, H, 1)
    flags = torch.ones(n, dtype=torch.int32, device="cuda:0")
    lin = torch.full((H, W, 3), -7.25, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device="cuda:0")
    noise, support = (torch.full((H, W), v, dtype=torch.float32, device="cuda:0") for v in (-3.0, -5.0))
    info = torch.full((2,), -9, dtype=torch.int32, device="cuda:0")
    outs = [x.data_ptr() for x in (lin, rgb8, noise, support, info)]
    with pytest.raises(rt.RtkError, match="max_tiles"):
        r.render_tiles_device(cam, flags.data_ptr(), *outs, max_tiles=-1)
    with pytest.raises(rt.RtkError, match="no output"):
        r.render_tiles_device(cam, flags.data_ptr(), 0, 0, 0, 0, outs[4])
    with pytest.raises(rt.RtkError, match="d_tile_flags"):
        r.render_tiles_device(cam, 0, *outs)
    with pytest.raises(rt.RtkError, match="d_linear"):
        r.render_tiles_device(cam, flags.data_ptr(), outs[0] + 4, *outs[1:])
    with pytest.raises(rt.RtkError, match="launches"):
        r.render_tiles_device(rt.derive_camera(1920, 16.0 / 9.0, spp=176, max_depth=5), flags.data_ptr(), *outs)
    opts = rt.RenderOpts(RENDER_SEED, 0, 0, 2, 0, 0, None)
    assert lib.rtk_render_tiles(r._ctx, C.byref(cam), C.byref(opts), flags.data_ptr(), 0, *outs) == -1 and "n_ranks" in _err(rt)
    empty = rt.Renderer(0)
    opts = rt.RenderOpts(RENDER_SEED, 0, 0, 1, 0, 0, None)
    assert lib.rtk_render_tiles(empty._ctx, C.byref(cam), C.byref(opts), flags.data_ptr(), 0, *outs) == -5 and "no scene" in _err(rt)   # RTK_ERR_NO_SCENE
    empty.close()
    m = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    with pytest.raises(rt.RtkError, match="dilate"):
        r.tiles_select_device(W, H, m.data_ptr(), 0, flags.data_ptr(), below=0.5, dilate=9)
    with pytest.raises(rt.RtkError, match="both null"):
        r.tiles_select_device(W, H, 0, 0, flags.data_ptr(), below=0.5)
    with pytest.raises(ValueError):
        r.render_tiles(cam, np.ones(n + 1, np.int32))
    torch.cuda.synchronize()
    assert bool((lin == -7.25).all()) and bool((rgb8 == 0xA5).all()) and bool((noise == -3.0).all()) and bool((support == -5.0).all())
    assert bool((info == -9).all()) and bool((flags == 1).all())
    # and the same arguments, accepted; a scene-less context selects
    r.render_tiles_device(cam, flags.data_ptr(), *outs)
    torch.cuda.synchronize()
    assert info.tolist() == [n, n] and bool((support == 1.0).all()) and bool(torch.isfinite(lin).all())
    other = rt.Renderer(0)
    other.tiles_select_device(W, H, m.data_ptr(), 0, flags.data_ptr(), below=0.5)
    torch.cuda.synchronize()
    assert bool((flags == 1).all())                                  # 0 is not >= 0.5: every tile
    other.close()


# ------------------------------------------------------------------------------------------------ GPU: refinement
def _frame(renderer, cam, seed, real_mode=0):
    p = renderer.progressive(cam, seed=seed, real_mode=real_mode)
    linear, _, noise = p.step(cam.samples_per_pixel)
    p.close()
    return linear, noise


REFINE_BELOW, REFINE_DILATE = 0.25, 1


@pytest.mark.gpu
def test_upsample_refined_end_to_end(rt):
    """cornell_box at 64 x 64 from a 32 x 32 frame, fast order: refine_below 0.25 with dilate 1 flags 60 of the 64 tiles (on the
    MI355X; 0.5 flags all 64: the walls' support is about 0.5.  The test asserts only 0 < flagged < 64).  The composition equals the three calls made by hand, plain
    upsampling outside the flagged tiles and the full camera's frame inside them."""
    r = rt.Renderer(0)
    scene = rt.Scene.build("cornell_box", rt.SCENE_SEED, EARTH)
    w, spp = 64, 16
    cam = scene.camera(w, w, spp, 8)
    assert r.upload_fast(scene, cam.center)["exact"]
    low = rt.upsample_camera(cam, 2)
    low_linear, low_noise = _frame(r, low, RENDER_SEED)
    g, low_g = r.guides(cam, 4), r.guides(low, 4)
    plain = r.upsample(cam, low_linear, low_noise, low_g, g)
    out, out_se, rgb8, support, info = r.upsample_refined(cam, low_linear, low_noise, low_g, g, refine_below=REFINE_BELOW, refine_dilate=REFINE_DILATE)
    print("cornell_box 64x64 / 2: refine_below %.2f dilate %d flags %d of %d tiles" % (REFINE_BELOW, REFINE_DILATE, info["flagged"], info["tiles"]))
    assert info["tiles"] == 64 and 0 < info["flagged"] < 64 and info["rendered"] == info["flagged"]
    # by hand
    flags = r.tiles_select(plain[3], below=REFINE_BELOW, dilate=REFINE_DILATE)
    assert np.array_equal(flags, tr.select(plain[3], None, REFINE_BELOW, 0.0, REFINE_DILATE)) and int(flags.sum()) == info["flagged"]
    hand = r.render_tiles(cam, flags, linear=plain[0], rgb8=plain[2], noise=plain[1], support=plain[3])
    for x, y in zip((out, rgb8, out_se, support), hand[:4]):
        assert np.array_equal(x, y)
    m = tr.pixel_mask(flags, w, w)
    full, full8, _ = r.render_host(cam)
    _, full_se = _frame(r, cam, RENDER_SEED)
    for x, y in zip((out, out_se, rgb8, support), plain):
        assert np.array_equal(x[~m], y[~m])
    assert np.array_equal(out[m], full[m]) and np.array_equal(rgb8[m], full8[m]) and np.array_equal(out_se[m], full_se[m]) and (support[m] == 1).all()
    assert not np.array_equal(out[m], plain[0][m])
    # over the share: nothing re-rendered, the upsampled frame as it was
    *over, over_info = r.upsample_refined(cam, low_linear, low_noise, low_g, g, refine_below=REFINE_BELOW, refine_dilate=REFINE_DILATE, max_share=0.01)
    assert over_info["flagged"] == info["flagged"] and over_info["rendered"] == 0
    for x, y in zip(over, plain):
        assert np.array_equal(x, y)
    r.close()


@pytest.mark.gpu
def test_camera_refines_the_upsampled_frame(rt, tmp_path):
    from tests.test_denoise import _read_png

    pkg = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
    exe = str(tmp_path / "refine_camera_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "helpers", "refine_camera_check.cpp"),
                           "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "include"), "-L" + pkg, "-lrtk_hip",
                           "-Wl,-rpath," + pkg, "-o", exe])
    name, w, h, spp, depth = "cornell_box", 64, 64, 16, 8
    done = subprocess.run([exe, str(tmp_path), name, EARTH, str(w), str(h), str(spp), str(depth), str(REFINE_BELOW), str(REFINE_DILATE)], timeout=300,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    v = json.loads(done.stdout.strip().splitlines()[-1])
    assert done.stderr.count("none re-rendered") == 1, done.stderr

    r = rt.Renderer(0)
    scene = rt.Scene.build(name, rt.SCENE_SEED, EARTH)
    cam = scene.camera(w, h, spp, depth)
    if r.upload_fast(scene, cam.center)["exactness"] != 2:          # camera::auto_order: the fast order where it is proven exact
        r.upload(scene)
    low = rt.upsample_camera(cam, 2)
    low_linear, low_noise = _frame(r, low, rt.RENDER_SEED)
    g, low_g = r.guides(cam, 4, seed=rt.RENDER_SEED), r.guides(low, 4, seed=rt.RENDER_SEED)
    plain8 = r.upsample(cam, low_linear, low_noise, low_g, g)[2]
    *_, rgb8, _, info = r.upsample_refined(cam, low_linear, low_noise, low_g, g, refine_below=REFINE_BELOW, refine_dilate=REFINE_DILATE)
    assert v == {"upsampled": [1, 1, 1], "refined": [info["rendered"], 0, 0]} and info["rendered"] > 0, (v, info)
    assert np.array_equal(_read_png(str(tmp_path / "refined.png")), rgb8)
    assert np.array_equal(_read_png(str(tmp_path / "unrefined.png")), plain8)        # refine_support = 0: render_scale's bytes, as before
    assert np.array_equal(_read_png(str(tmp_path / "over.png")), plain8)
    assert not np.array_equal(rgb8, plain8)
    r.close()


# MSE against the 1024-spp frame, cornell_box at 200 x 200 (the setting of tests/test_upsample.py's
# test_real_frames_at_equal_sample_budget: A = 16 spp at full resolution, B = 64 spp at half resolution, upsampled), measured on
# an MI355X ("Tile lists"): "refined/unrefined in tiles" = the MSE over the pixels of the refined tiles, refined frame
# against B; "refined/A" = the whole frame against A; "share" = the tiles refined: the refined frame spends 1 + share times A's
# samples, so against a full-resolution frame of that many samples (MSE ~ 1 / samples) the ratio is refined/A x (1 + share) =
# 0.621, where B/A is 0.472 at equal samples.  refine_below 0.25, dilate 1.  The test allows each measured ratio + 15 %.  A ratio
# above 1 is a finding, not a target; so is this: refinement mends the light's border (below 0.1 the same ratio in tiles is 2.2:
# 16 noisy samples replace a smooth interpolation of 64) but, per sample spent, plain upsampling stays ahead.
REFINE_RATIOS_MEASURED = {"refined/unrefined in tiles": 0.8913, "refined/A": 0.4293, "share": 0.4464}


@pytest.mark.gpu
def test_refinement_quality_at_the_light_border(rt, renderer):
    scene = rt.Scene.build("cornell_box", rt.SCENE_SEED, EARTH)
    renderer.upload(scene)
    w = 200
    camera = lambda spp: scene.camera(w, w, spp, 10)  # noqa: E731
    cam = camera(16)
    low = rt.upsample_camera(camera(64), 2)
    a, _ = _frame(renderer, cam, 31)
    low_linear, low_se = _frame(renderer, low, 32)
    g, low_g = renderer.guides(cam, 4), renderer.guides(low, 4)
    b = renderer.upsample(cam, low_linear, low_se, low_g, g)
    refined, _, _, _, info = renderer.upsample_refined(cam, low_linear, low_se, low_g, g, refine_below=REFINE_BELOW, refine_dilate=REFINE_DILATE, seed=33)
    truth, _, _ = renderer.render_host(camera(1024), seed=1031)
    flags = renderer.tiles_select(b[3], below=REFINE_BELOW, dilate=REFINE_DILATE)
    m = tr.pixel_mask(flags, w, w)
    assert 0 < info["rendered"] == int(flags.sum()) < info["tiles"]
    se2 = lambda img: ((img - truth) ** 2).sum(-1)  # noqa: E731
    ratios = {"refined/unrefined in tiles": float(se2(refined)[m].mean() / se2(b[0])[m].mean()), "refined/A": float(se2(refined).mean() / se2(a).mean()),
              "share": info["rendered"] / info["tiles"]}
    print("cornell_box 200x200, 64 spp at half resolution refined at 16 spp:", json.dumps({"ratios": ratios, "B/A": float(se2(b[0]).mean() / se2(a).mean()),
                                                                                         "tiles": info}))
    assert np.array_equal(refined[~m], b[0][~m])
    for key, measured in REFINE_RATIOS_MEASURED.items():
        assert measured is not None, "the measured ratio %s has not been recorded" % key
        assert ratios[key] <= 1.15 * measured, (key, ratios[key], measured)
