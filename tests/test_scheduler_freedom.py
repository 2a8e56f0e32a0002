"""GPU tests (-m gpu) of the render kernels' promise that WHICH LANE RENDERS A PIXEL, AND WHEN, NEVER CHANGES ITS VALUE
(csrc/rtk_render_body.inc: the item prefetch, the two-round hand_out, the refill inside the shade step, the per-lane
my_slot / my_view / s_end, the box loop with its ride-alongs and exit thresholds, the vote).

plan_launch gives a small frame one wave per work item, so in every other small test a wave's first hand_out serves all 64
lanes and nothing of the above runs -- unless a wave that starts before the others happens to draw a second item.  Here
variant bits 5-7 (the grid cap, host only: rtk_grid_plan.h) hold the launch to 1, 2 or 4 waves, and the frame -- the matrix's 37 x 21 (15 ragged tiles) at 5 spp in chunks of two samples (2, 2, 1: 45 work items, the
last chunk shorter) -- makes every wave take at least eight items one after the other: lanes refill inside the shade step, the
second hand_out round runs, one wave holds lanes of two items (chunks, tiles, views), and a lane inherits s_end and my_slot
from another chunk.  Every test asserts n_items >= 8 x waves from the camera, so none can fall back to one item per wave.

  a  every row of tests/kernel_matrix.py (65 rows, all 61 instantiations) uncapped and at 1, 2, 4 waves: the same bits; f64 rows at one
     wave against the oracle as test_kernel_matrix.py holds the uncapped frame; COUNT rows: the twelve counters equal;
  b  every row at 2 waves under each scheduler knob (variant bits 8-19) one at a time and three combined words: the same bits;
  c  four ranks at one wave each (rank 3's last local tile does not exist: an it_ok == false item between real ones);
  d  the hand-out order: none, learned, fixed -- the same frame;
  e  a view batch (lanes of two views in one wave) and a tile list at 1 and 2 waves;
  f  the cap is real: the grids a child process prints under RTK_DEBUG.

The partial-sum workspace is reused between renders, so a (pixel, chunk) that a kernel skips would keep the previous render's
value -- the right one, if that was the same frame.  `fresh` therefore renders the same camera and variant with ANOTHER seed
before every compared render.

MUTANTS is the record of what these tests see (each mutation made by hand in a scratch copy of csrc/rtk_render_body.inc, the
library built and this file run once on the MI355X; the unmutated library passes all of it); UNREACHED, what they cannot see.

The whole file on the MI355X: 140 tests in 11.9 s (FILE_SECONDS below); the slowest case is the child process of f, 2.1 .. 2.7 s, the
slowest render case (31 knob words x 2 renders of book2_final) 0.4 s.
"""
import os
import re
import signal
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_matrix as km
from tests.conftest import ROOT
from tests.scene_cases import RENDER_SEED
from tests.test_gpu_parity import F64_RMSE_BOUND, _assert_culling_counters, rmse
from tests.test_kernel_matrix import _State
from tests.test_view_batch import VIEW_TUPLES, five_views, view_kernel_name

pytestmark = pytest.mark.gpu

FILE_SECONDS = 11.9          # measured duration of `pytest tests/test_scheduler_freedom.py -m gpu`: 140 passed

SPP = 5
CHUNKS_OF_2 = 2 << 3         # variant bits 3-4 = 2: chunks of two samples
FIXED_ORDER = 4              # variant bit 2
OTHER_SEED = RENDER_SEED ^ 0x2545F491


def cap(waves):
    """variant bits 5-7 = k: at most 2^(k-1) waves in the launch."""
    k = {1: 1, 2: 2, 4: 3, 8: 4, 16: 5, 32: 6, 64: 7}[waves]
    return k << 5


def n_items(cam, n_ranks=1, n_views=1, n_tiles=None):
    """tiles x chunks of a launch for `cam` at CHUNKS_OF_2, from the camera alone."""
    tiles = -(-cam.image_width // 8) * -(-cam.image_height // 8)
    local = -(-tiles // n_ranks) * n_views if n_tiles is None else n_tiles
    return local * -(-cam.samples_per_pixel // 2)


def assert_many_items_per_wave(cam, waves, **kw):
    assert n_items(cam, **kw) >= 8 * waves, (n_items(cam, **kw), waves)


# What the tests see.  Every mutation leaves all addresses, program counters and loop exits as they are.  "kernel matrix green":
# tests/test_kernel_matrix.py (the earlier suite's small tests of the same kernels) on the mutated library.
# km.ROWS has 65 rows for the 61 instantiations; a and b have one case per row.  The five rows that stay green under S1, S2, S3
# and S6 are the kernels compiled without the refill in the shade step (kRefillInShade false: the glossy quad/box family, FEAT 69
# in f64 and f32 and 325), where the mutated lines are dead code.
MUTANTS = {
    "S1 refill in shade does not clear L.sum for the new pixel":
        "a 60 / 65, b 60 / 65, c 3 / 3, d 2 / 2, e views 2 / 2 and tiles 2 / 2.  Kernel matrix NOT green: 10 of 68 red in that run (material_zoo "
        "f64, one mesh_metal_large f32 row) -- a wave that starts early can draw a second item before the others start, so those "
        "tests see it when the timing falls that way",
    "S2 refill in shade keeps the previous s_end":
        "a 60 / 65, b 60 / 65, c 3 / 3, d 2 / 2, e views 2 / 2 and tiles 2 / 2 (the last chunk has one sample, the others two).  Kernel matrix "
        "green, 68 passed: its frames have one chunk, every s_end is the same",
    "S3 refill in shade keeps the previous my_slot":
        "a 60 / 65, b 60 / 65, c 3 / 3, d 2 / 2, e views 2 / 2 and tiles 2 / 2.  Kernel matrix NOT green: the same 10 of 68 as S1, for the same reason",
    "S4 the second hand_out round is given the first round's idle mask":
        "a 38 / 65, b 59 / 65, d 1 / 2 (material_zoo COLD).  A second round needs idle lanes while the item still has pixels -- here the "
        "lanes that drew a pixel outside the ragged frame -- so what a row sees depends on its knobs and timing; c and e stayed "
        "green.  Kernel matrix green, 68 passed",
    "S5 (view kernel) refill in shade does not update my_view":
        "e views 2 / 2, nothing else (no other test runs a view kernel).  Kernel matrix green, 68 passed",
    "S6 refill in shade starts at sample 0 instead of it_s_begin":
        "a 60 / 65, b 60 / 65, c 3 / 3, d 2 / 2, e views 2 / 2 and tiles 2 / 2.  Kernel matrix green, 68 passed: one chunk, it_s_begin is 0",
}
UNREACHED = {
    "a dropped fetch(), other refill_next arithmetic, rec_at":
        "not built: such a mutation can run a pc off the program, and a fault may not be provoked",
}


class State(_State):
    """test_kernel_matrix's per-(scene, order) state at this file's frame: one upload per run of rows, one oracle render per
    (scene, hierarchy), one reference-order render per scene."""

    def camera(self, name, **kw):
        return self.scene(name).camera(spp=SPP, **kw)

    def ensure(self, name, order):
        scene, _ = super().ensure(name, order)     # (uploads with the scene's own camera as the fast order's eye)
        return scene, self.camera(name)

    def oracle(self, name, order):
        if (name, order) not in self.oracle_renders:
            scene = self.scene(name)
            what = scene.fast_order(scene.camera().center) if order == km.FAST else scene
            self.oracle_renders[name, order] = self.orc.render(what.desc_ptr, self.camera(name), RENDER_SEED, 8)
        return self.oracle_renders[name, order]

    def reference_render(self, name):
        if name not in self.reference_renders:
            _, cam = self.ensure(name, km.REFERENCE)
            self.reference_renders[name] = fresh(self.renderer, cam, self.rt.RTK_REAL_F64, CHUNKS_OF_2)[:2]
        return self.reference_renders[name]


@pytest.fixture(scope="module")
def state(rt, orc):
    renderer = rt.Renderer(0)
    yield State(rt, orc, renderer)
    renderer.close()


@pytest.fixture(scope="module", params=km.ROWS, ids=[km.row_id(r) for r in km.ROWS])
def row(request):
    """Module-scoped, so that the tests of one row run together and share its upload."""
    return request.param


def fresh(renderer, cam, real_mode, variant, count=False, stale_variant=None):
    """render_host(cam) at `variant` after a render of the same camera and variant (`stale_variant`: d's one exception) with
    another seed in the same context: whatever the compared render does not write holds another frame's sums."""
    renderer.render_host(cam, seed=OTHER_SEED, real_mode=real_mode, count=count, variant=variant if stale_variant is None else stale_variant)
    return renderer.render_host(cam, seed=RENDER_SEED, real_mode=real_mode, count=count, variant=variant)


def _mode(rt, real):
    return rt.RTK_REAL_F64 if real == km.F64 else rt.RTK_REAL_F32


def assert_same_frame(got, want, what):
    assert np.isfinite(got[0]).all(), what
    assert np.array_equal(got[0], want[0]), (what, int((got[0] != want[0]).any(axis=2).sum()), "pixels differ")
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], (what, got[2], want[2])      # the twelve work counters of a COUNT row (None otherwise)


# ------------------------------------------------------------------------------------------------ a
def test_every_instantiation_crosses_item_boundaries(rt, state, row):
    real_mode = _mode(rt, row.real)
    variant = row.variant | CHUNKS_OF_2
    base = state.reference_render(row.scene) if row.real == km.F64 else None
    _, cam = state.ensure(row.scene, row.order)
    info = state.info[row.scene, row.order]
    assert info is None or info["exact"], info
    assert_many_items_per_wave(cam, 4)
    name = state.renderer.kernel_name(real_mode, variant)
    assert row.count or name == km.kernel_name(row.expect)
    uncapped = fresh(state.renderer, cam, real_mode, variant, row.count)
    frames = {}
    for waves in (1, 2, 4):
        assert state.renderer.kernel_name(real_mode, variant | cap(waves)) == name
        frames[waves] = fresh(state.renderer, cam, real_mode, variant | cap(waves), row.count)
        assert_same_frame(frames[waves], uncapped, f"{waves} wave(s) against the uncapped grid")
    img, img8, counters = frames[1]
    if row.count:
        assert counters["samples"] == cam.image_width * cam.image_height * SPP      # every (pixel, sample) exactly once
    if row.real == km.F32:
        return
    ref, ref8, ocnt = state.oracle(row.scene, row.order)
    assert rmse(img, ref) < F64_RMSE_BOUND and np.array_equal(img8, ref8)
    assert np.array_equal(img, base[0]) and np.array_equal(img8, base[1])
    if row.count:
        if row.expect[1] & 256:    # F_F32_BOX: conservative culling boxes
            _assert_culling_counters(counters, ocnt, slack=km.CULLING_SLACK[row.scene])
        else:
            assert counters == ocnt


# ------------------------------------------------------------------------------------------------ b
# The four scheduler fields of the variant word (rtk_render_body.inc), 0 = the kernel family's default:
#   bits  8-10  box-loop exit threshold in eighths of the starters            1 .. 7
#   bits 11-13  sphere-loop exit threshold in eighths of the starters         1 .. 7
#   bits 14-16  refill batch size, kRefillMinTable = {4, 1, 4, 8, 16, 24, 32, 12}
#   bits 17-19  lanes for a ride-along sphere step, kSphereMinTable = {16, 65 (never), 4, 8, 12, 16, 24, 32}
BOX, SPHERE, REFILL, RIDE = 8, 11, 14, 17
KNOB_WORDS = [(v << shift) for shift in (BOX, SPHERE, REFILL, RIDE) for v in range(1, 8)] + [
    (1 << REFILL) | (1 << RIDE) | (7 << BOX) | (7 << SPHERE),      # refill 1, ride-along never, both thresholds 7/8
    (6 << REFILL) | (2 << RIDE) | (1 << BOX) | (1 << SPHERE),      # refill 32, ride-along at 4 lanes, both thresholds 1/8
    (7 << REFILL) | (7 << RIDE) | (7 << BOX) | (7 << SPHERE),      # every field at 7
]
assert len(KNOB_WORDS) == 31 and len(set(KNOB_WORDS)) == 31


def test_every_scheduler_knob_renders_the_same_frame(rt, state, row):
    real_mode = _mode(rt, row.real)
    variant = row.variant | CHUNKS_OF_2 | cap(2)
    _, cam = state.ensure(row.scene, row.order)
    assert_many_items_per_wave(cam, 2)
    name = state.renderer.kernel_name(real_mode, variant)
    want = fresh(state.renderer, cam, real_mode, variant, row.count)
    for word in KNOB_WORDS:
        assert state.renderer.kernel_name(real_mode, variant | word) == name
        assert_same_frame(fresh(state.renderer, cam, real_mode, variant | word, row.count), want, f"knob word {word:#x}")


# ------------------------------------------------------------------------------------------------ c
RANK_CASES = [("three_spheres", km.FAST, km.F64), ("cornell_box", km.FAST, km.F64), ("material_zoo", km.REFERENCE, km.F32)]


@pytest.mark.parametrize("name,order,real", RANK_CASES, ids=[f"{n}-{o}-{r}" for n, o, r in RANK_CASES])
def test_four_ranks_of_one_wave_each(rt, state, name, order, real):
    """15 tiles on four ranks: four local tiles each, and rank 3's last one is tile 15, which does not exist -- its three chunks
    are work items that give their lanes nothing, handed out between real ones."""
    import torch
    from raytracingoneweekendapplication_amd import tiling

    n_ranks = 4
    real_mode, dtype = _mode(rt, real), (torch.float64 if real == km.F64 else torch.float32)
    _, cam = state.ensure(name, order)
    w, h = cam.image_width, cam.image_height
    tpr = tiling.tiles_per_rank(w, h, n_ranks)
    assert tpr == 4 and 3 + n_ranks * (tpr - 1) == 15 == -(-w // 8) * -(-h // 8)
    assert_many_items_per_wave(cam, 1, n_ranks=n_ranks)
    whole, whole8, _ = fresh(state.renderer, cam, real_mode, CHUNKS_OF_2)
    dev = torch.device("cuda", 0)
    variant = CHUNKS_OF_2 | cap(1)
    parts = []
    for rank in range(n_ranks):
        buf = torch.full((tpr, 3, 64), float("nan"), dtype=dtype, device=dev)
        for seed in (OTHER_SEED, RENDER_SEED):      # (`fresh` for a rank)
            state.renderer.render_device(cam, buf.data_ptr(), 0, seed=seed, real_mode=real_mode, rank=rank, n_ranks=n_ranks, variant=variant)
        parts.append(buf)
    gathered = torch.stack(parts).contiguous()
    image = torch.empty((h, w, 3), dtype=dtype, device=dev)
    rgb8 = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    state.renderer.unpermute(w, h, n_ranks, real_mode, gathered.data_ptr(), image.data_ptr(), rgb8.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy().astype(np.float64), whole)
    assert np.array_equal(rgb8.cpu().numpy(), whole8)


# ------------------------------------------------------------------------------------------------ d
ORDER_CASES = [("three_spheres", 0, 256, True), ("material_zoo", km.V_COLD, 383 | 1024, False)]


@pytest.mark.parametrize("name,bits,feat,in_lds", ORDER_CASES, ids=["lean-staged", "material_zoo-cold"])
def test_hand_out_order_none_learned_and_fixed(rt, state, name, bits, feat, in_lds):
    """One wave takes the 45 items in row-major order (no order yet), in the order learned from that frame (the tile_order table
    in LDS where the plan finds room, in memory otherwise), and in row-major order again (bit 2): one frame, the uncapped one."""
    real_mode = rt.RTK_REAL_F64
    _, cam = state.ensure(name, km.FAST)
    assert_many_items_per_wave(cam, 1)
    variant = bits | CHUNKS_OF_2
    assert state.renderer.kernel_name(real_mode, variant | cap(1)) == km.kernel_name((km.F64, feat, False, in_lds))
    want = fresh(state.renderer, cam, real_mode, variant)
    v1 = variant | cap(1)
    # the stale frame, then a frame of another shape: the context forgets the order it learned
    state.renderer.render_host(cam, seed=OTHER_SEED, real_mode=real_mode, variant=v1)
    state.renderer.render_host(state.camera(name, width=8, height=8), real_mode=real_mode, variant=v1)
    first = state.renderer.render_host(cam, seed=RENDER_SEED, real_mode=real_mode, variant=v1)
    assert_same_frame(first, want, "no order yet")
    # the stale frame in fixed order neither reads nor replaces what the first frame taught
    second = fresh(state.renderer, cam, real_mode, v1, stale_variant=v1 | FIXED_ORDER)
    assert_same_frame(second, want, "learned order")
    assert_same_frame(fresh(state.renderer, cam, real_mode, v1 | FIXED_ORDER), want, "fixed order")


# ------------------------------------------------------------------------------------------------ e
VIEW_CASES = [("three_spheres", (km.F64, 256, True)), ("cornell_box", (km.F64, 837, True))]


@pytest.mark.parametrize("name,expect", VIEW_CASES, ids=["mixed-staged", "compact-quadbox"])
def test_a_view_batch_on_one_and_two_waves(rt, state, name, expect):
    """Five unlike 16 x 16 views: 20 tiles x 3 chunks on one or two waves -- lanes of two views side by side in a wave, a lane
    inheriting another view's record offset."""
    real_mode = rt.RTK_REAL_F64
    state.ensure(name, km.FAST)
    cam = state.camera(name, width=16, height=16)
    cams, seeds = five_views(rt, cam)
    assert expect in VIEW_TUPLES
    want = [state.renderer.render_host(c, seed=s, real_mode=real_mode, variant=CHUNKS_OF_2)[:2] for c, s in zip(cams, seeds)]
    for waves in (1, 2):
        assert_many_items_per_wave(cam, waves, n_views=len(cams))
        variant = CHUNKS_OF_2 | cap(waves)
        assert state.renderer.view_kernel_name(real_mode, variant) == view_kernel_name(expect)
        state.renderer.render_views(cams, seeds=[s ^ 0x9E3779B9 for s in seeds], real_mode=real_mode, variant=variant)      # (`fresh` for a batch)
        linear, rgb8, _ = state.renderer.render_views(cams, seeds=seeds, real_mode=real_mode, variant=variant)
        for v in range(len(cams)):
            assert np.array_equal(linear[v], want[v][0]) and np.array_equal(rgb8[v], want[v][1]), (waves, v)
    assert not np.array_equal(want[0][0], want[4][0])


@pytest.mark.parametrize("name", ["three_spheres", "cornell_box"])
def test_a_checkerboard_tile_list_on_one_wave(rt, state, name):
    """Eight of the fifteen tiles, flagged like a checkerboard, x 3 chunks on one wave: the flagged tiles carry the frame's own
    bits, every other pixel keeps what it held."""
    real_mode = rt.RTK_REAL_F64
    _, cam = state.ensure(name, km.FAST)
    w, h = cam.image_width, cam.image_height
    tx, ty = -(-w // 8), -(-h // 8)
    flags = np.array([(x + y) % 2 == 0 for y in range(ty) for x in range(tx)], np.int32)
    assert_many_items_per_wave(cam, 1, n_tiles=int(flags.sum()))
    want, want8, _ = fresh(state.renderer, cam, real_mode, CHUNKS_OF_2)
    variant = CHUNKS_OF_2 | cap(1)
    init, init8 = np.full((h, w, 3), -7.25), np.full((h, w, 3), 77, np.uint8)
    state.renderer.render_tiles(cam, flags, linear=init, rgb8=init8, seed=OTHER_SEED, real_mode=real_mode, variant=variant)      # (`fresh` for a list)
    linear, rgb8, _, _, info = state.renderer.render_tiles(cam, flags, linear=init, rgb8=init8, real_mode=real_mode, variant=variant)
    assert info == {"flagged": int(flags.sum()), "rendered": int(flags.sum())}
    mask = np.kron(flags.reshape(ty, tx), np.ones((8, 8), np.int32))[:h, :w].astype(bool)
    assert np.array_equal(linear[mask], want[mask]) and np.array_equal(rgb8[mask], want8[mask])
    assert np.array_equal(linear[~mask], init[~mask]) and np.array_equal(rgb8[~mask], init8[~mask])


# ------------------------------------------------------------------------------------------------ f
# One run of the child on the MI355X took CAP_RUN_SECONDS (process start with the library load, one scene build, one upload,
# three renders at 37 x 21: 2.08 s after this file alone, 2.72 s at the end of the whole suite -- the larger); the time limit is
# three times that.
CAP_RUN_SECONDS = 2.72
CAP_TIMEOUT = 3 * CAP_RUN_SECONDS


def test_the_cap_is_real():
    """The grids plan_launch prints (RTK_DEBUG) for a frame at cap 1, at cap 3 and uncapped: 1 wave, 4 waves, more than 4."""
    child = os.path.join(ROOT, "tests", "helpers", "grid_cap_child.py")
    env = dict(os.environ, RTK_DEBUG="1")
    t0 = time.monotonic()
    with subprocess.Popen([sys.executable, child], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True) as proc:
        try:
            stdout, stderr = proc.communicate(timeout=CAP_TIMEOUT)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.communicate()
            pytest.fail(f"the child did not finish within {CAP_TIMEOUT} s")
    print(f"grid_cap_child.py: {time.monotonic() - t0:.2f} s")
    assert proc.returncode == 0, (stdout[-2000:], stderr[-2000:])
    grids = [(int(b), int(t)) for b, t in re.findall(r"launch plan: .* grid (\d+) x (\d+) threads", stderr)]
    assert len(grids) == 3, stderr[-4000:]
    waves = [b * t // 64 for b, t in grids]
    assert all(t % 64 == 0 for _, t in grids) and waves[0] == 1 and waves[1] == 4 and waves[2] > 4, grids
