"""GPU tests of the lean MIXED kernel on its LDS image (the staged kernel copies a host-built image of the program
whose heads tell their kind in their first 16 bytes).  The image holds the values of the records in memory, so the staged
kernel, the in-memory kernel and the reference order must give the same bytes and the two kernels the same counters, within
the existing cap over the oracle on the same hierarchy."""
import numpy as np
import pytest

from tests.scene_cases import RENDER_SEED, SCENE_SEED
from tests.test_gpu_parity import F64_RMSE_BOUND, _assert_culling_counters, _spheres_of, rmse

pytestmark = pytest.mark.gpu

IN_MEMORY = 1        # variant bit 0: the program stays in memory (rtk_render_kernel<double, 256u, *, false>)
HIT_KEYS = ("samples", "segments", "surface_hits", "rng_draws")


def _render_forms(renderer, cam, count=True):
    return {name: renderer.render_host(cam, count=count, variant=v) for name, v in (("staged", 0), ("memory", IN_MEMORY))}


def test_book1_staged_and_in_memory_kernels_agree_bit_for_bit(rt, orc, renderer):
    scene = rt.Scene.build("book1_final", SCENE_SEED)
    cam = scene.camera(128, 72, 8, 50)
    renderer.upload(scene)
    base, base8, _ = renderer.render_host(cam)
    renderer.upload_fast(scene, cam.center)
    assert "double, 256u, false, true" in renderer.kernel_name() and "double, 256u, false, false" in renderer.kernel_name(variant=IN_MEMORY)
    got = _render_forms(renderer, cam)
    for name, (img, img8, _) in got.items():
        assert np.array_equal(img, base) and np.array_equal(img8, base8), name
    plain, plain8, _ = renderer.render_host(cam)   # the non-counting build
    assert np.array_equal(plain, base) and np.array_equal(plain8, base8)
    fast = scene.fast_order(cam.center)
    _, _, ocnt = orc.render(fast.desc_ptr, cam, RENDER_SEED, 8)
    staged, memory = got["staged"][2], got["memory"][2]
    for key in HIT_KEYS:
        assert staged[key] == ocnt[key], key
    assert staged == memory   # the image holds the values of the records in memory
    _assert_culling_counters(staged, ocnt)


def test_moving_spheres_and_far_camera_on_the_image(rt, orc, renderer):
    """3-unit records in the permuted LDS image, and the exact f64 box test (rays from outside the sized bound) on the
    image's box heads."""
    scene = rt.Scene.build("three_spheres", SCENE_SEED)
    spheres = _spheres_of(scene)
    spheres[1].center_dir[0], spheres[1].center_dir[1] = 0.3, 0.2
    spheres[3].center_dir[2] = -0.25
    cam = scene.camera(96, 54, 8, 10)
    fast = scene.fast_order(cam.center)
    ref, ref8, _ = orc.render(fast.desc_ptr, cam, RENDER_SEED, 4)
    renderer.upload_fast(scene, cam.center)
    for name, (img, img8, _) in _render_forms(renderer, cam, count=False).items():
        assert rmse(img, ref) < F64_RMSE_BOUND and np.array_equal(img8, ref8), name
    far = scene.camera(96, 54, 8, 10)
    for v in (far.center, far.pixel00_loc):
        v.z += 700.0
    ref_far, _, _ = orc.render(fast.desc_ptr, far, RENDER_SEED, 4)
    renderer.upload_fast(scene, None)
    forms = _render_forms(renderer, far, count=False)
    for name, (img, _, _) in forms.items():
        assert np.array_equal(img, forms["staged"][0]) and rmse(img, ref_far) < F64_RMSE_BOUND, name
    assert forms["staged"][0].std() > 0.01


def _poke(scene, edits):
    spheres = _spheres_of(scene)
    for i, (centre, radius) in edits.items():
        for k in range(3):
            spheres[i].center0[k] = centre[k]
        spheres[i].radius = radius


def test_zero_radius_and_tiny_centres(rt, orc, renderer):
    """Zero-width boxes (the margins carry them) and centres at 1e-6."""
    scene = rt.Scene.build("three_spheres", SCENE_SEED)
    _poke(scene, {1: ((1e-6, 1e-6, -1.0 + 1e-6), 0.5), 2: ((-1.0, 0.0, -1.0), 0.0)})
    cam = scene.camera(96, 54, 4, 10)
    fast = scene.fast_order(cam.center)
    ref, ref8, _ = orc.render(fast.desc_ptr, cam, RENDER_SEED, 4)
    renderer.upload_fast(scene, cam.center)
    assert "double, 256u" in renderer.kernel_name()
    for name, (img, img8, _) in _render_forms(renderer, cam, count=False).items():
        assert rmse(img, ref) < F64_RMSE_BOUND and np.array_equal(img8, ref8), name


def test_two_camera_view_batch_on_the_image(rt, renderer):
    scene = rt.Scene.build("book1_final", SCENE_SEED)
    cams = [scene.camera(32, 32, 4, 8), scene.camera(32, 32, 4, 8)]
    for v in (cams[1].center, cams[1].pixel00_loc):
        v.x -= 2.0
        v.y += 0.5
    renderer.upload_fast(scene, cams[0].center)
    singles = [renderer.render_host(c)[0] for c in cams]
    assert "rtk_view_batch_kernel<double, 256u, true>" in renderer.view_kernel_name()
    batch = renderer.render_views(cams)[0]
    for k in range(2):
        assert np.array_equal(np.asarray(batch[k]), singles[k]), k
