"""GPU tests (-m gpu) over tests/kernel_matrix.py: every rtk_render_kernel instantiation that kernel_choice::choose can select is
launched by the row that selects it and checked there --

  every row      rtk_kernel_name's answer is the row's name, character for character (COUNT = false rows: the entry point
                 always asks with count = false)
  f64 rows       against the CPU oracle executing the same hierarchy (RMSE < F64_RMSE_BOUND, equal bytes) and bit-identical to
                 the scene's reference-order default render (every fast order here reports `exact`); COUNT rows: counters equal to
                 the oracle's on the slot program, within _assert_culling_counters' slack on a MIXED / COMPACT program
  f32 rows       bit-identical to the f32 render of the same scene and order at variant 0: the variant bits and count_work move
                 data (LDS or memory) or add counters, never an operation, and -ffp-contract=off holds everywhere.  The f32
                 COUNT rows are on material_zoo, whose non-counting kernel is the full-feature template as well.
                 Coherence with the f64 kernel at 1 spp for the (scene, order) pairs tests/test_f32_parity.py does not run.
  the trace      one child process renders every row under `rocprofv3 --kernel-trace`; the set of dispatched
                 rtk::rtk_render_kernel<...> names must be the set the rows expect -- what confirms that the launch of the
                 table row (launch_chosen) reaches the device under the printed name, and the COUNT rows.
"""
import os
import shutil
import signal
import subprocess
import sys

import numpy as np
import pytest

from tests import kernel_matrix as km
from tests.conftest import ROOT
from tests.scene_cases import RENDER_SEED
from tests.test_f32_parity import COHERENT_P99, coherence
from tests.test_gpu_parity import F64_RMSE_BOUND, _assert_culling_counters, rmse

pytestmark = pytest.mark.gpu


class _State:
    """One upload per (scene, order) run of rows, one oracle render per (scene, hierarchy), one reference-order render per scene."""

    def __init__(self, rt, orc, renderer):
        self.rt, self.orc, self.renderer = rt, orc, renderer
        self.scenes, self.uploaded, self.info = {}, None, {}
        self.oracle_renders, self.reference_renders, self.f32_renders = {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = km.MatrixScene(self.rt, name)
        return self.scenes[name]

    def ensure(self, name, order):
        scene = self.scene(name)
        cam = scene.camera()
        if self.uploaded != (name, order):
            self.uploaded = None
            self.info[name, order] = km.upload(self.renderer, scene, cam, order)
            self.uploaded = (name, order)
        return scene, cam

    def oracle(self, name, order):
        if (name, order) not in self.oracle_renders:
            scene = self.scene(name)
            cam = scene.camera()
            what = scene.fast_order(cam.center) if order == km.FAST else scene
            self.oracle_renders[name, order] = self.orc.render(what.desc_ptr, cam, RENDER_SEED, 8)
        return self.oracle_renders[name, order]

    def reference_render(self, name):
        if name not in self.reference_renders:
            _, cam = self.ensure(name, km.REFERENCE)
            self.reference_renders[name] = self.renderer.render_host(cam, seed=RENDER_SEED, real_mode=self.rt.RTK_REAL_F64)[:2]
        return self.reference_renders[name]

    def f32_render(self, name, order):
        if (name, order) not in self.f32_renders:
            _, cam = self.ensure(name, order)
            self.f32_renders[name, order] = self.renderer.render_host(cam, seed=RENDER_SEED, real_mode=self.rt.RTK_REAL_F32)[:2]
        return self.f32_renders[name, order]


@pytest.fixture(scope="module")
def state(rt, orc):
    renderer = rt.Renderer(0)     # its own context: the uploads cached here must not depend on what other modules upload
    yield _State(rt, orc, renderer)
    renderer.close()


@pytest.mark.parametrize("row", km.ROWS, ids=[km.row_id(r) for r in km.ROWS])
def test_row_selects_its_kernel_and_renders_the_reference_image(rt, state, row):
    real_mode = rt.RTK_REAL_F64 if row.real == km.F64 else rt.RTK_REAL_F32
    base, base8 = state.reference_render(row.scene) if row.real == km.F64 else (None, None)
    _, cam = state.ensure(row.scene, row.order)
    info = state.info[row.scene, row.order]
    assert info is None or info["exact"], info
    if not row.count:
        assert state.renderer.kernel_name(real_mode, row.variant) == km.kernel_name(row.expect)
    img, img8, counters = state.renderer.render_host(cam, seed=RENDER_SEED, real_mode=real_mode, count=row.count, variant=row.variant)
    if row.real == km.F32:
        want, want8 = state.f32_render(row.scene, row.order)
        assert np.isfinite(img).all() and np.array_equal(img, want) and np.array_equal(img8, want8)
        assert not row.count or counters["samples"] == km.WIDTH * km.HEIGHT * km.SPP
        return
    ref, ref8, ocnt = state.oracle(row.scene, row.order)
    assert rmse(img, ref) < F64_RMSE_BOUND and np.array_equal(img8, ref8)
    assert np.array_equal(img, base) and np.array_equal(img8, base8)
    if row.count:
        if row.expect[1] & 256:    # F_F32_BOX: conservative culling boxes
            _assert_culling_counters(counters, ocnt, slack=km.CULLING_SLACK[row.scene])
        else:
            assert counters == ocnt


CUSTOM_F32 = sorted({(r.scene, r.order) for r in km.ROWS if r.real == km.F32 and r.scene in km.CUSTOM_SCENES})


@pytest.mark.parametrize("name,order", CUSTOM_F32, ids=[f"{n}-{o}" for n, o in CUSTOM_F32])
def test_f32_sample_coherence_of_the_scenes_built_here(rt, state, name, order):
    """tests/test_f32_parity.py::test_f32_sample_coherence_with_f64 for the (scene, order) pairs it does not run."""
    state.uploaded = None
    case = (name, km.WIDTH, km.HEIGHT, 1, km.SCENE_DEPTH[name])
    r = coherence(rt, state.renderer, state.scene(name), case, order)
    print(name, order, r)
    assert r["incoherent_frac"] <= km.MATRIX_INCOHERENT[name][2], r
    assert r["coherent_p99"] <= COHERENT_P99, r


# One run of the child on the MI355X under rocprofv3 took TRACE_RUN_SECONDS (process start with the torch import, 10 scene
# builds, 19 uploads, 65 renders at 8 x 8, the profiler's own start and its CSV output); the time limit is three times that, 9.51 s.
TRACE_RUN_SECONDS = 3.17
TRACE_TIMEOUT = 3 * TRACE_RUN_SECONDS


def test_every_row_dispatches_the_kernel_it_names(tmp_path):
    """The names in a kernel trace of one process that renders every row == the names the rows expect: rtk_kernel_name prints
    kernel_choice::choose's result and launch_chosen launches the table row with that tuple (tests/test_kernel_choice.py, CPU) -- here the
    launch is seen to reach the device under that name, COUNT rows included."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        pytest.skip("rocprofv3 not present")
    child = os.path.join(ROOT, "tests", "helpers", "kernel_matrix_child.py")
    cmd = [rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path), "--", sys.executable, child]
    # subprocess.run's timeout, with the child in a session of its own so that a late one is killed whole (profiler and program)
    with subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True) as proc:
        try:
            stdout, _ = proc.communicate(timeout=TRACE_TIMEOUT)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.communicate()
            pytest.fail(f"the traced child did not finish within {TRACE_TIMEOUT} s")
    done = subprocess.CompletedProcess(cmd, proc.returncode, stdout)
    assert done.returncode == 0, done.stdout[-4000:]
    ran, n_files = km.dispatched_instantiations(tmp_path)
    assert n_files == 1, (n_files, done.stdout[-2000:])
    expected = {r.expect for r in km.ROWS}
    assert not ran & set(km.UNREACHABLE), sorted(ran & set(km.UNREACHABLE))
    assert ran == expected, {"not dispatched": sorted(expected - ran), "dispatched, in no row": sorted(ran - expected)}
