"""Child process of tests/test_view_batch.py's trace test (run under a kernel trace): on three_spheres in the fast order, one batch
of 70 views of 5 x 3 at 10 spp through the view kernel, then the same batch with the program kept in global memory (variant bit 0:
no view kernel, one plain frame per view) -- and nothing else that launches a render kernel."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import raytracingoneweekendapplication_amd as rt  # noqa: E402
from tests import kernel_matrix as km  # noqa: E402
from tests.test_view_batch import many_views  # noqa: E402


def main():
    renderer = rt.Renderer(0)
    scene = km.MatrixScene(rt, "three_spheres")
    km.upload(renderer, scene, scene.camera(), km.FAST)
    cams, seeds = many_views(rt, scene.camera(5, 3, 10, 6), 70)
    print("view name =", renderer.view_kernel_name(rt.RTK_REAL_F64, 0))
    print("plain name =", renderer.view_kernel_name(rt.RTK_REAL_F64, km.V_GLOBAL))
    renderer.render_views(cams, seeds=seeds)
    renderer.render_views(cams, seeds=seeds, variant=km.V_GLOBAL)
    renderer.close()
    print("rendered two batches of", len(cams))


if __name__ == "__main__":
    main()
