"""Child process of tests/test_scheduler_freedom.py::test_the_cap_is_real (started with RTK_DEBUG=1, so that plan_launch prints
each launch's grid on stderr): three_spheres in the fast order at 37 x 21, 5 spp in chunks of two, rendered once with variant
bits 5-7 = 1 (one wave), once with 3 (four waves) and once without a cap -- three render launches and nothing else."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import raytracingoneweekendapplication_amd as rt  # noqa: E402
from tests import kernel_matrix as km  # noqa: E402


def main():
    renderer = rt.Renderer(0)
    scene = km.MatrixScene(rt, "three_spheres")
    cam = scene.camera(spp=5)
    km.upload(renderer, scene, cam, km.FAST)
    for cap in (1, 3, 0):
        renderer.render_host(cam, variant=(cap << 5) | (2 << 3))
    renderer.close()
    print("rendered 3 frames")


if __name__ == "__main__":
    main()
