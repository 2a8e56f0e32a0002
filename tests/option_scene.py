"""A scene on which every option the probe bake and the surface gathers read changes the answer (data and functions only; CPU).

The named scenes the device tests of those entry points run on hold nothing that moves, so `time` never reached a comparison.
Here two spheres move across the points and the probes between t = 0 and t = 1, an emitter and a point light make the radiance
depend on where they are, a ceiling over half the sky keeps enough paths alive for the last bounce to count, and -- in the form
with a medium -- a fog ball makes the walk draw from the ray's stream, so that the stream keys matter to occlusion too.  Without
the medium the occlusion gather takes its early-exit instantiation.

`build(medium)` returns the description (tests/desc_builder.py); POINTS / NORMALS are five surface points, PROBES three probe
positions off every surface at t = 0, 0.375 and 1 but for probe 0, which the red sphere swallows around t = 0.4 (on purpose:
inside it the probe sees the sphere's back face and nothing else); `probe_records` restates what rtk_probe_rays writes, as
tests/gather_rules.py `records` restates rtk_gather_rays.  tests/test_entry_options.py states what the scene has to show."""
import math

import numpy as np

from tests.desc_builder import DescBuilder

SEED = 5                          # opts.seed, as in tests/test_light_probes.py and tests/test_surface_gather.py
TIMES = (0.375, 1.0)              # both exact in float: the F32 kernels hold the same value
FIRST_KEY = 2 ** 32 - 2           # point 2 has key 0: the 32-bit wrap is inside every batch
MAX_DEPTH = 6
BACKGROUND = (0.7, 0.8, 1.0)
REACH = 1.5                       # the finite max_distance of the occlusion cases
EYE = (0.0, 1.0, 3.0)             # what the fast order is priced for

GROUND_CENTRE, GROUND_RADIUS = (0.0, -100.5, -1.0), 100.0


def _on_the_ground(dx, dz):
    """(point, normal) of the ground sphere radially above its centre + (dx, ., dz)."""
    n = np.array([dx, math.sqrt(GROUND_RADIUS ** 2 - dx * dx - dz * dz), dz]) / GROUND_RADIUS
    return np.array(GROUND_CENTRE) + GROUND_RADIUS * n, n


_GROUND = [_on_the_ground(dx, 0.0) for dx in (-1.0, 0.0, 1.0)] + [_on_the_ground(-1.8, 2.2)]      # the last: beside the fog ball
POINTS = np.array([_GROUND[0][0], _GROUND[1][0], _GROUND[2][0], (0.0, 0.4, -1.9), _GROUND[3][0]])
NORMALS = np.array([_GROUND[0][1], _GROUND[1][1], _GROUND[2][1], (0.0, 0.0, 1.0), _GROUND[3][1]])
PROBES = np.array([(0.0, 0.6, -1.0), (-1.2, 0.3, -0.2), (0.9, 0.9, -1.8)])


def build(medium):
    b = DescBuilder()
    world = [b.sphere(GROUND_CENTRE, GROUND_RADIUS, b.lambertian((0.6, 0.6, 0.5))),
             b.sphere((-1.0, 0.25, -1.0), 0.5, b.lambertian((0.8, 0.2, 0.2)), motion=(2.0, 0.0, 0.0)),     # crosses the ground points
             b.sphere((0.0, 0.4, -2.6), 0.6, b.dielectric(1.5), motion=(0.0, 0.8, 0.0)),                   # rises behind point 3
             b.sphere((1.6, 0.1, -0.4), 0.45, b.metal((0.8, 0.8, 0.7), 0.1)),
             b.sphere((0.0, 3.0, -1.0), 0.7, b.light((6.0, 5.0, 4.0))),
             # A ceiling over half the sky (47 degrees around the zenith, seen from the ground).  Under an open sky about one path
             # in 300 lives to its sixth segment, and "max_depth one lower" moved one point of five in some cases; under the
             # ceiling every point and probe of every case moves.
             b.sphere((0.0, 15.9, -1.0), 12.0, b.lambertian((0.7, 0.7, 0.7)))]
    b.point_light((2.0, 2.5, 0.5), (3.0, 4.0, 5.0), 0.4)
    if medium:
        # The glass shell is the medium's boundary only, as in single_fog: were it an object of the world as well, every ray that
        # enters the ball would be occluded by the shell whatever the medium draws, and no occlusion count could show a stream key.
        world.append(b.medium(b.sphere((-1.8, 0.2, 0.3), 0.7, b.dielectric(1.5)), 0.8, (0.7, 0.8, 0.9)))
    return b.finish(b.list(world))


def probe_directions(rays):
    """The spherical Fibonacci set of include/rtk.h "Light probes", as tests/test_light_probes.py `directions` has it."""
    j = np.arange(rays, dtype=np.uint64)
    z = 1.0 - (2 * j + 1).astype(np.float64) / np.float64(rays)
    u = (j * np.uint64(2654435769)) % np.uint64(2 ** 32)
    phi = u.astype(np.float64) * (2.0 * np.pi * 2.0 ** -32)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def probe_records(dtype, positions, *, rays, samples=1, first_key=0, time=0.0):
    """The (n * R,) ray records of rtk_probe_rays, probe-major."""
    positions = np.asarray(positions, np.float64)
    out = np.zeros(len(positions) * rays, dtype)
    d, j = probe_directions(rays), np.arange(rays)
    for k in range(len(positions)):
        rec = out[k * rays:(k + 1) * rays]
        rec["origin"], rec["direction"] = positions[k], d
        rec["time"], rec["tmin"], rec["tmax"] = time, 0.001, np.inf
        rec["pixel"], rec["sample"] = (first_key + k) % 2 ** 32, (j * samples) % 2 ** 32
    return out
