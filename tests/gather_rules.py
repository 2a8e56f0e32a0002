"""The conventions of the surface gathers (include/rtk.h "Surface gathers") restated in numpy float64, from the header's text
alone: the cosine-weighted Fibonacci set, each point's rotation of it, the branch-free frame of Duff et al. 2017, the ray records.
Uses nothing of the package but the record's dtype.  numpy evaluates every expression below left to right, as the rule is
written, and fuses nothing."""
import numpy as np

GOLDEN_RATIO_32 = 2654435769
ROTATION_MULTIPLIER = 0x85EBCA6B
TMIN = 0.001


def rotation(first_key, k, rotate):
    """rot_k, exact integers: 0 without rotation, else ((first_key + k) mod 2^32) * 0x85EBCA6B mod 2^32."""
    return ((int(first_key) + int(k)) % 2 ** 32) * ROTATION_MULTIPLIER % 2 ** 32 if rotate else 0


def local_directions(rays, rot=0):
    """(R, 3): (r_j cos phi_j, r_j sin phi_j, z_j)."""
    j = np.arange(rays, dtype=np.uint64)
    u = (2 * j + 1).astype(np.float64) / np.float64(2 * rays)
    r, z = np.sqrt(u), np.sqrt(1.0 - u)
    a = (j * np.uint64(GOLDEN_RATIO_32) + np.uint64(rot)) % np.uint64(2 ** 32)
    phi = a.astype(np.float64) * (2.0 * np.pi * 2.0 ** -32)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def frame(n):
    """(t, bt) of the normal n (3,)."""
    nx, ny, nz = (np.float64(c) for c in n)
    s = np.copysign(1.0, nz)
    a = -1.0 / (s + nz)
    b = nx * ny * a
    return np.array([1.0 + s * nx * nx * a, s * b, -s * nx]), np.array([b, s + ny * ny * a, -ny])


def world_directions(rays, rot, n):
    """(R, 3): d = x t + y bt + z n, summed left to right."""
    local = local_directions(rays, rot)
    t, bt = frame(n)
    n = np.asarray(n, np.float64)
    x, y, z = local[:, 0:1], local[:, 1:2], local[:, 2:3]
    return x * t + y * bt + z * n


def records(dtype, points, normals, *, rays, samples=1, first_key=0, rotate=0, time=0.0, max_distance=0.0):
    """The (n * R,) ray records of rtk_gather_rays, point-major."""
    points, normals = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    out = np.zeros(len(points) * rays, dtype)
    j = np.arange(rays)
    for k in range(len(points)):
        rec = out[k * rays:(k + 1) * rays]
        rec["origin"] = points[k]
        rec["direction"] = world_directions(rays, rotation(first_key, k, rotate), normals[k])
        rec["time"], rec["tmin"], rec["tmax"] = time, TMIN, max_distance if max_distance > 0 else np.inf
        rec["pixel"], rec["sample"] = (first_key + k) % 2 ** 32, (j * samples) % 2 ** 32
    return out
