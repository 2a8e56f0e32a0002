"""The lens models' sample rule (include/rtk.h "Lens models") restated in numpy float64, using nothing of the package: the stream
of a sample, the three draws, the film coordinates, the three film models, the frame, and the frame a look-at gives.  numpy's
+, -, *, / and sqrt are the IEEE operations the rule is written in; its sin and cos are within one ulp, as the device's are."""
import numpy as np

PERSPECTIVE, EQUIRECT, FISHEYE, ORTHOGRAPHIC = 0, 1, 2, 3
MASK = np.uint64(0xFFFFFFFF)
MUL, INC, PERM = np.uint64(747796405), np.uint64(2891336453), np.uint64(277803737)


def _u32(x):
    return np.asarray(x, np.uint64) & MASK


def pcg_hash(v):
    st = (_u32(v) * MUL + INC) & MASK
    w = (((st >> ((st >> np.uint64(28)) + np.uint64(4))) ^ st) * PERM) & MASK
    return (w >> np.uint64(22)) ^ w


def stream_key(seed, pixel, sample):
    """The state of the stream keyed (seed, pixel, sample)."""
    return pcg_hash((_u32(pixel) + pcg_hash((_u32(sample) + pcg_hash(seed)) & MASK)) & MASK)


def draw(state):
    """(next state, the draw v * 2^-24 as float64)."""
    old = _u32(state)
    w = (((old >> ((old >> np.uint64(28)) + np.uint64(4))) ^ old) * PERM) & MASK
    v = ((w >> np.uint64(22)) ^ w) >> np.uint64(8)
    return (old * MUL + INC) & MASK, v.astype(np.float64) * 2.0 ** -24


def look_at(lookfrom, lookat, vup):
    """(center, u, v, w) of Camera.txt:147-149 with vec3.h's operations in their order."""
    f, a, up = (np.asarray(x, np.float64) for x in (lookfrom, lookat, vup))
    cross = lambda p, q: np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])  # noqa: E731
    unit = lambda p: (1.0 / np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])) * p  # noqa: E731
    w = unit(f - a)
    u = unit(cross(up, w))
    return f, u, cross(w, u), w


def halves(model, fov_h=0.0, fov_v=0.0, ortho_width=0.0, ortho_height=0.0):
    """(fov_h / 2, fov_v / 2) with the defaults resolved, or the halves of the orthographic window."""
    if model == ORTHOGRAPHIC:
        return ortho_width / 2.0, ortho_height / 2.0
    return (fov_h if fov_h != 0.0 else (np.pi if model == FISHEYE else 2.0 * np.pi)) / 2.0, (fov_v if fov_v != 0.0 else np.pi) / 2.0


def film_records(model, width, height, samples, first_sample, seed, center, u, v, w, half_h, half_v, jitter=None):
    """The records of samples first_sample .. + samples - 1 of every pixel, pixel-major, samples inner: a dict of arrays origin
    [n][3], direction [n][3], time, pixel, sample, skip, and the film coordinates x, y.  jitter = (oy, ox) overrides the draws."""
    center, u, v, w = (np.asarray(a, np.float64) for a in (center, u, v, w))
    pixel = np.repeat(np.arange(width * height, dtype=np.uint64), samples)
    sample = np.tile(np.arange(samples, dtype=np.uint64), width * height) + np.uint64(first_sample)
    i, j = (pixel % np.uint64(width)).astype(np.float64), (pixel // np.uint64(width)).astype(np.float64)
    state = stream_key(seed, pixel, sample)
    state, oy = draw(state)
    state, ox = draw(state)
    state, time = draw(state)
    oy, ox = oy - 0.5, ox - 0.5
    if jitter is not None:
        oy, ox = np.full_like(oy, jitter[0]), np.full_like(ox, jitter[1])
    x = 2.0 * ((i + ox) + 0.5) / np.float64(width) - 1.0
    y = 1.0 - 2.0 * ((j + oy) + 0.5) / np.float64(height)
    n = len(pixel)
    lx, ly, lz = np.zeros(n), np.zeros(n), -np.ones(n)
    origin = np.tile(center, (n, 1))
    if model == EQUIRECT:
        lon, lat = x * half_h, y * half_v
        c = np.cos(lat)
        lx, ly, lz = c * np.sin(lon), np.sin(lat), -(c * np.cos(lon))
    elif model == FISHEYE:
        yy = y * (np.float64(height) / np.float64(width))
        r = np.sqrt(x * x + yy * yy)
        theta = r * half_h
        ok = r != 0.0
        rs = np.where(ok, r, 1.0)
        lx = np.where(ok, np.sin(theta) * (x / rs), 0.0)
        ly = np.where(ok, np.sin(theta) * (yy / rs), 0.0)
        lz = np.where(ok, -np.cos(theta), -1.0)
    else:
        ax, ay = x * half_h, y * half_v
        origin = (center[None, :] + ax[:, None] * u[None, :]) + ay[:, None] * v[None, :]
    direction = (lx[:, None] * u[None, :] + ly[:, None] * v[None, :]) + lz[:, None] * w[None, :]
    return {"origin": origin, "direction": direction, "time": time, "pixel": pixel.astype(np.uint32), "sample": sample.astype(np.uint32),
            "skip": np.full(n, 3, np.uint32), "x": x, "y": y, "local": np.stack([lx, ly, lz], 1)}


def standard_error(radiance):
    """se [pixels] of radiance [pixels][S][3] (float64 values): the header's estimate over samples, in double, in sample order."""
    s = radiance.shape[1]
    if s < 2:
        return np.zeros(radiance.shape[0])
    s1, s2 = np.zeros(radiance.shape[0]), np.zeros(radiance.shape[0])
    for k in range(s):
        y = ((radiance[:, k, 0] + radiance[:, k, 1]) + radiance[:, k, 2]) / 3.0
        s1 = s1 + y
        s2 = s2 + y * y
    m = s1 / s
    return np.sqrt(np.maximum((s2 - s * m * m) / (s - 1), 0.0) / s)
