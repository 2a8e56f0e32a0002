"""The float culling tests of the fast order's render kernels on rays that are AIMED: every primary ray of a camera meets a
primitive of its own at a corner, an edge, a seam or inside a 1e-4 thick box (tests/aimed_rays.py builds the scene around the
rays).  A random ray passes within 2^-21 (relative) of a box face and still hits what is inside with probability near zero; these do
it by construction, so a culling margin that is too small by a factor of two loses hits here that no random scene shows.

The truth is the oracle on the FLAT original (no bvh node: no box test can have touched it).  CPU tests: the census of what the
aimed rays do (conditions on the inputs, asserted), and the oracle on rtk_scene_optimize's output against the flat original, bit
for bit.  GPU tests (-m gpu): the device in the reference order and in every program form of the fast order against the oracle, bit
for bit -- images, 8-bit images and the counters a closest hit determines; no tolerance anywhere.  A mismatch names the pixel, its
rung and its target kind.

MUTANTS is the record of what these tests see (each mutation made by hand in a scratch copy of the library and the GPU tests run once
on the MI355X; the unmutated library passes all of them); UNREACHED, what they cannot see and why."""
import numpy as np
import pytest

from tests import aimed_rays as ar
from tests import kernel_matrix as km

gpu = pytest.mark.gpu
CASES = [(f, v) for f in ar.FAMILIES for v in ar.CAMERAS]
CASE_IDS = [f"{f}-{v}" for f, v in CASES]
EYES = ("eye", "no_eye")
ORIGIN_FAMILIES = ("spheres", "triangles")
MIN_PER_RUNG = 16            # the census bounds
MAX_OCCLUDED = 0.25
DETERMINED = ("samples", "segments", "surface_hits", "rng_draws")   # the counters a closest hit determines

# One-line changes to a culling budget (rtk_api.cpp, rtk_trace.hip begin_culling32, rtk_optimize.cpp) -> the cases of
# test_device_matches_the_oracle_in_every_program_form that turn red (both eyes unless said), the forms, the rungs and kinds lost.
MUTANTS = {
    "M1 box_margin = 0, min/max bounds rounded to nearest":
        "quads, full x axis, outward: COMPACT forms (837, 2431, 3455 and the counting kernel); 3 .. 13 pixels a frame; corner, axis_corner, "
        "axis_edge at rungs 0 .. 8 (r <= 2^-20)",
    "M2 no 2^-21 (|c| + h) in the centre / half-extent records":
        "mesh_spheres x outward: COMPACT 834 and the counting kernel; 48 pixels; both sphere kinds from radius 2^-17 L down",
    "M3 no 2^-20 extent in build_mixed_program":
        "spheres x far, far_flat, eye only (without the eye the camera is outside the extent: the exact path): MIXED 256 staged and in memory, the "
        "counting kernel; 72 .. 77 pixels; both kinds from radius 2^-17 L down",
    "M5 oi32 bracket with k = 0":
        "quads x far_flat: COMPACT 837 and the counting kernel; 1 pixel, a corner at rung 2 (2^-48)",
    "M6 m2slack32 = 0":
        "mesh_spheres x far, far_flat: COMPACT 834 and the counting kernel; 3 .. 72 pixels; both kinds from radius 2^-17 L down",
    "M7 rtk_scene_optimize's margin = 0":
        "quads, full x every camera: the slot programs (581 literal test, 255 fused test; staged and in memory); 4 .. 30 pixels, corners at rungs "
        "0 .. 3; the COMPACT forms keep the image (their float margins cover it) but their counters leave the oracle's, which loses the same "
        "hits on that description -- test_oracle_agrees_in_both_orders is red on the CPU for the same eight cases",
}
UNREACHED = {
    "M4 below / above = float(x)":
        "the interval's rounding moves a bound by 2^-24 |t|, and |t| <= |b / d| + |o / d|: an eighth of what the box margin (2^-21 |b|, or "
        "2^-20 extent) and the ray's own slack (the 2^-21 |o / d| bracket, m2slack32) carry for the same planes.  It decides only where both of "
        "those errors sit within an eighth of their worst case at once AND an earlier hit lies within 2^-24 of the box's entry; no aimed "
        "ray of any family and camera here does, and nothing honest makes one (the visiting order that finds the farther hit first is the "
        "optimiser's choice)",
}

# The program forms the variant word can steer each family's scene to in the fast order, f64: variant -> (FEAT, IN_LDS) of
# rtk_render_kernel<double, FEAT, false, IN_LDS> by kernel_choice::choose's rules (rtk_kernel_choice.h) -- the MIXED / COMPACT program staged or (lean)
# in memory, the slot program with the fused f64 test (quad/box: the literal test) staged, in memory or behind a box table, the
# hot/cold form.  The slot program of 576 triangles does not fit one CU's LDS (447 KB): that family stages the box table instead.
S, B = 2048, 1024            # F_SPHERE_MEDIA_ONLY: the full family's fog ball has a stationary sphere for a boundary; F_LDS_BOXES
FORMS = {
    "spheres": {0: (256, True), km.V_GLOBAL: (256, False), km.V_SLOT: (128, True), km.V_SLOT | km.V_GLOBAL: (128, False),
                km.V_NO_LDS_BOXES: (256, True)},
    "quads": {0: (837, True), km.V_GLOBAL: (581, False), km.V_SLOT: (581, True), km.V_SLOT | km.V_GLOBAL: (581, False),
              km.V_NO_LDS_BOXES: (837, True)},
    "triangles": {0: (834, True), km.V_GLOBAL: (706 | B, False), km.V_SLOT: (706 | B, False), km.V_SLOT | km.V_NO_LDS_BOXES: (706, False),
                  km.V_NO_LDS_BOXES: (834, True)},
    "mesh_spheres": {0: (834, True), km.V_GLOBAL: (706, False), km.V_SLOT: (706, True), km.V_SLOT | km.V_GLOBAL: (706, False),
                     km.V_NO_LDS_BOXES: (834, True)},
    "full": {0: (383 | S, True), km.V_GLOBAL: (255, False), km.V_SLOT: (255, True), km.V_SLOT | km.V_GLOBAL: (255, False),
             km.V_COLD: (383 | B | S, False), km.V_NO_LDS_BOXES: (383 | S, True)},
}


class _Case:
    """One (family, camera): the scene, its rays and the oracle on the flat original, computed once."""

    def __init__(self, rt, orc, family, view):
        self.family, self.view = family, view
        self.cam, self.aimed = ar.build(rt, view, ar.SEED, family)
        self.hits = orc.hits(self.aimed.desc_ptr, self.aimed.rays, ar.SEED)
        self.linear, self.rgb8, self.counters = orc.render(self.aimed.desc_ptr, self.cam, ar.SEED)
        self._fast = {}
        self._rt, self._orc = rt, orc

    def eye(self, which):
        return self.cam.center if which == "eye" else None

    def fast(self, which):
        """(the optimised description, the oracle's frame of it) for eye = the camera / none."""
        if which not in self._fast:
            scene = self._rt.FastOrderScene(self.aimed, self.eye(which))
            self._fast[which] = (scene, self._orc.render(scene.desc_ptr, self.cam, ar.SEED))
        return self._fast[which]


@pytest.fixture(scope="module")
def cases(rt, orc):
    cache = {}

    def get(family, view):
        if (family, view) not in cache:
            cache[family, view] = _Case(rt, orc, family, view)
        return cache[family, view]
    return get


@pytest.fixture(scope="module")
def origin_cases(rt, orc):
    cache = {}

    def get(family):
        if family not in cache:
            cams, views = ar.origins(rt, ar.SEED, family)
            cache[family] = (cams, views, [orc.render(views[0].desc_ptr, cam, ar.SEED) for cam in cams])
        return cache[family]
    return get


def own_hit(aimed, hits):
    return (hits["hit"] == 1) & ((hits["material"] == aimed.own[:, 0]) | (hits["material"] == aimed.own[:, 1]))


def differing(aimed, got, want, limit=8):
    """The pixels at which two frames differ, each with its ray's rung and target kind -- a finding one can read."""
    bad = np.nonzero((np.asarray(got).reshape(len(aimed.rays), -1) != np.asarray(want).reshape(len(aimed.rays), -1)).any(axis=1))[0]
    w = int(round(len(aimed.rays) ** 0.5))
    lines = [f"pixel ({k % w}, {k // w}) {aimed.describe(k)}: got {np.asarray(got).reshape(len(aimed.rays), -1)[k].tolist()}, "
             f"want {np.asarray(want).reshape(len(aimed.rays), -1)[k].tolist()}" for k in bad[:limit]]
    by_rung = {int(r): int((aimed.rung[bad] == r).sum()) for r in np.unique(aimed.rung[bad])}
    return f"{len(bad)} pixels differ (per rung {by_rung}): " + "; ".join(lines)


def same_frame(aimed, got, want, what):
    """'' or what differs between (linear, rgb8) pairs."""
    if got[0].tobytes() != want[0].tobytes():
        return f"{what}: linear image: " + differing(aimed, got[0], want[0])
    if got[1].tobytes() != want[1].tobytes():
        return f"{what}: 8-bit image: " + differing(aimed, got[1], want[1])
    return ""


# ------------------------------------------------------------------------------------------------ CPU: the inputs, the oracle in both orders
@pytest.mark.parametrize("family,view", CASES, ids=CASE_IDS)
def test_census_of_the_aimed_rays(cases, family, view):
    """Conditions on the inputs, from the oracle on the flat original: at every rung r >= 2^-40 (every radius, for spheres) at
    least 16 rays have their own target as closest hit; quads and triangles at the coin-flip rungs r <= 2^-48 have at least 16 rays
    that hit and 16 that miss, each; at most a quarter of the rays are occluded by another ray's primitive.
    Measured (seed 7, over the thirty cases): own-target hits per rung at least 19 (full-axis at 2^-36; spheres from radius 2^-20 L down
    are the discriminant's own coin flip, |oc|^2 - r^2 having lost r^2, and keep 24 .. 44 of 52), coin-flip rungs 21 .. 109 hits and
    18 .. 79 misses, occluded at most 0.5 %."""
    c = cases(family, view)
    a, h = c.aimed, c.hits
    own = own_hit(a, h)
    assert len(a.rays) == c.cam.image_width * c.cam.image_height and (a.kind >= 0).all()
    assert (h["draws"] == 0).all()                               # no medium in a primary ray's way
    spheres = family in ("spheres", "mesh_spheres")
    first = 0 if spheres else 4
    for rung in range(first, len(a.ladder)):
        n = int(own[a.rung == rung].sum())
        print(f"{family}-{view} rung {rung} ({a.ladder[rung]:.3g}): {int((a.rung == rung).sum())} rays, {n} hit their own target")
        assert n >= MIN_PER_RUNG, (rung, n)
    if not spheres:
        for rung in ar.COIN_RUNGS:
            sel = a.rung == rung
            hit, miss = int((h["hit"][sel] == 1).sum()), int((h["hit"][sel] == 0).sum())
            print(f"{family}-{view} rung {rung} ({a.ladder[rung]:.3g}): {hit} hit, {miss} miss")
            assert hit >= MIN_PER_RUNG and miss >= MIN_PER_RUNG, (rung, hit, miss)
        assert len(set(a.kind.tolist())) == len(ar.KINDS[family])
    if family in ("quads", "full"):
        inside = a.instance >= 0
        assert 0.25 < inside.mean() < 0.42 and len(set(a.instance[inside].tolist())) == ar.N_INSTANCES
        assert own[inside].sum() >= 4 * MIN_PER_RUNG                # the object-space construction meets its targets too
    occluded = (h["hit"] == 1) & ~own
    print(f"{family}-{view}: {occluded.mean():.4f} occluded")
    assert occluded.mean() <= MAX_OCCLUDED
    # a lost hit changes the pixel: the frame shows the targets that are hit and the background where nothing is
    sky = c.linear.reshape(-1, 3)[h["hit"] == 0]
    assert len(sky) == 0 or (sky > 0).all()
    assert c.counters["surface_hits"] >= int((h["hit"] == 1).sum())


@pytest.mark.parametrize("family,view", CASES, ids=CASE_IDS)
def test_oracle_agrees_in_both_orders(cases, orc, family, view):
    """orc.hits and orc.render on the flat original and on rtk_scene_optimize's output: equal in every field, image and
    rng_draws, with and without the eye -- triangles (exact == 1, 'measured') included, since the flat original has no box whose
    rounding could drop a hit."""
    c = cases(family, view)
    for which in EYES:
        scene, (linear, rgb8, counters) = c.fast(which)
        assert scene.exact and scene.info["n_bvh_nodes_out"] > 0
        got = orc.hits(scene.desc_ptr, c.aimed.rays, ar.SEED)
        for field in got.dtype.names:
            x, y = (np.ascontiguousarray(r[field]).reshape(len(got), -1).view(np.uint8) for r in (got, c.hits))
            bad = np.nonzero((x != y).any(axis=1))[0]
            assert len(bad) == 0, (which, field, [c.aimed.describe(k) for k in bad[:8]])
        problem = same_frame(c.aimed, (linear, rgb8), (c.linear, c.rgb8), f"{which}: oracle, fast order")
        assert not problem, problem
        for key in DETERMINED:
            assert counters[key] == c.counters[key], (which, key)
        assert counters["box_tests"] > 0 == c.counters["box_tests"]


def test_forms_name_each_familys_kernels():
    """FORMS against the families' feature words: the default form is the family's MIXED / COMPACT kernel (F_F32_BOX 256), and
    every family has a slot-program form and one that keeps the program in memory."""
    assert set(FORMS) == set(ar.FAMILIES)
    for family, forms in FORMS.items():
        feat, in_lds = forms[0]
        assert feat & 256 and in_lds and (feat & ~(256 | S)) == ar.FAMILY_FEAT[family], family
        assert not forms[km.V_SLOT][0] & 256 and not forms[km.V_GLOBAL][1] and forms[km.V_NO_LDS_BOXES] == forms[0], family


def test_builders_are_deterministic(rt):
    for family in ar.FAMILIES:
        (cam_a, a), (cam_b, b) = (ar.build(rt, "near", ar.SEED, family) for _ in range(2))
        assert bytes(cam_a) == bytes(cam_b) and a.rays.tobytes() == b.rays.tobytes()
        assert ar.desc_bytes(a.desc) == ar.desc_bytes(b.desc) and a.desc.desc.root == b.desc.desc.root
        assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("rung", "kind", "own", "instance"))
    (cams_a, views_a), (cams_b, views_b) = (ar.origins(rt, ar.SEED, "spheres") for _ in range(2))
    assert all(bytes(x) == bytes(y) for x, y in zip(cams_a, cams_b))
    assert ar.desc_bytes(views_a[0].desc) == ar.desc_bytes(views_b[0].desc)
    assert all(x.rays.tobytes() == y.rays.tobytes() for x, y in zip(views_a, views_b))
    _, other = ar.build(rt, "near", ar.SEED + 1, "quads")
    assert ar.desc_bytes(other.desc) != ar.desc_bytes(ar.build(rt, "near", ar.SEED, "quads")[1].desc)


@pytest.mark.parametrize("family", ORIGIN_FAMILIES)
def test_origins_scene_on_the_oracle(rt, orc, origin_cases, family):
    """Sixteen cameras around one cloud: every camera's rays meet targets of their own, and the oracle agrees in both orders."""
    cams, views, frames = origin_cases(family)
    assert len(cams) == ar.N_ORIGINS and len({bytes(c.center) for c in cams}) == ar.N_ORIGINS
    fast = [rt.FastOrderScene(views[0], eye) for eye in (cams[0].center, None)]
    for cam, a, (linear, rgb8, counters) in zip(cams, views, frames):
        h = orc.hits(a.desc_ptr, a.rays, ar.SEED)
        assert own_hit(a, h).sum() >= MIN_PER_RUNG and (h["hit"] == 0).sum() >= 1
        for scene in fast:
            assert orc.hits(scene.desc_ptr, a.rays, ar.SEED).tobytes() == h.tobytes()
            got = orc.render(scene.desc_ptr, cam, ar.SEED)
            problem = same_frame(a, got[:2], (linear, rgb8), "oracle, fast order")
            assert not problem and got[2]["rng_draws"] == counters["rng_draws"], problem


# ------------------------------------------------------------------------------------------------ GPU: the device against the oracle
@gpu
@pytest.mark.parametrize("which", EYES)
@pytest.mark.parametrize("family,view", CASES, ids=CASE_IDS)
def test_device_matches_the_oracle_in_every_program_form(rt, renderer, cases, family, view, which):
    """The flat original in the reference order, then rtk_scene_upload_fast in every program form of FORMS and with work
    counters: every frame equals the oracle's frame of the flat original bit for bit (linear and 8-bit), the counters a closest
    hit determines equal the oracle's on the same description, and the culling kernels test at least the boxes the oracle
    tests.  eye: the extent includes the camera and the primary rays take the float tests; no_eye: where the camera then lies
    outside [-extent, extent]^3 the primaries take the guarded exact path and only the bounces cull in float."""
    c = cases(family, view)
    a, want = c.aimed, (c.linear, c.rgb8)
    problems = []
    renderer.upload(a)
    linear, rgb8, counters = renderer.render_host(c.cam, seed=ar.SEED, count=True)
    problems.append(same_frame(a, (linear, rgb8), want, "reference order"))
    problems += [f"reference order: {key} {counters[key]} != {c.counters[key]}" for key in DETERMINED if counters[key] != c.counters[key]]

    scene, (_, _, fast_counters) = c.fast(which)
    info = renderer.upload_fast(a, c.eye(which))
    assert info["exact"] and info["n_bvh_nodes_out"] == scene.info["n_bvh_nodes_out"]
    for variant, expect in FORMS[family].items():
        name = renderer.kernel_name(rt.RTK_REAL_F64, variant)
        if name != km.kernel_name((km.F64,) + expect[:1] + (False,) + expect[1:]):
            problems.append(f"variant {variant:#x}: kernel {name}, expected {expect}")
        linear, rgb8, _ = renderer.render_host(c.cam, seed=ar.SEED, variant=variant)
        problems.append(same_frame(a, (linear, rgb8), want, f"fast order, variant {variant:#x} ({name})"))
    for variant in (0, km.V_SLOT):
        linear, rgb8, counters = renderer.render_host(c.cam, seed=ar.SEED, count=True, variant=variant)
        what = f"fast order with counters, variant {variant:#x}"
        problems.append(same_frame(a, (linear, rgb8), want, what))
        problems += [f"{what}: {key} {counters[key]} != {fast_counters[key]}" for key in DETERMINED if counters[key] != fast_counters[key]]
        if counters["box_tests"] < fast_counters["box_tests"]:      # conservative culling never tests fewer boxes
            problems.append(f"{what}: box_tests {counters['box_tests']} < the oracle's {fast_counters['box_tests']}")
    problems = [p for p in problems if p]
    assert not problems, "\n".join(problems)


@gpu
@pytest.mark.parametrize("family", ORIGIN_FAMILIES)
def test_sixteen_origins_one_by_one_and_in_one_batch(rt, renderer, origin_cases, family):
    """Sixteen origins for the float tests in ONE scene: every camera's frame, rendered alone and as one view of a
    rtk_render_views batch (the view-batch kernel), equals the oracle's frame of the flat original for that camera."""
    cams, views, frames = origin_cases(family)
    feat = {"spheres": 256, "triangles": 834}[family]
    problems = []
    for eye in (cams[0].center, None):
        renderer.upload_fast(views[0], eye)
        if renderer.kernel_name(rt.RTK_REAL_F64, 0) != km.kernel_name((km.F64, feat, False, True)):
            problems.append("kernel " + renderer.kernel_name(rt.RTK_REAL_F64, 0))
        if renderer.view_kernel_name(rt.RTK_REAL_F64, 0) != f"rtk_view_batch_kernel<double, {feat}u, true>":
            problems.append("view kernel " + renderer.view_kernel_name(rt.RTK_REAL_F64, 0))
        batch_linear, batch_rgb8, _ = renderer.render_views(cams, seed=ar.SEED)
        for v, (cam, a, (linear, rgb8, _)) in enumerate(zip(cams, views, frames)):
            alone = renderer.render_host(cam, seed=ar.SEED)
            problems.append(same_frame(a, alone[:2], (linear, rgb8), f"camera {v} alone, eye {eye is not None}"))
            problems.append(same_frame(a, (batch_linear[v], batch_rgb8[v]), (linear, rgb8), f"camera {v} in the batch, eye {eye is not None}"))
    problems = [p for p in problems if p]
    assert not problems, "\n".join(problems)
