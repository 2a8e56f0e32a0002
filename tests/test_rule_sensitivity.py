"""Can the inputs of the device comparisons tell a subtly wrong kernel from the rule?  (CPU only; no kernel is involved.)

The a-trous filter, temporal accumulation and guided upsampling are compared on the device with a float64 restatement of the
rule in include/rtk.h, to 1e-4 of max(1, |ref|).  That comparison sees a term of the rule only if the term moves the output on the
inputs used.  Here every VARIANT -- a deliberate one-term deviation, what a subtly wrong kernel would compute -- must move the
restatement's own output by at least 10 x that tolerance on at least 1 % of the pixels (at least 16) of the 64x48 and the 37x23
case of tests/rule_inputs.py, under at least one configuration (options, form, factor, camera path) that the device comparison
runs.  For temporal accumulation the count is taken after the fragile-pixel exclusion.  This is a condition on the inputs, not a
measurement: the inputs were shaped until it held.  UNREACHED lists what cannot be seen and why.  (The filter's own 48x64 case,
height x width, is the 64x48 one here.)

The last tests keep the record of why the rich inputs exist: on the earlier synthetic inputs set 2 is set 1 bit for bit and whole
terms leave the output where it was."""
import math

import numpy as np
import pytest

from tests.rule_inputs import rich_filter_case, rich_guides, view_of
from tests.test_denoise import DEFAULTS as FILTER_DEFAULTS
from tests.test_denoise import _synthetic, reference_denoise
from tests.test_guided_denoise import _doubled, _synthetic_guides, reference_denoise_guided
from tests.test_temporal import DEFAULTS as TEMPORAL_DEFAULTS
from tests.test_temporal import FRAGILE, PATHS, _history, reference_temporal, rich_frames, synthetic_camera, synthetic_frames, synthetic_guides
from tests.test_temporal import OTHER as TEMPORAL_OTHER
from tests.test_upsample import DEFAULTS as UPSAMPLE_DEFAULTS
from tests.test_upsample import FACTORS, reference_upsample, rich_case, synthetic_case
from tests.test_upsample import OTHER as UPSAMPLE_OTHER

TOL = 1e-4                                                        # the device comparisons' tolerance, of max(1, |ref|)
SIZES = [(64, 48), (37, 23)]                                      # (width, height)


def need(w, h):
    return max(16, math.ceil(0.01 * w * h))


def moved(ref, alt, keep=None):
    """Pixels at which any output of `alt` is further than 10 x TOL x max(1, |ref|) from `ref` (a NaN counts as moved)."""
    out = None
    for r, a in zip(ref, alt):
        with np.errstate(invalid="ignore"):
            far = ~(np.abs(a - r) <= 10 * TOL * np.maximum(1.0, np.abs(r)))
        far = far.any(-1) if far.ndim == 3 else far
        out = far if out is None else out | far
    return int((out if keep is None else out & keep).sum())


def _v(name):
    return lambda o: {"variant": name}                            # noqa: E731


def _scaled(key, factor):
    return lambda o: {key: o[key] * factor}                       # noqa: E731


# What every rule with guide weights shares (the filter, its guided form, upsampling).
SHARED = {"w_n exponent halved": _scaled("sigma_n", 0.5), "cosine without the division by the lengths": _v("cos_without_lengths"),
          "sigma_z x 1.2": _scaled("sigma_z", 1.2), "the 1e-3 z_p term dropped": _v("no_z_term"), "depth gradient by min": _v("gradient_min"),
          "hit fraction == 0 read as < 1": _v("hit_below_1")}
GUIDED = {"w_n from set 1 only": _v("wn_set1_only"), "w_z from set 1 only": _v("wz_set1_only"), "w_z of set 2 with set 1's hit fraction": _v("wz2_with_hit1"),
          "w_z of set 2 with set 1's gradient": _v("wz2_with_grad1")}
FIRST_ALBEDO = {"w_a on the first albedo": _v("wa_first_albedo")}

# (variants, forms they apply to)
FILTER_FORMS = ("plain", "guided", "demodulated")
FILTER_VARIANTS = [(SHARED, FILTER_FORMS), (GUIDED, ("guided", "demodulated")), (FIRST_ALBEDO, ("guided",)),
                   ({"sigma_a x 1.2": _scaled("sigma_a", 1.2)}, ("plain", "guided")),
                   ({"sigma_l x 1.1": _scaled("sigma_l", 1.1), "gv = the centre variance": _v("gv_centre"), "variance propagated with w": _v("variance_w")}, FILTER_FORMS),
                   ({"demodulation floor 0": _v("floor_0"), "variance divided per channel": _v("variance_per_channel")}, ("demodulated",))]
# two of the device comparison's option sets: one iteration, and the "sigmas" set
FILTER_OPTIONS = {"it1": dict(FILTER_DEFAULTS, iterations=1), "sigmas": dict(FILTER_DEFAULTS, iterations=3, sigma_l=2.0, sigma_n=32.0, sigma_z=0.5, sigma_a=0.3)}

UPSAMPLE_FORMS = ("plain", "demodulated")
UPSAMPLE_VARIANTS = [(SHARED, UPSAMPLE_FORMS), (GUIDED, UPSAMPLE_FORMS), (FIRST_ALBEDO, ("plain",)), ({"sigma_a x 1.2": _scaled("sigma_a", 1.2)}, ("plain",)),
                     ({"o = 1": _v("o_is_1"), "the floor 1e-3 -> 0": _v("floor_0"), "support with omega": _v("support_omega")}, UPSAMPLE_FORMS),
                     ({"A_p and A_q swapped": _v("albedo_swapped")}, ("demodulated",))]
UPSAMPLE_OPTIONS = {"defaults": UPSAMPLE_DEFAULTS, "other": UPSAMPLE_OTHER}

TEMPORAL_VARIANTS = {"cosine without the division by the lengths": "cos_without_lengths", "hit fraction == 0 read as < 1": "hit_below_1",
                     "tap validity with g'[3] != 0": "tap_hit_nonzero", "depth test against a g'[7]-relative tolerance": "depth_test_relative_to_tap",
                     "albedo check on g[0..2]": "albedo_check_first", "history keeps the first albedo": "history_first_albedo",
                     "history keeps the end-hit fraction": "history_end_hit", "sum omega var'": "variance_omega", "n_out without the cap": "no_history_cap"}
TEMPORAL_OPTIONS = {"defaults": TEMPORAL_DEFAULTS, "other": TEMPORAL_OTHER}

# (rule, form, variant, (w, h)) -> why no input can show it.  The test asserts that these stay unreached, so the list stays true.
UNREACHED = {
    ("temporal", "", "tap validity with g'[3] != 0", size): "a hit fraction is never negative: > 0 and != 0 agree on every valid input" for size in SIZES}
# Terms of the list "all three rules" that temporal accumulation does not have: w_n's exponent, sigma_z, the 1e-3 z_p term and
# the depth gradient belong to the guide weights; the temporal rule tests a cosine and a relative depth against thresholds.


# ------------------------------------------------------------------------------------------------------------- filter --
def filter_inputs(kind, w, h):
    """(noisy, guides (H, W, 16), se): the rich case, or the earlier synthetic one (kind = "old")."""
    return rich_filter_case(h, w) if kind == "new" else _synthetic_guides(h, w)


def filter_rows(kind, w, h):
    """[(form, variant name, best count, option set)] on the filter inputs of `kind`."""
    noisy, g, se = filter_inputs(kind, w, h)
    rows = []
    for form in FILTER_FORMS:
        guides = _doubled(g[..., 0:8]) if form == "plain" else g  # the plain filter is the guided one with set 2 = set 1 (asserted below)
        demod = form == "demodulated"
        refs = {name: reference_denoise_guided(noisy, guides, se, demodulate=demod, **opts) for name, opts in FILTER_OPTIONS.items()}
        for variants, forms in FILTER_VARIANTS:
            if form not in forms:
                continue
            for label, change in variants.items():
                with np.errstate(invalid="ignore"):               # (a floor of 0 divides by albedos that are 0)
                    best = max((moved((refs[name],), (reference_denoise_guided(noisy, guides, se, demodulate=demod, **dict(opts, **change(opts))),)), name)
                               for name, opts in FILTER_OPTIONS.items())
                rows.append((form, label) + best)
    return rows


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_filter_inputs_show_every_term(size):
    w, h = size
    noisy, g, se = filter_inputs("new", w, h)
    assert np.array_equal(reference_denoise_guided(noisy, _doubled(g[..., 0:8]), se, **FILTER_OPTIONS["sigmas"]),
                          reference_denoise(noisy, g[..., 0:8], se, **FILTER_OPTIONS["sigmas"]))   # "plain" below is rtk_denoise's rule
    failed = []
    for form, label, count, where in filter_rows("new", w, h):
        print("filter %-12s %-45s %5d of %d pixels (need %d) with %s" % (form, label, count, w * h, need(w, h), where))
        if (count >= need(w, h)) == (("filter", form, label, size) in UNREACHED):
            failed.append((form, label, count))
    assert not failed, failed


# ----------------------------------------------------------------------------------------------------------- upsample --
def upsample_rows(rt, kind, w, h):
    """[(form, variant name, best count, configuration)] on the upsampling inputs of `kind`."""
    make = rich_case if kind == "new" else synthetic_case
    best = {}
    for f in FACTORS:
        _, colour, se, low_g, g = make(rt, w, h, f)
        for form in UPSAMPLE_FORMS:
            for name, opts in UPSAMPLE_OPTIONS.items():
                ref = reference_upsample(w, h, f, colour, se, low_g, g, demodulate=form == "demodulated", **opts)
                for variants, forms in UPSAMPLE_VARIANTS:
                    if form not in forms:
                        continue
                    for label, change in variants.items():
                        alt = reference_upsample(w, h, f, colour, se, low_g, g, demodulate=form == "demodulated", **dict(opts, **change(opts)))
                        with np.errstate(invalid="ignore"):
                            count = moved((ref[0], np.sqrt(ref[1]), ref[2]), (alt[0], np.sqrt(alt[1]), alt[2]))
                        best[(form, label)] = max(best.get((form, label), (-1, "")), (count, "f = %d, %s" % (f, name)))
    return [key + value for key, value in best.items()]


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_upsample_inputs_show_every_term(rt, size):
    w, h = size
    failed = []
    for form, label, count, where in upsample_rows(rt, "new", w, h):
        print("upsample %-12s %-45s %5d of %d pixels (need %d) with %s" % (form, label, count, w * h, need(w, h), where))
        if (count >= need(w, h)) == (("upsample", form, label, size) in UNREACHED):
            failed.append((form, label, count))
    assert not failed, failed


# ----------------------------------------------------------------------------------------------------------- temporal --
def temporal_rows(rt, kind, w, h):
    """[("", variant name, best count in one frame, configuration)] on the frames of `kind`: every path and option set of the
    device comparison, the history being the rule's own previous outputs, fragile pixels left out."""
    make = rich_frames if kind == "new" else synthetic_frames
    best = {}
    for path in PATHS:
        frames = make(rt, path, w, h)
        for name, opts in TEMPORAL_OPTIONS.items():
            prev = None
            for k, (cam, colour, g, se) in enumerate(frames):
                out, var, n, _, margin = reference_temporal(cam, colour, g, se, prev, **opts)
                for label, variant in TEMPORAL_VARIANTS.items() if k else ():
                    alt = reference_temporal(cam, colour, g, se, prev, variant=variant, **opts)
                    count = moved((out, np.sqrt(var), n), (alt[0], np.sqrt(alt[1]), alt[2]), margin >= FRAGILE)
                    best[label] = max(best.get(label, (-1, "")), (count, "%s, %s, frame %d" % (path, name, k)))
                prev = _history(rt, cam, out.astype(np.float32), var.astype(np.float32), n.astype(np.float32), g)
    return [("", label) + value for label, value in best.items()]


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_temporal_inputs_show_every_term(rt, size):
    w, h = size
    failed = []
    for _, label, count, where in temporal_rows(rt, "new", w, h):
        print("temporal %-45s %5d of %d pixels (need %d) with %s" % (label, count, w * h, need(w, h), where))
        if (count >= need(w, h)) == (("temporal", "", label, size) in UNREACHED):
            failed.append((label, count))
    assert not failed, failed


# ------------------------------------------------------------------------------- the record: what the old inputs hid --
def test_old_temporal_and_upsample_guides_have_one_set_and_tame_channels(rt):
    for w, h in SIZES:
        g = synthetic_guides(synthetic_camera(rt, w, h, (0.0, 2.0, 6.0))).astype(np.float64)
        assert np.array_equal(g[..., 8:16], g[..., 0:8])                                   # set 2 is set 1 bit for bit
        assert set(np.unique(g[..., 3])) <= {0.0, 1.0}                                     # hit fractions 0 / 1
        length = np.sqrt((g[..., 4:7] ** 2).sum(-1))[g[..., 3] > 0]
        assert np.abs(length - 1.0).max() <= 1e-7                                          # unit normals
        assert len(np.unique(g[g[..., 3] > 0][:, 0:3], axis=0)) == 3                       # one flat albedo per surface
        # the rich guides of the same camera
        r = rich_guides(view_of(synthetic_camera(rt, w, h, (0.0, 2.0, 6.0)))).astype(np.float64)
        hit = r[..., 3] > 0
        assert (r[..., 8:16] != r[..., 0:8]).any(-1).mean() > 0.2 and (hit & (r[..., 8:16] == r[..., 0:8]).all(-1)).mean() > 0.2
        assert set(np.unique(r[..., 3])) == {0.0, 0.25, 0.5, 0.75, 1.0} and set(np.unique(r[..., 11])) == {0.0, 0.25, 0.5, 0.75, 1.0}
        assert (hit & (r[..., 11] == 0)).sum() >= 16 and (~hit & (r[..., 11] > 0)).sum() >= 16   # first hit without end hit, and the reverse
        length = np.sqrt((r[..., 4:7] ** 2).sum(-1))[hit]
        assert 0.3 - 1e-6 <= length.min() < 0.4 and 0.9 < length.max() <= 1.0 + 1e-6
        assert ((r[..., 8:11] < 0.02).any(-1) & hit).sum() >= 4                            # seen albedos below the demodulation floor


def test_old_upsample_inputs_hide_the_albedo_weight_and_set_2(rt):
    for w, h in SIZES:
        rows = {(form, label): count for form, label, count, _ in upsample_rows(rt, "old", w, h)}
        for label in list(GUIDED) + list(FIRST_ALBEDO) + ["sigma_a x 1.2"]:
            assert rows[("plain", label)] == 0, (label, rows[("plain", label)])
        assert rows[("plain", "w_n exponent halved")] >= need(w, h) and rows[("plain", "sigma_z x 1.2")] >= need(w, h)   # those two it did see
        for f in FACTORS:                                         # sigma_a x 1.2: not one bit of the output moves
            _, colour, se, low_g, g = synthetic_case(rt, w, h, f)
            a = reference_upsample(w, h, f, colour, se, low_g, g)
            b = reference_upsample(w, h, f, colour, se, low_g, g, sigma_a=0.12)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_old_temporal_inputs_hide_the_history_record_and_the_albedo_check(rt):
    for w, h in SIZES:
        rows = {label: count for _, label, count, _ in temporal_rows(rt, "old", w, h)}
        for label in ("albedo check on g[0..2]", "history keeps the first albedo", "history keeps the end-hit fraction", "hit fraction == 0 read as < 1",
                      "cosine without the division by the lengths"):
            assert rows[label] == 0, (label, rows[label])


def test_old_filter_inputs_hide_the_normal_weight_and_the_lengths():
    for h, w in ((48, 64), (75, 100)):
        noisy, aov, se = _synthetic(h, w)
        ref = reference_denoise(noisy, aov, se)
        assert set(np.unique(aov[..., 3])) == {0.0, 1.0}
        assert np.abs(reference_denoise(noisy, aov, se, sigma_n=64.0) - ref).max() < 1e-9          # w_n is only ever 1 or about 1e-19
        assert np.abs(reference_denoise(noisy, aov, se, sigma_a=0.12) - ref).max() < TOL           # below the comparison's tolerance
        # unit normals: a kernel that never divides by the lengths stays inside the tolerance
        assert np.abs(reference_denoise_guided(noisy, _doubled(aov), se, variant="cos_without_lengths") - ref).max() < TOL
        noisy, g, se = rich_filter_case(h, w)
        rich = reference_denoise(noisy, g[..., 0:8], se)
        assert moved((rich,), (reference_denoise(noisy, g[..., 0:8], se, sigma_n=64.0),)) >= need(w, h)
        assert moved((rich,), (reference_denoise(noisy, g[..., 0:8], se, sigma_a=0.12),)) >= need(w, h)
