"""The a-trous filters on planted planes, without a device: the fp32 restatements (denoise_ref.atrous_numpy,
guided_denoise_ref.guided_numpy) against the float64 truth (denoise_ref.atrous_truth64, guided_truth64) on every case of
denoise_ref.cases().

The two must take the same decisions — which taps are left out and why, which pixels stay, where g = 0 — on every pixel but
the ones a case lists as "unchanged" (a first-hit distance whose sigmaWorld^2 underflows in binary32 only: invWorld = inf, the
centre's e is NaN and the restatement leaves the pixel alone; in float64 every other tap weighs 0 and the centre's colour comes
back, which is the same picture).  Every skip rule of the kernels must have fired in the truth's record somewhere, or the cases
do not plant what they say they do.

E_ref( case ) = max |restatement - truth| over the colour channels the truth has finite (variance: relative to |truth|) is the
yardstick of tests/test_gpu_filter_planes.py: the device may be 4 E_ref + an ulp from the truth.  It is measured afresh in every
run; the table is a record of one run — restatement on x86-64 numpy, device on an MI355X — the largest value per class:

  class                                          kind    E_ref colour  device colour  E_ref variance  device variance
  1 hit / miss layouts the stencil straddles     plain   1.788e-07     1.788e-07      -               -
                                                 guided  1.788e-07     1.788e-07      3.877e-06       3.207e-06
  2 colours that are not finite                  plain   2.276e-07     2.538e-07      -               -
                                                 guided  3.915e-07     3.879e-07      4.754e-06       6.357e-06
  3 variances (guided only)                      guided  3.988e-07     3.106e-07      4.007e-06       3.854e-06
  4 feature distances that overflow binary32     plain   4.041e-07     3.991e-07      -               -
                                                 guided  5.458e-07     5.458e-07      5.650e-06       7.165e-06
  5 underflowing weights                         plain   0             0              -               -
                                                 guided  0             0              2.002e-07       2.002e-07
  6 standard deviations of 0                     plain   2.439e-07     3.034e-07      -               -
                                                 guided  3.975e-07     3.439e-07      4.105e-06       4.351e-06
  7 degenerate first-hit distances               plain   3.351e-07     2.671e-07      -               -
                                                 guided  2.920e-07     3.178e-07      3.039e-06       2.957e-06
  8 neutral, 1 x 1 .. 70 x 9, 1 .. 8 passes      plain   2.583e-07     2.580e-07      -               -
                                                 guided  3.386e-07     3.439e-07      4.718e-06       3.060e-06
(Class 5's colours are a constant and lone pixels whose taps weigh nothing: every result is exact.  Class 4's colours reach
1e19, where one binary32 ulp is 1.1e12; the pixels that hold them come back exactly.)

A wrong filter must leave that band: the last test mutates copies of the restatements' source and holds them to
denoise_ref.against_truth, the check the device gets."""
import inspect

import numpy as np
import pytest

import denoise_ref as R
import guided_denoise_ref
import hand_scenes

RUNS = [pytest.param(case, kind, id="%s-%s" % (case.name, ("plain", "guided")[kind])) for case in R.cases() for kind in case.kinds]


def test_the_table_has_every_size_pass_count_and_class():
    neutral = {(c.w, c.h, c.params[0].passes) for c in R.cases() if c.classes == {8}}
    assert neutral == {(w, h, p) for (w, h) in R.SIZES for p in R.PASSES}
    assert set().union(*(c.classes for c in R.cases())) == set(R.CLASSES)
    assert len({c.name for c in R.cases()}) == len(R.cases())
    for c in R.cases():
        assert c.w * c.h <= 4096 and all(1 <= c.params[kind].passes <= 8 for kind in c.kinds)
        assert (3 in c.classes) <= (c.kinds == (1,))                                  # variances are the guided filter's
        assert not c.unchanged or c.classes == {7}                                    # only class 7 may list pixels


@pytest.mark.parametrize("case, kind", RUNS)
def test_restatement_and_truth_decide_alike(case, kind):
    r = R.evaluate(case, kind)
    assert len(r.rest_record) == len(r.truth_record) == case.params[kind].passes
    apart = np.zeros((case.h, case.w), bool)
    for rest, truth in zip(r.rest_record, r.truth_record):
        assert (rest.reason != 255).all() and (truth.reason != 255).all()
        apart |= ~rest.same_decisions(truth)
    # the pixels that cannot agree are the listed ones, all of them planted with a degenerate distance
    assert set(zip(*np.nonzero(apart))) <= set(case.unchanged), sorted(set(zip(*np.nonzero(apart))) - set(case.unchanged))[:8]
    for (y, x) in case.unchanged:
        t = case.features[0, y, x, 3]
        assert 0 < t < 1e-20 and case.features[1, y, x, 3] == 1
        assert apart[y, x]                                                            # ... and they do part, or the list is stale
        assert all(rec.stayed[y, x] for rec in r.rest_record)                         # the expected outcome, on the restatement
        assert R._same_bits(r.rest[0][y, x], case.image[y, x]).all()
        if kind == 1:
            assert R._same_bits(r.rest[1][y, x], case.variance[y, x]).all()
    # values: what is not finite in one is not in the other, and the restatement passes the device's check against the truth
    print("%s kind %d: E_ref colour %.3e%s" % (case.name, kind, r.e_ref, "" if kind == 0 else ", variance %.3e" % r.e_ref_variance))
    # relative variance errors mean the filter's only where sum w w V does not cancel: the cases are planted so that it does not
    assert all(rec.condition.max() < 1.001 for rec in r.truth_record)
    failures, _, _ = R.against_truth(case, kind, *r.rest)
    assert not failures, failures
    assert np.isfinite(r.e_ref) and (kind == 0 or np.isfinite(r.e_ref_variance))


def test_a_constant_image_under_the_pure_spline_is_the_constant():
    for case in (c for c in R.cases() if c.name.startswith("off_all_constant")):
        for kind in case.kinds:
            r = R.evaluate(case, kind)
            assert np.abs(r.truth[0] - case.image[..., :3].astype(np.float64)).max() < 1e-15
            assert R.colour_error(r.rest[0], case.image[..., :3].astype(np.float64)) <= 4 * r.e_ref + R.ulp32(R.largest_colour(case))


def fired(classes, what, kinds=(0, 1)):
    """The pixels over all passes of the cases of `classes` where what( truth record, case ) holds."""
    count = 0
    for case in R.cases():
        if case.classes & set(classes):
            for kind in set(case.kinds) & set(kinds):
                count += sum(int(np.count_nonzero(what(rec, case))) for rec in R.evaluate(case, kind).truth_record)
    return count


def test_every_rule_fired_in_the_truth():
    skipped = lambda code: (lambda rec, case: (rec.reason == code).any(-1))
    assert fired({2}, skipped(R.COLOUR), (0,)) and fired({2}, skipped(R.COLOUR), (1,))
    assert fired({3}, skipped(R.VARIANCE), (1,))
    assert fired({4}, skipped(R.OVERFLOW), (0,)) and fired({4}, skipped(R.OVERFLOW), (1,))
    assert fired({1}, skipped(R.DIVIDE), (0,)) and fired({1}, skipped(R.DIVIDE), (1,))
    assert fired({2}, lambda rec, case: rec.stayed, (0,)) and fired({2, 3}, lambda rec, case: rec.stayed, (1,))
    assert fired({3}, lambda rec, case: rec.g_zero, (1,))
    assert fired({5}, lambda rec, case: rec.tiny, (0,)) and fired({5}, lambda rec, case: rec.tiny, (1,))
    assert fired({8}, lambda rec, case: rec.only_centre(), (0,)) and fired({8}, lambda rec, case: rec.only_centre(), (1,))
    # a stayed pixel of every kind of reason: a centre that is not finite, a variance that is not, sd = NaN under a negative g
    assert fired({7}, skipped(R.OVERFLOW))                                            # the float64 side of an unchanged pixel
    # with the luminance term off a tap that is not finite is not left out: it spreads
    case = next(c for c in R.cases() if c.name == "nonfinite_colour_luminance_off")
    assert (~np.isfinite(R.evaluate(case, 1).truth[0]).all(-1)).sum() > 9 * (~np.isfinite(case.image[..., :3]).all(-1)).sum()
    # class 5 plants e where it says: 80 .. 110 at the lone pixels' neighbours in the first pass
    for case in (c for c in R.cases() if 5 in c.classes and c.params[0].passes == 1):
        kind = case.kinds[0]
        assert R.evaluate(case, kind).truth_record[0].tiny.sum() >= 26


@pytest.mark.parametrize("shape", sorted(hand_scenes.FEATURE_CAMERAS))
def test_feature_cameras_keep_every_pixel_centre_ray_off_edges_silhouettes_and_ties(pbr, shape):
    """What tests/test_gpu_filter_planes.py asserts before it looks at the device, here too: the cameras of
    hand_scenes.FEATURE_CAMERAS are chosen for it."""
    from test_gpu_filter_planes import feature_case_on_the_host
    sc, rays, t, face, hit = feature_case_on_the_host(pbr, shape)
    print("%s: %d faces, %d seen, %.0f %% of the pixels hit" % (shape, sc.arrays["facesV"].shape[0], len(set(face[hit].tolist())), 100 * hit.mean()))


# ---- a wrong filter leaves the band ---------------------------------------------------------------------------------------

def mutant(function, old, new, caller=None):
    """A copy of a restatement with one piece of its source replaced; caller: the function of the same module to return in its
    place, bound to the copy."""
    source = inspect.getsource(function)
    assert source.count(old) == 1, old
    namespace = dict(vars(inspect.getmodule(function)))
    exec(compile(source.replace(old, new), "<mutant of %s>" % function.__name__, "exec"), namespace)
    if caller is not None:
        exec(compile(inspect.getsource(caller), "<caller of a mutant>", "exec"), namespace)
    return namespace[(caller or function).__name__]


def guided_with(pass_function):
    def run(image, var, features, params, px_dim):
        colour, v = np.asarray(image, np.float32)[..., :3], np.asarray(var, np.float32)
        for k in range(int(params.passes)):
            colour, v = pass_function(colour, v, features, 1 << k, params.sigma_luminance, params.sigma_normal, params.sigma_world,
                                      params.sigma_albedo, px_dim)
        out = np.asarray(image, np.float32).copy()
        out[..., :3] = colour
        return out, v
    return run


MUTANTS = {
    # kind, the restatement, what is replaced, by what, the classes whose cases must notice
    "no hit / miss divide": (0, R.atrous_numpy, "ok = inside & (n[..., 3] == normal[..., 3])", "ok = inside", {1}),
    "sigma_color is not halved": (0, R.atrous_numpy, "f32(params.sigma_color) / f32(1 << k)", "f32(params.sigma_color)", {8}),
    "taps outside the image are clamped in": (0, R.atrous_numpy, "inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)", "inside = ty == ty", {8}),
    "the world term takes the tap's distance": (0, R.atrous_numpy, "sigma_world = world_scale * position[..., 3]",
                                                "sigma_world = world_scale * np.roll(position[..., 3], 1, axis=1)", {8}),
    "a spline of 0.05 at the ends": (0, R.atrous_numpy, "[0.0625, 0.25, 0.375, 0.25, 0.0625]", "[0.05, 0.25, 0.375, 0.25, 0.05]", {8}),
    "no finite1( c.w ) test": (1, guided_denoise_ref.guided_pass, "ok &= (e < np.inf) & np.isfinite(v)", "ok &= (e < np.inf)", {3}),
    "w * c.w in place of ( w * w ) * c.w": (1, guided_denoise_ref.guided_pass, "(wt * wt) * v", "wt * v", {8}),
    "the local variance skips no tap": (1, guided_denoise_ref.local_variance, "ok = inside & np.isfinite(v)", "ok = inside", {3}),
    "1e-3 in place of 1e-6": (1, guided_denoise_ref.guided_pass, "F(1e-6)", "F(1e-3)", {3, 5}),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_wrong_filter_leaves_the_band(name):
    kind, function, old, new, classes = MUTANTS[name]
    wrong = mutant(function, old, new, guided_denoise_ref.guided_pass if function is guided_denoise_ref.local_variance else None)
    noticed = []
    for case in R.cases():
        if case.classes & classes and kind in case.kinds and case.w * case.h > 64:
            p, feats = case.params[kind], tuple(case.features)
            out = (wrong(case.image, feats, p, R.PX_DIM), None) if kind == 0 else guided_with(wrong)(case.image, case.variance, feats, p, R.PX_DIM)
            failures, _, _ = R.against_truth(case, kind, *out)
            noticed.append(bool(failures))
    print("%s: noticed in %d of %d cases" % (name, sum(noticed), len(noticed)))
    assert any(noticed)
