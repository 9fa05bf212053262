"""The oracle's Phong-tessellation stages (orc_math "cbrt", orc_solve_cubic, orc_phong_face) against float64 references
that share no algebra with them (tests/phong_ref.py): np.cbrt, np.roots + Newton in longdouble, and Newton's iteration
on S( u, v ) = o + t d from the patch's definition.  No GPU: this holds the oracle — and with it, through the bit-exact
parity tests, the HIP kernels' exact arithmetic — to the definitions, and holds the reference module to something before
any device is involved.  test_gpu_phong_ref.py runs the same drivers through the device, in both arithmetics.

MEASURED on the oracle (batches of phong_ref.BATCH = 4096 items, seeds fixed in phong_ref.py), and the bounds set from it:

  cbrt         1 058 185 values (phong_ref.cbrt_inputs): worst error 0.49999993 ulp of the float32 result against np.cbrt in
               float64 — correctly rounded on this set; asserted <= 1 ulp.
  solveCubic   cubic_batch: 514 of 4096 counts ambiguous (discriminant within COUNT_MARGIN = 16 float32 rounding bounds of
               0: the nearly-quadratic cubics and the roots spread over 1e-3 ... 1e3, whose float32 discriminant is rounding
               noise); off that set every count right.  Worst |root - true| / ( 2^-23 ( cond + |r| ) ) = 115.4 (a nearly
               quadratic cubic, a0 = 4.8e-4: Cardano's small root carries the cancellation against w = a1 / 3 a0 and one
               Newton step does not take all of it back); by kind: three roots 0.42, one root 16.0, spread roots 82.2,
               random 40.4, nearly quadratic 115.4, quadratics 0.42, linear 0.16; median 0.076.
               K_CUBIC = 512 (the next power of two at least 4 x 115.4).
  patches      per batch, off the ambiguous set: failures (hit / miss differs, or |t - t_ref| > 1e-3 max( 1, t_ref )) against
               the cap FAIL_MAX = 0.5 %, the ambiguous share against AMBIGUOUS_MAX = 10 %, the median of the relative error
               in t (MEDIAN_T, bound 8 x), the worst and the median angle to the reference's normal:
                 batch        ambiguous  failures          median rel t   worst angle  median angle
                 random 0.3   0.78 %     0.12 % (2 + 3)    1.04e-7        2.58e-3      2.25e-7
                 random 0.6   0.59 %     0.02 % (1 + 0)    7.76e-8        8.06e-4      2.09e-7
                 random 1.0   0.73 %     0.02 % (0 + 1)    7.10e-8        1.95e-4      2.28e-7
                 curved       0.63 %     0                 6.08e-8        3.30e-3      2.50e-7
                 axis         0.76 %     0                 7.08e-8        4.29e-3      1.75e-7
                 tNear < 0    0.71 %     0.02 % (0 + 1)    7.48e-8        1.38e-3      2.14e-7
                 interval     38.6 %     0                 8.22e-8        1.95e-5      2.38e-7
               (failures: hit / miss differs + t beyond 1e-3.  interval: the boundaries sit next to the hits by construction,
               phong_ref.interval_batch; its ambiguous share is not capped.)  The oracle never reported a hit the reference
               lacks on these batches.  The normal is compared where both hit within the tolerance in t and |dot( ns, r )| >
               phong_ref.NS_TOL; it is of unit length to 1.4e-7 (bound 1e-5).
               ANGLE_MAX = 2^-5 rad (the next power of two at least 4 x 4.29e-3); the median angle is bounded too, at 8 x
               the measured one (MEDIAN_ANGLE), so that a rare wrong choice between the two normals cannot hide under the
               worst case's bound and a systematic one cannot either.
  recorded, not asserted beyond the hard invariants (what the reference's formulas give; Phong tessellation renders so):
    nearly flat  the conic method loses most hits of a nearly flat patch: of the hits the float64 reference finds the oracle
                 misses 100 % with three equal normals (the renderer sends those to the flat test), 86 - 88 % at a normal
                 spread of 1e-7 ... 1e-4, 60 % at 1e-4 ... 1e-3, 7.6 % at 1e-3 ... 1e-2; 51 hits the reference lacks.  All
                 cubic coefficients go to 0 with the C terms and the pencil's roots are rounding noise.  No NaN.
    through the  origin = -4 dir: cross( origin, dir ) is 0 only where its products are exact; elsewhere the fused
    origin       multiply-add of the cross product leaves its rounding residue, whose normalisation is a plane normal that
                 means nothing: 68 % of the non-ambiguous cases fail, 71 hits the reference lacks, no NaN in the outputs (a
                 NaN n1 ends in solveCubic's `> 0` tests: no root, a miss).  A camera AT the origin is such a case.
"""
import numpy as np
import pytest

import phong_ref as pr
from conftest import same_values

K_CUBIC = 512
FAIL_MAX = 0.005
AMBIGUOUS_MAX = 0.10
T_TOL = 1e-3
ANGLE_MAX = 2.0 ** -5
MEDIAN_T = {"random 0.3": 1.04e-7, "random 0.6": 7.76e-8, "random 1.0": 7.10e-8, "curved": 6.08e-8, "axis": 7.08e-8,
            "tnear": 7.48e-8, "interval": 8.22e-8}
MEDIAN_ANGLE = {"random 0.3": 2.25e-7, "random 0.6": 2.09e-7, "random 1.0": 2.28e-7, "curved": 2.50e-7, "axis": 1.75e-7,
                "tnear": 2.14e-7, "interval": 2.38e-7}
MEDIAN_FACTOR = 8.0


class Stages:
    """The three stages under test as callables, and the factor on the bounds that scale with the arithmetic."""

    def __init__(self, cbrt, solve_cubic, phong_face, scale=1.0):
        self.cbrt, self.solve_cubic, self.phong_face, self.scale = cbrt, solve_cubic, phong_face, scale


@pytest.fixture(scope="module")
def stages(oracle):
    return Stages(lambda x: oracle.math("cbrt", x), oracle.solve_cubic, oracle.phong_face)


BATCHES = {
    "random 0.3": lambda: pr.random_batch(0.3), "random 0.6": lambda: pr.random_batch(0.6), "random 1.0": lambda: pr.random_batch(1.0),
    "curved": pr.curved_batch, "axis": pr.axis_batch, "tnear": pr.negative_near_batch, "interval": pr.interval_batch,
    "flat": lambda: pr.nearly_flat_batch()[0], "origin": pr.through_origin_batch,
}
_ITEMS = {}


def batch_items(name):
    if name not in _ITEMS:
        items = BATCHES[name]()
        items.setflags(write=False)
        _ITEMS[name] = items
    return _ITEMS[name]


def batch(name):
    """The batch's items and its float64 reference: built once per process and shared; neither is modified."""
    return batch_items(name), pr.reference(batch_items(name), key=name)


# ---------------------------------------------------------------------------------------------------------------------
# drivers (shared with test_gpu_phong_ref.py)
# ---------------------------------------------------------------------------------------------------------------------

def run_cbrt(st):
    x = pr.cbrt_inputs()
    got = st.cbrt(x)
    fin = np.isfinite(x) & (x != 0)
    special = ~fin
    assert same_values(got[special], x[special])                  # +-0, +-inf and NaN pass through
    assert np.array_equal(np.signbit(got[special]), np.signbit(x[special]))
    ref = np.cbrt(x[fin].astype(np.float64))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got[fin].astype(np.float64) - ref) / ulp
    k = int(err.argmax())
    print("cbrt: %d values, worst error %.8f ulp at x = %r" % (x.size, err[k], float(x[fin][k])))
    assert err[k] <= 1.0
    cubes = np.arange(1, 257, dtype=np.float32)
    assert np.array_equal(st.cbrt(cubes ** 3), cubes) and np.array_equal(st.cbrt(-(cubes ** 3)), -cubes)


_CUBIC_REF = []


def cubic_reference():
    if not _CUBIC_REF:
        c = pr.cubic_batch()
        c.setflags(write=False)
        _CUBIC_REF.append((c, [pr.cubic_real_roots(row) for row in c]))
    return _CUBIC_REF[0]


def run_cubic(st, k_bound):
    c, refs = cubic_reference()
    out = st.solve_cubic(c)
    assert same_values(out, st.solve_cubic(c))                    # deterministic
    count = out[:, 0]
    cubic, quad = c[:, 0] != 0, (c[:, 0] == 0) & (c[:, 1] != 0)
    linear = (c[:, 0] == 0) & (c[:, 1] == 0) & (c[:, 2] != 0)
    none = ~(cubic | quad | linear)
    # hard, every case: the count is one the branch taken can return, the slots beyond it are 0
    assert np.isin(count[cubic], [1, 3]).all() and np.isin(count[quad], [0, 2]).all()
    assert (count[linear] == 1).all() and (count[none] == 0).all()
    for k in range(3):
        assert not out[count <= k, 1 + k].any()
    ambiguous, worst, ratios = 0, (0.0, -1), []
    for i, (roots, cond, expected, margin) in enumerate(refs):
        if margin < pr.COUNT_MARGIN:
            ambiguous += 1
            continue
        n = int(count[i])
        assert n == expected, (i, c[i].tolist(), n, expected, roots.tolist())
        got = out[i, 1: 1 + n].astype(np.float64)
        if n == 3:
            assert got[0] <= got[1] <= got[2], (i, got.tolist())
        bound = pr.EPS32 * (cond + np.abs(roots)) + 2.0 ** -149
        for g in got:
            ratio = float(np.min(np.abs(g - roots) / bound))
            ratios.append(ratio)
            if not ratio <= worst[0]:
                worst = (ratio, i)
    print("solveCubic: %d of %d counts ambiguous; worst |root - true| / ( 2^-23 ( cond + |r| ) ) = %.4g (case %d: %s), median %.3g; bound %g"
          % (ambiguous, len(refs), worst[0], worst[1], c[worst[1]].tolist(), float(np.median(ratios)), k_bound))
    assert ambiguous <= 0.15 * len(refs)
    assert worst[0] <= k_bound, worst


def angle(a, b):
    """Angle between unit-ish vectors, accurate near 0."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


def hard_invariants(items, out, allow_nan_t=False):
    """Every case, no exclusions: t is +inf or finite inside [ |tNear|, min( rayT, tFar ) ]; never NaN; the normal is 0
    exactly when t is inf."""
    t = out[:, 0]
    lo, hi = np.abs(items[:, 25]), np.minimum(items[:, 24], items[:, 26])
    finite = np.isfinite(t)
    miss = np.isinf(t) & (t > 0)
    if allow_nan_t:
        miss = miss | np.isnan(t)
    else:
        assert not np.isnan(t).any(), "t is NaN at %s" % np.flatnonzero(np.isnan(t))[:8]
    inside = finite & (t >= lo) & (t <= hi)
    bad = ~(miss | inside)
    assert not bad.any(), "t outside its interval at %s: %s" % (np.flatnonzero(bad)[:8], out[bad][:4])
    zero = ~out[:, 1:4].any(axis=1)                              # (a NaN component is not zero)
    assert np.array_equal(zero, ~finite), np.flatnonzero(zero == finite)[:8]


def compare_batch(name, items, ref, out):
    """The figures of one batch against its float64 reference."""
    t = out[:, 0].astype(np.float64)
    normal = out[:, 1:4].astype(np.float64)
    clear = ~ref["amb"]
    hit = np.isfinite(t)
    wrong_kind = clear & (hit != ref["hit"])
    both = clear & hit & ref["hit"]
    rel = np.abs(t[both] - ref["t"][both]) / np.maximum(1.0, ref["t"][both])
    fails = int(wrong_kind.sum()) + int((rel > T_TOL).sum())
    sel = both & (ref["ns_dot"] > pr.NS_TOL)
    sel[both] &= rel <= T_TOL                                     # the normal AT the reference's hit, not at another one
    ang = angle(normal[sel], ref["normal"][sel])
    length = np.abs(np.linalg.norm(normal[sel], axis=1) - 1.0)
    fig = dict(ambiguous=float(ref["amb"].mean()), fail_share=fails / max(1, int(clear.sum())), wrong_kind=int(wrong_kind.sum()),
               extra_hits=int((clear & hit & ~ref["hit"]).sum()), far_t=int((rel > T_TOL).sum()),
               median_t=float(np.median(rel)) if rel.size else 0.0, max_t=float(rel.max()) if rel.size else 0.0,
               max_angle=float(ang.max()) if ang.size else 0.0, median_angle=float(np.median(ang)) if ang.size else 0.0,
               max_length=float(length.max()) if length.size else 0.0, hits=int(ref["hit"].sum()), normals=int(sel.sum()))
    print("%-11s hits %d, ambiguous %.2f %%, failures %.3f %% (%d hit / miss [%d hits the reference lacks], %d beyond 1e-3), "
          "rel t median %.3g max %.3g, angle of %d normals median %.3g max %.3g, | |n| - 1 | max %.2g"
          % (name, fig["hits"], 100 * fig["ambiguous"], 100 * fig["fail_share"], fig["wrong_kind"], fig["extra_hits"], fig["far_t"],
             fig["median_t"], fig["max_t"], fig["normals"], fig["median_angle"], fig["max_angle"], fig["max_length"]))
    return fig


def run_patch_batch(st, name):
    items, ref = batch(name)
    out = st.phong_face(items)
    hard_invariants(items, out)
    fig = compare_batch(name, items, ref, out)
    assert fig["hits"] > 1000
    if name != "interval":                                         # (its boundaries sit next to the hits by construction)
        assert fig["ambiguous"] <= AMBIGUOUS_MAX
    assert fig["fail_share"] <= FAIL_MAX
    assert fig["median_t"] <= MEDIAN_FACTOR * st.scale * MEDIAN_T[name]
    assert fig["normals"] > 200
    assert fig["max_length"] <= 1e-5 * st.scale
    assert fig["max_angle"] <= ANGLE_MAX
    assert fig["median_angle"] <= MEDIAN_FACTOR * st.scale * MEDIAN_ANGLE[name]
    return fig


def run_recorded_batch(st, name):
    """Nearly flat patches and rays through the origin: what the reference's formulas give is recorded (module docstring);
    asserted are determinism and that t is never a finite value outside its interval."""
    items, ref = batch(name)
    out = st.phong_face(items)
    assert same_values(out, st.phong_face(items))
    hard_invariants(items, out, allow_nan_t=(name == "origin"))
    fig = compare_batch(name, items, ref, out)
    print("%s: NaN in the outputs: %s" % (name, bool(np.isnan(out).any())))
    if name == "flat":
        spread = pr.nearly_flat_batch()[1]
        t = out[:, 0]
        for lo, hi in ((None, None), (-7, -6), (-6, -5), (-5, -4), (-4, -3), (-3, -2)):
            sel = (spread == 0) if lo is None else (spread >= 10.0 ** lo) & (spread < 10.0 ** hi)
            want = ref["hit"] & sel
            print("  normal spread %s: %d hits in float64, %.1f %% of them missed, %d hits the reference lacks"
                  % ("0" if lo is None else "1e%d ... 1e%d" % (lo, hi), int(want.sum()),
                     100.0 * float((np.isinf(t) & want).sum()) / max(1, int(want.sum())), int((np.isfinite(t) & sel & ~ref["hit"]).sum())))
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------------------------------------------------

def test_patch_point_is_the_definition_at_the_corners_and_flat_for_equal_normals():
    rng = np.random.default_rng(7)
    P = rng.uniform(-1, 1, (64, 3, 3))
    ng = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    N = ng[:, None, :] + 0.3 * rng.normal(size=(64, 3, 3))
    N /= np.linalg.norm(N, axis=2, keepdims=True)
    one, zero = np.ones(64), np.zeros(64)
    for k, (u, v) in enumerate(((one, zero), (zero, one), (zero, zero))):          # the patch interpolates its corners
        assert np.allclose(pr.patch_point(P, N, u, v, 0.6), P[:, k], atol=1e-14)
    u, v = rng.dirichlet([1, 1, 1], 64)[:, :2].T
    flat = np.repeat(ng[:, None, :], 3, axis=1)
    p = u[:, None] * P[:, 0] + v[:, None] * P[:, 1] + (1 - u - v)[:, None] * P[:, 2]
    assert np.allclose(pr.patch_point(P, flat, u, v, 1.0), p, atol=1e-14)         # equal normals: the flat triangle
    assert np.allclose(pr.patch_point(P, N, u, v, 0.0), p, atol=1e-14)            # alpha = 0 likewise
    # the two forms of the module agree, and the analytic derivatives are those of the definition
    a = np.full(64, 0.6)
    S, Su, Sv = pr._patch(P, N, a, u, v, derivs=True)
    assert np.allclose(S, pr.patch_point(P, N, u, v, a), atol=1e-14)
    h = 1e-6
    assert np.allclose(Su, (pr.patch_point(P, N, u + h, v, a) - pr.patch_point(P, N, u - h, v, a)) / (2 * h), atol=1e-8)
    assert np.allclose(Sv, (pr.patch_point(P, N, u, v + h, a) - pr.patch_point(P, N, u, v - h, a)) / (2 * h), atol=1e-8)


def test_patch_hits_finds_the_points_it_was_aimed_at():
    """Rays aimed at S( u0, v0 ) of a strongly curved patch: ( u0, v0, |S - o| ) is among the solutions."""
    rng = np.random.default_rng(8)
    items = pr.make_items(rng, 512, 0.6, 0.7)
    P, N, o, d, _, _, _, alpha = pr.split_items(items)
    uv = rng.dirichlet([1, 1, 1], 512)[:, :2]
    S = pr.patch_point(P, N, uv[:, 0], uv[:, 1], alpha)
    o = S - 4.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    sol, _ = pr.patch_hits(P, N, o, d, alpha)
    want = np.concatenate([uv, 4.0 / np.linalg.norm(d, axis=1, keepdims=True)], axis=1)
    with np.errstate(invalid="ignore"):
        gap = np.nanmin(np.abs(sol - want[:, None, :]).max(-1), axis=1)
    print("aimed rays: worst gap to the aimed-at solution %.3g" % gap.max())
    assert gap.max() <= 1e-7


def test_the_start_grid_is_dense_enough():
    """A 136-point grid changes no decision of the 21-point grid (an eighth of one batch here; every batch once against
    231 points, see phong_ref)."""
    items, ref = batch("curved")
    n = 512
    fine = pr.reference(items[:n], div=15)
    assert np.array_equal(fine["hit"], ref["hit"][:n]) and np.array_equal(fine["amb"], ref["amb"][:n])
    hit = ref["hit"][:n]
    assert np.allclose(fine["t"][hit], ref["t"][:n][hit], rtol=1e-9, atol=0)


def test_cubic_reference_on_known_polynomials():
    r, cond, expected, margin = pr.cubic_real_roots(np.float32([2, -12, 22, -12]))            # 2 ( x - 1 )( x - 2 )( x - 3 )
    assert expected == 3 and np.allclose(r, [1, 2, 3], atol=1e-13) and margin > pr.COUNT_MARGIN
    assert np.allclose(cond, [12, 60, 60])                                                   # sum |a_i| |r|^(3-i) = 48, 120, 240 over |p'( r )| = 4, 2, 4
    r, _, expected, _ = pr.cubic_real_roots(np.float32([1, 0, 1, 0]))                        # x ( x^2 + 1 )
    assert expected == 1 and np.allclose(r, [0])
    r, _, expected, margin = pr.cubic_real_roots(np.float32([1, -3, 3, -1]))                 # ( x - 1 )^3
    assert margin < pr.COUNT_MARGIN
    assert pr.cubic_real_roots(np.float32([0, 1, 0, 1]))[2] == 0 and pr.cubic_real_roots(np.float32([0, 1, 0, -4]))[2] == 2
    assert pr.cubic_real_roots(np.float32([0, 0, 2, 1]))[2] == 1 and pr.cubic_real_roots(np.float32([0, 0, 0, 1]))[2] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------

def test_cbrt_within_one_ulp_of_float64(stages):
    run_cbrt(stages)


def test_solve_cubic_against_float64_roots(stages):
    run_cubic(stages, K_CUBIC)


@pytest.mark.parametrize("name", ["random 0.3", "random 0.6", "random 1.0", "curved", "axis", "tnear", "interval"])
def test_patch_intersection_against_float64(stages, name):
    run_patch_batch(stages, name)


@pytest.mark.parametrize("name", ["flat", "origin"])
def test_nearly_flat_patches_and_rays_through_the_origin_are_recorded(stages, name):
    run_recorded_batch(stages, name)


def test_negative_tnear_drops_the_hits_nearer_than_its_magnitude(stages):
    """The reference's quirk (pt_phongtess.cl:202), kept: with tNear = -a a hit at t < a is dropped, the same item with
    tNear = 0 finds it."""
    items, ref = batch("tnear")
    free = np.array(items)
    free[:, 25] = 0.0
    got, unclipped = stages.phong_face(items), stages.phong_face(free)
    dropped = np.isfinite(unclipped[:, 0]) & (unclipped[:, 0] < np.abs(items[:, 25]))
    assert dropped.sum() > 500
    assert (got[dropped, 0] > unclipped[dropped, 0]).all()        # a farther solution of the same patch, or inf
