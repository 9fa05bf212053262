"""Steps 0 to 4 of pbr_denoise_temporal on planted histories, without a device: the fp32 restatements (temporal_ref.integrate,
temporal_motion_ref.integrate) against the float64 truth (temporal_planes.integrate_truth64) on every case of
temporal_planes.cases().

DECISIONS first: on every pixel of every case the two take the same ones — a candidate or why none, per tap used or the rule
that left it out, the tap Hl came from, blend or the rule that made a copy, L, the motion code.  No pixel is excused.  Every
threshold a case plants on both sides (`pairs`) is accepted on the one and rejected on the other, by both.

VALUES then: E_ref, the restatement's distance from the truth, stays under a bound made of the definition alone — the binary32
roundings on the value's path times the ulp of the path's largest intermediate (derived at `bounds` below).  Measured in
every run; the table is a record of one (x86-64 numpy), the largest value per class, in brackets as a share of its bound:

  class          fx / fy            I.rgb              I.w                Pprev              nref               len
  1 sizes        8.692e-06 (0.04)   2.691e-06 (0.03)   5.655e-08 (0.00)   5.495e-07 (0.05)   1.561e-07 (0.08)   3.401e-07 (0.06)
  2 candidates   4.639e-07 (0.03)   2.644e-07 (0.00)   2.994e-09 (0.00)   -                  -                  -
  3 tap tests    0         (0.00)   7.417e-08 (0.00)   1.129e-09 (0.00)   -                  -                  -
  4 blend        0         (0.00)   1.572e+31 (0.00)   8.790e+30 (0.00)   -                  -                  -
  5 miss pixels  7.825e-06 (0.04)   2.691e-06 (0.00)   5.655e-08 (0.00)   -                  -                  -
  6 motion       8.692e-06 (0.00)   1.479e-07 (0.03)   3.579e-09 (0.00)   5.495e-07 (0.05)   1.561e-07 (0.08)   3.401e-07 (0.06)
(fx / fy in pixels.  Classes 3 and 4 plant dyadic candidates: exact.  Class 4's colours and variances reach 3e38, where one
binary32 ulp is 2e31.  The candidate 8e30 pixels away of class 2 is exact too: the pixel's own coordinate is below half an ulp
of the eye's in either format.  Left out: 25 pixels of near_flt_max, where C - Hc overflows binary32 and the definition's value
does not — see temporal_planes.py.  On the overflowing face of the motion scene both sides give inf and NaN alike.)

MUTANTS last: twelve one-token variants of the restatements' source.  Each must differ from the restatement on a planted case,
or a case is missing.  `c >= 0` for `c > 0` differs in no value — c == 0 makes scale 0 and fx not finite either way — and
shows in the record alone: the pixel has no candidate for another reason."""
import collections
import inspect

import numpy as np
import pytest

import temporal_motion_ref as mref
import temporal_planes as T
import temporal_ref as ref
from conftest import same_values

CASES = [pytest.param(case, id=case.name) for case in T.cases()]
QUANTITIES = ("fx / fy", "I.rgb", "I.w", "Pprev", "nref", "len")
MEASURED = {}            # case name -> {quantity: (largest error, largest error / bound)}


def test_the_table_has_every_size_and_class():
    names = [c.name for c in T.cases()]
    assert len(set(names)) == len(names)
    assert set().union(*(c.classes for c in T.cases())) == set(T.CLASSES)
    assert {(c.w, c.h) for c in T.cases() if 1 in c.classes} == set(T.SIZES)
    assert {(c.w, c.h) for c in T.cases() if c.classes >= {1, 6}} == set(T.SIZES)          # both kernels at every size
    assert all(c.w * c.h <= 1024 for c in T.cases())
    for c in T.cases():
        if c.prev is not None:
            assert c.prev.lengths.min() >= 1 and c.prev.lengths.max() <= 1024
        if c.motion is not None:
            assert c.motion.face.min() >= -1 and c.motion.face.max() < len(c.motion.faces_v)
            assert c.motion.faces_v[:, :3].max() < len(c.motion.vertices) == len(c.motion.hist_vertices)


@pytest.mark.parametrize("case", CASES)
def test_restatement_and_truth_decide_alike(case):
    r = T.evaluate(case)
    for record in (r.rest_record, r.truth_record):
        assert (record.candidate != 255).all() and (record.tap != 255).all() and (record.copy != 255).all()
        assert ((record.source >= 0) == (record.tap == ref.USED).any(-1)).all()
    apart = ~r.rest_record.same_decisions(r.truth_record)
    assert not apart.any(), "%d pixels, the first %s" % (apart.sum(), np.argwhere(apart)[0])
    # the records are what the results say
    assert same_values(r.rest_record.valid(), r.rest.history[..., 3]) and same_values(r.truth_record.valid(), r.truth.valid)
    assert same_values(r.rest_record.length, r.rest.history[..., 2]) and same_values(r.truth_record.length, r.truth.length)
    assert same_values(r.rest_record.candidate == ref.CANDIDATE, np.isfinite(r.rest.history[..., 0]))
    if case.motion is not None:
        assert same_values(r.rest_record.code, r.rest.motion[..., 3]) and same_values(r.truth_record.code, r.truth.step0.motion[..., 3])
    for what, accepted, rejected, tap, rule in case.pairs:
        for record in (r.rest_record, r.truth_record):
            assert record.tap[accepted][tap] == ref.USED, what
            assert record.tap[rejected][tap] == rule, what


# ---- values ----------------------------------------------------------------------------------------------------------------------
#
# A binary32 operation's result is off by at most half an ulp of itself; a value's error is at most the sum, over the
# roundings in its expression tree, of what each contributes at the value's scale — which `roundings x ulp32( largest )`
# covers twice over when `largest` is the largest magnitude the tree reaches in the value's own units, with every cancellation
# undone (sums of absolute values in place of sums).  The trees, counted from csrc/pt_temporal.hpp:
#
#   fx, fy   d = P - eye' (1 per component, 3), dot( d, cu' ) (5), dot( cu', cu' ) (5), their quotient (1); the same 11 for c
#            (d is shared); scale (1), a / scale (1), + ( w - 1 ) (1); * 0.5 is exact: 3 + 11 + 11 + 3 = 28.  Largest: sum | d_k
#            cu'_k | / dot( cu', cu' ) / | scale |, times sum | d_k cw'_k | / | c dot( cw', cw' ) | for c's share, or w - 1
#            (temporal_planes: fx_largest).  On the motion path d starts from Pprev: its error E_P moves a and c by at most
#            3 max | cu'_k | / dot( cu', cu' ) E_P, and fx by ( da + | a / c | dc ) / ( 2 | scale | ) (fx_per_world).
#   Pprev    u: the corners' differences e1, e2, w (1 per component), five dot products (5 each), den and the numerator (3
#            each), the quotient (1) — as a tree with its repeats 86 roundings, relative to | u | with the cancellations of
#            the numerator and of den undone (u_size).  Then e1' (1), e1' * u (1), a' + (1), e2' (1), e2' * v (1), + (1):
#            86 ulp32( | e1' | u_size + | e2' | v_size ) + 6 ulp32( | a' | + | e1' | | u | + | e2' | | v | ).  An unmoved face: 0.
#   nref     per component two edge differences per factor (4), two products (2), one subtraction (1), the sign is exact:
#            8 ulp32( max | e1'_k | max | e2'_k | ) with the spare one.  An unmoved face: 0.
#   len      | d len | <= | d nref |_2 <= 2 E_nref; the dot product's 5 roundings are relative ones of len^2, so 2.5 of len,
#            and sqrtf 1: 2 E_nref + 4 ulp32( len ).
#   I.rgb    tx (1), 1 - tx (1), bw (1); per tap bw * I' (1) and the sum (1): 8; S (3); Hc (1); C - Hc (1), alpha (1), alpha *
#            (1), + (1): 19 ulp32( largest of | C |, | I' | over the used taps ).  The weights move with the candidate:
#            an error E_f in fx and fy moves each bw by at most 2 E_f and S by at most 8 E_f, so sum | d( bw / S ) | <= 16 E_f / S.
#   I.w      bw (3); per tap bw * bw (1), * I'.w (1) and the sum (1): 12; S (3), S * S (1), Hv (1); alpha (1), keep (1), keep *
#            keep (1), * Hv (1), alpha * alpha (1), * V (1), + (1): 29, taken as 32, ulp32( largest of | V |, | I'.w | );
#            sum | d( bw^2 / S^2 ) | <= 32 E_f / S.
#   A copy ( L = 1 ) is {C, V} bit for bit: 0.

def bounds(case, truth):
    """-> dict quantity -> (h, w) float64 bound, from the truth's magnitudes alone."""
    h, w = case.h, case.w
    out = {}
    e_p = np.zeros((h, w))
    if case.motion is not None:
        s = truth.step0
        size = lambda x: np.abs(x).max(-1)
        with np.errstate(all="ignore"):
            e_p = 86 * T.ulp32(size(s.e1p) * s.u_size + size(s.e2p) * s.v_size) \
                + 6 * T.ulp32(size(s.a2) + size(s.e1p) * np.abs(s.u) + size(s.e2p) * np.abs(s.v))
            e_n = 8 * T.ulp32(size(s.e1p) * size(s.e2p))
        e_p, e_n = np.where(s.unmoved, 0.0, e_p), np.where(s.unmoved, 0.0, e_n)
        out["Pprev"], out["nref"] = e_p, e_n
        out["len"] = np.where(s.unmoved, 0.0, 2 * e_n + 4 * T.ulp32(s.reference[..., 3]))
    if case.prev is None:
        zero = np.zeros((h, w))
        out.update({"fx / fy": zero, "I.rgb": zero, "I.w": zero})
        return out
    with np.errstate(all="ignore"):
        e_f = 28 * T.ulp32(truth.fx_largest) + 3 * truth.fx_per_world * np.where(np.isfinite(e_p), e_p, 0.0)
        moved = 16 * e_f / np.where(truth.blend, truth.weight, 1.0)
        out["fx / fy"] = e_f
        out["I.rgb"] = np.where(truth.blend, 19 * T.ulp32(truth.largest[..., :3].max(-1)) + moved * truth.largest[..., :3].max(-1), 0.0)
        out["I.w"] = np.where(truth.blend, 32 * T.ulp32(truth.largest[..., 3]) + 2 * moved * truth.largest[..., 3], 0.0)
    return out


def errors(case, got, truth):
    """got: a namespace integrated / history / motion / reference (the restatement's, or the device's) -> (dict quantity ->
    (h, w) float64 distance from the truth, NaN where it does not apply; (h, w) bool `apart`: one side finite, the other not)."""
    h, w = case.h, case.w
    with np.errstate(all="ignore"):
        pairs = {"fx / fy": (got.history[..., :2], np.stack([truth.fx, truth.fy], -1)), "I.rgb": (got.integrated[..., :3], truth.integrated[..., :3]),
                 "I.w": (got.integrated[..., 3:], truth.integrated[..., 3:])}
        if case.motion is not None:
            hit = (case.motion.face >= 0)[..., None]
            pairs["Pprev"] = (np.where(hit, got.motion[..., :3], 0), np.where(hit, truth.step0.motion[..., :3], 0))
            pairs["nref"] = (np.where(hit, got.reference[..., :3], 0), np.where(hit, truth.step0.reference[..., :3], 0))
            pairs["len"] = (np.where(hit, got.reference[..., 3:], 0), np.where(hit, truth.step0.reference[..., 3:], 0))
        out, apart = {}, np.zeros((h, w), bool)
        for what, (a, b) in pairs.items():
            a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
            b32 = b.astype(np.float32).astype(np.float64)                             # what the truth is as a binary32 quantity
            both = np.isfinite(a) & np.isfinite(b32)
            same = both | (np.isnan(a) & np.isnan(b32)) | (~np.isfinite(a) & (a == b32))
            apart |= ~same.all(-1)
            out[what] = np.where(both, np.abs(a - b), np.where(same, 0.0, np.nan)).max(-1)
    return out, apart


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_stays_within_the_definition_s_roundings_of_the_truth(case):
    r = T.evaluate(case)
    error, apart = errors(case, r.rest, r.truth)
    bound = bounds(case, r.truth)
    assert not (apart & ~case.may_overflow).any(), np.argwhere(apart & ~case.may_overflow)[:4]
    MEASURED[case.name] = {}
    for what, e in error.items():
        use = ~np.isnan(e) & ~apart & np.isfinite(bound[what])
        over = use & (e > bound[what])
        assert not over.any(), "%s: %s at %s is %.3e, bound %.3e" % (case.name, what, np.argwhere(over)[0], e[over][0], bound[what][over][0])
        with np.errstate(all="ignore"):
            share = np.where(use & (e > 0), e / bound[what], 0.0)
        MEASURED[case.name][what] = (float(np.where(use, e, 0.0).max()), float(share.max()), int(apart.sum()))
    # a copy is a copy
    given = np.concatenate([case.image[..., :3], case.variance[..., None]], -1)
    copied = r.truth_record.copy != ref.BLENDED
    assert same_values(r.rest.integrated[copied], given[copied]) and (r.truth.length[copied] == 1).all()
    if case.motion is not None:
        still = r.truth_record.code == 1
        assert same_values(r.rest.motion[still][:, :3], case.features[0][still][:, :3]) and (r.rest.reference[still][:, 3] == 1).all()
        assert same_values(r.rest.reference[still][:, :3], case.features[1][still][:, :3])


def test_measured_errors_per_class():
    """The docstring's table.  Runs after the cases above; alone it measures them itself."""
    for case in T.cases():
        if case.name not in MEASURED:
            test_the_restatement_stays_within_the_definition_s_roundings_of_the_truth(case)
    print("\n  class          " + "".join("%-19s" % q for q in QUANTITIES))
    for number, what in sorted(T.CLASSES.items()):
        row = "  %d %-13s" % (number, what)
        for q in QUANTITIES:
            cells = [MEASURED[c.name][q] for c in T.cases() if number in c.classes and q in MEASURED[c.name]]
            row += "%-19s" % (("%-9.3e (%.2f)" % (max(c[0] for c in cells), max(c[1] for c in cells))) if cells else "-")
        print(row)
    print("  left out (an intermediate overflows binary32 only): %s" % {c.name: MEASURED[c.name]["I.rgb"][2] for c in T.cases() if MEASURED[c.name]["I.rgb"][2]})


# ---- the class table ----------------------------------------------------------------------------------------------------------------

def decision_counts(case, record, history):
    """Counter of the decisions of one call: what the class table below and tests/test_gpu_temporal_planes.py's count print."""
    c = collections.Counter()
    for code, name in ref.CANDIDATES.items():
        c["candidate: " + name] += int((record.candidate == code).sum())
    for code, name in ref.REASONS.items():
        c["tap: " + name] += int((record.tap == code).sum())
    for code, name in ref.COPIES.items():
        c["blend: " + name] += int((record.copy == code).sum())
    for mask in range(16):
        c["valid mask %d" % mask] += int(((history[..., 3] == mask) & (record.candidate == ref.CANDIDATE)).sum())
    used = record.tap == ref.USED
    x0, y0 = np.floor(history[..., 0]), np.floor(history[..., 1])
    c["x0 == -1"], c["x0 == w - 1"] = int((x0 == -1).sum()), int((x0 == case.w - 1).sum())
    c["y0 == -1"], c["y0 == h - 1"] = int((y0 == -1).sum()), int((y0 == case.h - 1).sum())
    c["Hl from a tap other than 0"] = int((record.source > 0).sum())
    c["L == max_history"] = int(((record.copy == ref.BLENDED) & (record.length == case.params.max_history)).sum())
    c["L < max_history"] = int(((record.copy == ref.BLENDED) & (record.length < case.params.max_history)).sum())
    c["more than one tap used"] = int((used.sum(-1) > 1).sum())
    if record.code is not None:
        for code in (0, 1, 2, 3):
            c["motion code %d" % code] += int((record.code == code).sum())
    return c


def class_counts(number):
    total = collections.Counter()
    for case in T.cases():
        if number in case.classes:
            r = T.evaluate(case)
            total.update(decision_counts(case, r.truth_record, np.stack([r.truth.fx, r.truth.fy, r.truth.length, r.truth.valid], -1)))   # keeps a 0
    return total


def test_every_class_reaches_its_decisions():
    counts = {number: class_counts(number) for number in T.CLASSES}
    keys = sorted(set().union(*counts.values()))
    print("\n%-36s" % "decision (pixels or taps, truth)" + "".join("%14s" % T.CLASSES[n] for n in sorted(counts)))
    for key in keys:
        print("%-36s" % key + "".join("%14d" % counts[n][key] for n in sorted(counts)))
    need = {
        1: ["x0 == -1", "x0 == w - 1", "y0 == -1", "y0 == h - 1", "tap: outside the image", "valid mask 15", "motion code 1", "motion code 2"],
        2: ["valid mask 1", "valid mask 3", "valid mask 5", "valid mask 15", "x0 == -1", "x0 == w - 1", "y0 == -1", "y0 == h - 1",
            "candidate: !( c > 0 )", "candidate: fx or fy not finite", "tap: !( bw > 0 )", "tap: outside the image", "blend: !( S > 0 )",
            "blend: no previous call", "Hl from a tap other than 0", "tap: !( distance <= r * r )"],
        3: ["tap: N'.w != N.w", "tap: A'.w != A.w", "tap: !( dot >= normal_cos )", "tap: !( distance <= r * r )", "tap: I' not finite"],
        4: ["blend: max_history == 1", "blend: C or V not finite", "L == max_history", "L < max_history", "Hl from a tap other than 0",
            "valid mask 8"],
        5: ["tap: N'.w != N.w", "blend: blended", "blend: !( S > 0 )"],
        6: ["motion code 0", "motion code 1", "motion code 2", "motion code 3", "candidate: motion code 3", "tap: !( dot >= normal_cos )",
            "tap: !( distance <= r * r )", "blend: blended"],
    }
    for number, keys in need.items():
        for key in keys:
            assert counts[number][key] > 0, "class %d (%s) never reaches %r" % (number, T.CLASSES[number], key)
    # what the classes say they plant, by name
    by_name = {c.name: c for c in T.cases()}
    whole = T.evaluate(by_name["shift_whole_image"]).truth_record
    assert (whole.candidate == ref.CANDIDATE).all() and (whole.tap == ref.OUTSIDE).all()
    far = T.evaluate(by_name["eye_1e30"])
    assert (far.truth_record.candidate == ref.CANDIDATE).all() and np.abs(far.rest.history[..., 0]).min() > 1e30
    tiny = T.evaluate(by_name["c_subnormal"]).truth_record
    assert (tiny.candidate == ref.OFF_SCALE).sum() == T.W * T.H - 1 and (tiny.candidate == ref.CANDIDATE).sum() == 1
    assert (T.evaluate(by_name["c_zero"]).truth_record.candidate == ref.BEHIND).all()
    sky = T.evaluate(by_name["sky_to_sky_rotated"])
    assert (sky.truth_record.copy == ref.BLENDED).sum() > 20 and not np.isin(sky.rest.history[..., 3], (0, 1)).all()
    ties = T.evaluate(by_name["shift_hxy"])
    inner = ties.rest.history[..., 3] == 15
    assert inner.sum() == (T.W - 1) * (T.H - 1) and (ties.rest_record.source[inner] == 0).all()          # four equal bw: the first
    edge = T.evaluate(by_name["motion_all_faces"])
    face = by_name["motion_all_faces"].motion.face
    assert set(np.unique(face)) == set(range(-1, T.MOTION_FACES))
    assert (edge.rest.reference[face == 8][:, 3] == 0).all() and (edge.rest_record.code[np.isin(face, (7, 9))] == 3).all()
    assert (edge.rest.reference[face == 5][:, 2] < 0).all() and (edge.rest.reference[face == 1][:, 2] > 0).all()
    small = T.evaluate(by_name["weights_to_2^-22"]).rest
    assert (small.history[..., 3] == 8).sum() == 4 and same_values(small.history[0, 0, :2], np.float32([2.0 ** -11, 2.0 ** -11]))


def test_a_step_beyond_r_that_rounds_back_is_accepted():
    """Why `pairs` are verified and not assumed: r * r = 9 / 64 has an ulp of 2^-26.  A tap 2^-14 further out lies at r * r + 2^-28
    in the reals — beyond — and at r * r in binary32, which is what the definition asks: accepted.  2^-13 gives the next float."""
    case = next(c for c in T.cases() if c.name == "distance_r")
    position = [f.copy() for f in case.prev.features]
    position[0][1::2, ::2, 1] = case.features[0][1::2, ::2, 1] + np.float32(2.0 ** -14)
    prev = ref.previous(case.prev.integrated, tuple(position), case.prev.lengths, case.prev.cam, case.prev.px_dim)
    record = ref.Record(case.h, case.w)
    ref.integrate(case.image, case.variance, tuple(case.features), case.cam, case.px_dim, prev, case.params, record=record)
    assert record.tap[1, 0, 0] == ref.USED and T.evaluate(case).rest_record.tap[1, 0, 0] == ref.DISTANCE


# ---- a wrong restatement is noticed ----------------------------------------------------------------------------------------------

def mutant(function, replacements, caller=None):
    """A copy of a restatement with pieces of its source replaced; caller: the function of the same module to return in its
    place, bound to the copy."""
    source = inspect.getsource(function)
    for old, new in replacements:
        assert source.count(old) == 1, old
        source = source.replace(old, new)
    namespace = dict(vars(inspect.getmodule(function)))
    exec(compile(source, "<mutant of %s>" % function.__name__, "exec"), namespace)
    if caller is not None:
        exec(compile(inspect.getsource(caller), "<caller of a mutant>", "exec"), namespace)
    return namespace[(caller or function).__name__]


MUTANTS = {
    # the function, what is replaced by what, the function handed back
    ">= -> > on the normal test": (ref.integrate, [("albedo[..., 3]) & (dot(n, normal) >= F(params.normal_cos))",
                                                    "albedo[..., 3]) & (dot(n, normal) > F(params.normal_cos))")], None),
    "<= -> < on the distance test": (ref.integrate, [("on_surface &= sqdist(p, position) <= radius2", "on_surface &= sqdist(p, position) < radius2")], None),
    "bw > 0 -> bw >= 0": (ref.integrate, [("ok = has & inside & (bw > 0)", "ok = has & inside & (bw >= 0)")], None),
    "inside against w, not w - 1": (ref.integrate, [("(txf <= F(w - 1))", "(txf <= F(w))"),
                                                    ("xi = np.where(ok, txf, 0).astype(np.int64)", "xi = np.minimum(np.where(ok, txf, 0).astype(np.int64), w - 1)")], None),
    "the last of equals for Hl": (ref.integrate, [("better = ok & (bw > best)", "better = ok & (bw >= best)")], None),
    "Hl, not Hl + 1": (ref.integrate, [("np.minimum(length + 1, int(params.max_history))", "np.minimum(length, int(params.max_history))")], None),
    "S, not S * S, under Hv": (ref.integrate, [("hv = vsum / (wsum * wsum)", "hv = vsum / wsum")], None),
    ".w left out of the finite test": (ref.integrate, [("ok &= np.isfinite(old).all(-1)", "ok &= np.isfinite(old[..., :3]).all(-1)")], None),
    "c >= 0": (ref.candidate, [("ok = (c > 0) & np.isfinite(fx)", "ok = (c >= 0) & np.isfinite(fx)"),
                               ("record.set_candidate(c > 0,", "record.set_candidate(c >= 0,")], ref.integrate),
    "the flip test on n', not n": (mref.motion, [("(ref.dot(N, n) < 0)[..., None]", "(ref.dot(N, n2) < 0)[..., None]")], mref.integrate),
    "normal_cos not scaled by len": (mref.integrate, [("bound = F(params.normal_cos) * reference[..., 3]",
                                                       "bound = F(params.normal_cos) * np.ones_like(reference[..., 3])")], None),
    "r from Pprev's .w": (mref.integrate, [("radius = (F(params.sigma_world) * F(px_dim)) * position[..., 3]",
                                            "radius = (F(params.sigma_world) * F(px_dim)) * moved[..., 3]")], None),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_wrong_restatement_differs_on_a_planted_case(name):
    function, replacements, caller = MUTANTS[name]
    wrong = mutant(function, replacements, caller)
    moving = inspect.getmodule(function) is mref
    noticed, by_record = [], []
    for case in T.cases():
        if (case.motion is not None) != moving or case.prev is None:
            continue
        r = T.evaluate(case)
        record = ref.Record(case.h, case.w)
        got = T.restatement(case, record, **({"moving": wrong} if moving else {"static": wrong}))
        values = all(same_values(getattr(got, k), getattr(r.rest, k)) for k in ("integrated", "history") + (("motion", "reference") if moving else ()))
        noticed.append(case.name if not values else None)
        by_record.append(case.name if not record.same_decisions(r.rest_record).all() else None)
    hits, record_hits = [n for n in noticed if n], [n for n in by_record if n]
    print("%s: values differ in %d of %d cases (%s), the record in %d" % (name, len(hits), len(noticed), ", ".join(hits[:4]), len(record_hits)))
    if name == "c >= 0":
        assert not hits and "c_zero" in record_hits       # equivalent in every value, see the module's docstring
    else:
        assert hits
