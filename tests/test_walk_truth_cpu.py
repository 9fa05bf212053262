"""What tests/test_gpu_walk_truth.py assumes, established without a GPU, so that a failure there is the device's and not the
method's (tests/walk_truth.py): the cases are the trees they are there for; their cameras and lights leave enough decided
pixels, hits, shadowed and lit pixels at the native margin; the oracle alone, in the reference walk and in eight orders, breaks
neither probe on a single decided pixel; and each of three planted tree defects — the kind the probes are there to see —
is caught against the truth of the unplanted geometry.

64 x 48, two frames.  The margins are input conditions: EDGE_MARGIN for the exact arithmetic, NATIVE_SCALE * EDGE_MARGIN for
the native one (the rule of tests/test_gpu_shading_ref.py over the barycentric margin of tests/hand_scenes.py)."""
import numpy as np
import pytest

import hand_scenes
import refit_ref
import walk_truth as wt
from hand_scenes import EDGE_MARGIN
from test_gpu_shading_ref import K_NATIVE, NATIVE_SCALE

NATIVE_MARGIN = NATIVE_SCALE * EDGE_MARGIN
MARGINS = {0: EDGE_MARGIN, 1: NATIVE_MARGIN}              # by pbr_config.arith
PLANTED_ON = ("wide40", "sponza-6k")
# where the unplanted truth foresees no pixel that a defect must change, no probe can catch it: plant() refuses, and another
# hand-made tree stands in.  wide40 has no container below node 1 — both of its containers end the array, so no miss link
# there can be copied onto a first child and change it — and none of its 3072 centre rays passes a leaf's box by when that
# is pulled in by 2 %
STAND_IN = {("wide40", "skipped_subtree"): "cut257", ("wide40", "shrunk_box"): "cut257"}
LEAK_LIGHT = (-6.3, 2.667, 1.571)      # sponza-6k: behind the end wall at x = -6, whose faces are second faces of their leaves


def oracle_image(oracle, sc, cfg):
    r = oracle.Renderer(sc.desc, cfg, threads=8)
    return r.render(0, sc.seeds, sc.px, sc.cam), r.counter_dict()


def assert_probe_a(image, first, mask, what):
    got = wt.probe_a(image, first, mask)
    assert got["outliers"].size == 0, (what, "t", wt.describe(first, image, got["outliers"]))
    assert got["colour"].size == 0, (what, "rgb", wt.describe(first, image, got["colour"]))
    return got["worst"]


def assert_probe_b(image, first, black, lit, what):
    got = wt.probe_b(image, black, lit)
    assert got["leaks"].size == 0, (what, "light on the black set", wt.describe(first, image, got["leaks"]))
    assert got["dark"].size == 0, (what, "no light on the lit set", wt.describe(first, image, got["dark"]))


@pytest.mark.parametrize("name", wt.CASES)
def test_cases_are_what_they_are_there_for(pbr, name):
    sc = wt.case(pbr, name)
    a = sc.arrays
    assert pbr.validate_scene(sc.desc) == ""
    assert a["lights"].shape == (1, 12) and a["lights"][0, 8] == 1 and (a["lights"][0, 4:7] > 0).all()
    assert a["materials"].shape[0] == 1 and not a["facesV"][:, 3].any() and sc.cam.focusPoint[0] < 0
    for brdf in wt.BRDFS[name]:
        m = wt.case(pbr, name, brdf).arrays["materials"][0]
        assert m[0] == 1 and (max(m[2], m[3]) < 50 if brdf == 1 else m[3] == 1)        # d = 1, never extends a path
    bvh = a["bvh"]
    leaf, face0, face1, end, parent = refit_ref.tree_tables(bvh)
    extent = bvh[:, 4:7] - bvh[:, 0:3]
    if name in ("wide7", "wide40"):
        assert len(list(refit_ref.children(1, end))) == int(name[4:]) == leaf.sum()
    if name == "chain300":
        assert int(refit_ref.heights(leaf, parent)[0]) == 301 and (bvh[:, [0, 1, 2, 4, 5, 6]] == bvh[0, [0, 1, 2, 4, 5, 6]]).all()
    if name == "cut257":
        assert bvh.shape[0] == 257
    if name == "cornell":
        assert (extent[leaf] == 0).any(axis=1).sum() >= 6                                # walls: boxes without extent on an axis
    if name == "sponza-6k":
        assert a["facesV"].shape[0] >= 6000 and (face1[leaf] >= 0).sum() > 1000          # leaf pairs
        assert (bvh[~leaf, 7] - np.flatnonzero(~leaf) > 1000).any()                      # long miss links


@pytest.mark.parametrize("name", wt.CASES)
def test_cameras_and_lights_hold_the_input_conditions(pbr, name):
    """At the native margin, per case and BRDF: >= 85 % of the pixels decided, 15 - 95 % hit, and among the decided hit pixels
    >= 10 % in the black set (shadowed) and >= 10 % in the lit set.  The exact margin is the smaller one: its sets contain these."""
    for brdf in wt.BRDFS[name]:
        sc, first, shadow, gate = wt.truth(pbr, name, brdf, K_NATIVE)
        mask, black, lit = wt.sets(first, shadow, gate, NATIVE_MARGIN)
        hits = mask & first["hit"]
        print("%s, BRDF %d: %.1f %% decided, %.1f %% hit; of %d decided hits %d shadowed, %d lit" % (
            name, brdf, 100 * mask.mean(), 100 * first["hit"].mean(), hits.sum(), (black & hits).sum(), lit.sum()))
        assert mask.mean() >= 0.85 and 0.15 <= first["hit"].mean() <= 0.95
        assert (black & hits).sum() >= 0.10 * hits.sum() and lit.sum() >= 0.10 * hits.sum()
        assert not (black & lit).any() and not (lit & ~hits).any()
        wider = wt.sets(first, shadow, gate, EDGE_MARGIN)
        assert all((inner <= outer).all() for inner, outer in zip((mask, black, lit), wider))


@pytest.mark.parametrize("name", wt.CASES)
def test_the_oracle_alone_stays_within_the_rules(pbr, oracle, name):
    """oracle.Renderer in the exact arithmetic, the reference walk and eight orders: probe A has no outlier and no colour off
    on the decided pixels at EDGE_MARGIN, probe B no light on the black set and light on every lit-set pixel — zero exceptions.
    The point light is nothing to configuration A (no shadow rays; traverseLights only meets orbs): the image without it is the
    same bits."""
    for brdf in wt.BRDFS[name]:
        sc, first, shadow, gate = wt.truth(pbr, name, brdf, K_NATIVE)
        mask, black, lit = wt.sets(first, shadow, gate, EDGE_MARGIN)
        for traversal in (0, 2):
            what = (name, brdf, traversal)
            image, counters = oracle_image(oracle, sc, wt.config_a(sc, brdf, traversal=traversal))
            worst = assert_probe_a(image, first, mask, what)
            finite = np.isfinite(image[..., 3])
            assert (finite | np.isposinf(image[..., 3])).all()
            assert counters["paths"] == wt.W * wt.H * wt.FRAMES and counters["hits"] == finite.sum() * wt.FRAMES
            image_b, _ = oracle_image(oracle, sc, wt.config_b(sc, brdf, traversal=traversal))
            assert_probe_b(image_b, first, black, lit, what)
            print("%s, BRDF %d, traversal %d: largest |w - t64| / max( 1, t64 ) = %.3g; %d pixels of B not finite" % (
                name, brdf, traversal, worst, (~np.isfinite(image_b[..., :3]).all(axis=2)).sum()))
        dark = hand_scenes.with_arrays(sc, lights=np.zeros((0, 12), np.float32))
        assert np.array_equal(oracle_image(oracle, dark, wt.config_a(sc, brdf))[0], oracle_image(oracle, sc, wt.config_a(sc, brdf))[0], equal_nan=True)


# ---- teeth --------------------------------------------------------------------------------------------------------------

def planted(pbr, name, defect, among=None):
    sc, first, shadow, gate = wt.truth(pbr, name, 1, K_NATIVE)
    mask = wt.decided(first["edge"], first["cosine"], EDGE_MARGIN)
    return wt.plant(sc, defect, first, mask, among)


@pytest.mark.parametrize("defect", wt.DEFECTS)
@pytest.mark.parametrize("name", PLANTED_ON)
def test_probe_a_catches_a_planted_defect(pbr, oracle, name, defect):
    """The oracle renders the planted tree; against the truth of the UNPLANTED geometry probe A reports an outlier or a colour
    off, in the reference walk and in eight orders, among them the pixels plant() chose the place for (STAND_IN: where it
    finds none)."""
    if (name, defect) in STAND_IN:
        with pytest.raises(ValueError):
            planted(pbr, name, defect)
        name = STAND_IN[(name, defect)]
    sc, first, shadow, gate = wt.truth(pbr, name, 1, K_NATIVE)
    mask = wt.decided(first["edge"], first["cosine"], EDGE_MARGIN)
    bad, what = planted(pbr, name, defect)
    assert pbr.validate_scene(bad.desc) == "" and what["pixels"].size >= 1
    assert not np.array_equal(bad.arrays["bvh"], sc.arrays["bvh"], equal_nan=True)
    for traversal in (0, 2):
        image, _ = oracle_image(oracle, bad, wt.config_a(sc, 1, traversal=traversal))
        got = wt.probe_a(image, first, mask)
        caught = np.union1d(got["outliers"], got["colour"])
        print("%s, %s at node %d, traversal %d: %d pixels caught, %d of the %d foreseen" % (
            name, defect, what["node"], traversal, caught.size, np.intersect1d(caught, what["pixels"]).size, what["pixels"].size))
        assert caught.size >= 1 and np.intersect1d(caught, what["pixels"]).size >= 1, (name, defect, traversal)


def test_probe_b_catches_a_lost_second_face_as_a_leak(pbr, oracle):
    """sponza-6k under LEAK_LIGHT: among the leaves' second faces that are a decided pixel's first hit, one is the ONLY face
    between the light and a decided shadowed pixel that passes the lit gate.  Without it the any-hit walk finds the light:
    probe B reports the leak — and the oracle on the unplanted tree under that light breaks no rule."""
    sc, first, _, _ = wt.truth(pbr, "sponza-6k", 1, K_NATIVE)
    light = wt.light_row(LEAK_LIGHT)
    sc = hand_scenes.with_arrays(sc, lights=light)
    shadow = wt.shadow_truth(sc, LEAK_LIGHT, first)
    gate = wt.lit_gate(sc, 1, first, light[0].astype(np.float64), K_NATIVE, shadow)
    mask, black, lit = wt.sets(first, shadow, gate, EDGE_MARGIN)
    assert_probe_b(oracle_image(oracle, sc, wt.config_b(sc, 1))[0], first, black, lit, "unplanted")
    alone = black & first["hit"] & shadow["sole"] & gate["passes"]
    bad, what = wt.plant(sc, "second_face", first, mask, among=set(shadow["blocker"][alone].tolist()))
    leaking = np.flatnonzero(alone & (shadow["blocker"] == what["face"]))
    assert leaking.size >= 1
    for traversal in (0, 2):
        image, _ = oracle_image(oracle, bad, wt.config_b(sc, 1, traversal=traversal))
        got = wt.probe_b(image, black, lit)
        print("second face %d lost, traversal %d: %d leaks, %d of the %d foreseen" % (
            what["face"], traversal, got["leaks"].size, np.intersect1d(got["leaks"], leaking).size, leaking.size))
        assert np.intersect1d(got["leaks"], leaking).size >= 1, traversal
