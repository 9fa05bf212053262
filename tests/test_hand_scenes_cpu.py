"""What tests/test_gpu_hand_trees.py assumes about the hand-made scenes of tests/hand_scenes.py, established without a GPU, so
that a failure there is the device's and not the model's: every shape is a valid, properly nested tree of the size and height
it is there for; the numpy folds agree with each other and with the C++ restatements (refit, re-link, thick refit) on every
shape and option; and the oracle's walks, in every traversal, find the closest hits of a float64 brute force over all faces
for exactly the seeded rays the GPU test traces — zero rays outside the tolerance, which is a condition on the inputs."""
import numpy as np
import pytest

import hand_scenes
import patch_refit_ref
import refit_ref
from flat_tree import check_flat_tree
from test_patch_refit_cpu import cxx_refit, driver as patch_lib  # noqa: F401  (fixtures)
from test_refit_cpu import Plan, bits, driver as refit_lib  # noqa: F401
from test_relink_cpu import assert_same_walk, run, driver as relink_lib  # noqa: F401

OPTIONS = ({"degenerate": True}, {"signed_zeros": True}, {"loose": True})
LAYOUTS = (1, 2, 3)
HOT = (None, 0, 8, 64)             # the ranking whole and shortened: cold records on every shape with more than 65 nodes
ALPHA = hand_scenes.ALPHA


@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_shapes_are_valid_nested_and_of_the_size_they_are_there_for(pbr, refit_lib, shape):
    """pbr_validate_scene, check_flat_tree (structure for every option, boxes too where they are tight), node count, height
    and leaves of the table, the nesting verdict, and the partition at the library's cut of 256 that the shape is there for."""
    nodes, height, leaves = hand_scenes.EXPECT[shape]
    for options in ({},) + OPTIONS:
        sc = hand_scenes.scene(pbr, shape, **options)
        a = sc.arrays
        assert pbr.validate_scene(sc.desc) == ""
        check_flat_tree(a["bvh"], a["facesV"], a["facesV"], a["vertices"], sample=(0, 0) if options.get("loose") else None)
        leaf, face0, face1, end, parent = refit_ref.tree_tables(a["bvh"])
        assert (a["bvh"].shape[0], int(refit_ref.heights(leaf, parent)[0]), int(leaf.sum())) == (nodes, height, leaves)
        assert a["vertices"].shape[0] == 3 * a["facesV"].shape[0] and np.array_equal(a["facesV"], a["facesN"])
    plan = Plan(refit_lib, sc.desc)
    assert plan.nested, plan.why
    assert plan.nodes == nodes and int(plan.height[0]) == height
    if nodes <= 256:
        assert plan.top == 0 and plan.levels == 0 and plan.groups == 1 and plan.subtree_roots.tolist() == [0]
    else:
        assert plan.top >= 1 and plan.top_nodes[-1] == 0
    if shape == "cut257":
        assert plan.top == 1 and plan.subtrees == 2                   # node 0 alone above the cut
    if shape == "chain300":
        assert plan.levels == plan.top > 100                           # one node per level
    if shape == "chain1400":
        assert plan.levels == plan.top > 1000
    if shape == "ternary10":
        # the leaf between two containers is a subtree of one node wherever its parent lies above the cut
        sizes = plan.end[plan.subtree_roots] - plan.subtree_roots
        assert plan.subtrees > plan.groups > 1 and (sizes == 1).sum() > 10
        assert max(len(list(refit_ref.children(int(i), plan.end))) for i in plan.top_nodes) == 3
    if shape in ("wide7", "wide40"):
        assert list(refit_ref.children(0, plan.end)) == [1] and len(list(refit_ref.children(1, plan.end))) == leaves
    plan.close()


def test_options_do_what_they_say(pbr):
    """Three equal corners; zeros of both signs in both fold orders, which decide box words; loose boxes are all the scene's;
    the move keeps all of that; lattice keys tie and both child orders occur."""
    sc = hand_scenes.scene(pbr, "wide40", degenerate=True)
    tri = sc.arrays["vertices"][:, :3].reshape(-1, 3, 3)
    point = (tri == tri[:, :1]).all(axis=(1, 2))
    assert 1 <= point.sum() < len(tri) // 2 and sc.flat[point].all()
    moved = hand_scenes.move(sc)[:, :3].reshape(-1, 3, 3)
    assert np.array_equal(point, (moved == moved[:, :1]).all(axis=(1, 2))) and not np.array_equal(moved, tri)
    for shape in ("leaf1", "wide7", "ternary10"):
        sc = hand_scenes.scene(pbr, shape, signed_zeros=True)
        v = sc.arrays["vertices"]
        tri = bits(v[:, :3]).reshape(-1, 3, 3)
        plus, minus = tri == 0, tri == 0x80000000
        assert plus[0, 0, :].any() and minus[0, 1, :].any()           # face 0: +0 before -0 on its axis
        if len(tri) > 1:
            assert ((minus[:, 0] & plus[:, 1]).any(axis=1)).any()      # and -0 before +0 on another face
        boxes = bits(sc.arrays["bvh"][:, [0, 1, 2, 4, 5, 6]])
        assert (boxes == 0).any() and (shape == "leaf1" or (boxes == 0x80000000).any())
        kept = bits(hand_scenes.move(sc)[:, :3]).reshape(-1, 3, 3)
        in_plane = np.broadcast_to((plus | minus).all(axis=1, keepdims=True), tri.shape)
        assert in_plane[:min(len(tri), 4)].any(axis=(1, 2)).all() and np.array_equal(kept[in_plane], tri[in_plane])
        # the move is rigid otherwise: the faces without area are the same ones
        moved = hand_scenes.move(sc)[:, :3].astype(np.float64).reshape(-1, 3, 3)
        assert np.array_equal(np.linalg.norm(np.cross(moved[:, 1] - moved[:, 0], moved[:, 2] - moved[:, 0]), axis=1) == 0, sc.flat)
    # ... and the order decides words of the boxes the GPU test compares: a fold by minimum and maximum instructions that
    # order -0 below +0 would give -0 where the fold keeps the +0 it met first, and +0 where it keeps -0
    for shape in ("leaf1", "wide7", "chain300", "cut257", "ternary10"):
        sc = hand_scenes.scene(pbr, shape, degenerate=True, signed_zeros=True, loose=True)
        v, after = hand_scenes.moved(sc)
        leaf, face0, face1, _, _ = refit_ref.tree_tables(after.arrays["bvh"])
        boxes, corners = bits(after.arrays["bvh"]), bits(v[:, :3]).reshape(-1, 3, 3)
        lo_decided = hi_decided = 0
        for i in np.nonzero(leaf)[0]:
            mine = corners[[face0[i]] + ([face1[i]] if face1[i] >= 0 else [])].reshape(-1, 3)
            lo_decided += int(((boxes[i, 0:3] == 0) & (mine == 0x80000000).any(axis=0)).sum())
            hi_decided += int(((boxes[i, 4:7] == 0x80000000) & (mine == 0).any(axis=0)).sum())
        assert lo_decided >= 1 and (shape == "leaf1" or hi_decided >= 1), (shape, lo_decided, hi_decided)
    sc = hand_scenes.scene(pbr, "cut257", loose=True)
    assert (sc.arrays["bvh"][:, [0, 1, 2, 4, 5, 6]] == sc.arrays["bvh"][0, [0, 1, 2, 4, 5, 6]]).all()
    sc = hand_scenes.scene(pbr, "wide40")
    key = sc.arrays["bvh"][2:, 0:3] + sc.arrays["bvh"][2:, 4:7]
    for axis in range(3):
        assert len(np.unique(key[:, axis])) < len(key)               # ties
        step = np.diff(key[:, axis])
        assert (step > 0).any() and (step < 0).any()                  # both orders among depth-first neighbours


@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_numpy_folds_agree_with_each_other_and_with_the_cxx_refit(pbr, refit_lib, shape):
    """refit_ref.refit == refit_slow (small trees) == the C++ refit of pt_refit_host.hpp, all eight words as bits, for V and
    for the moved V', under every option."""
    for options in OPTIONS:
        sc = hand_scenes.scene(pbr, shape, **options)
        a = sc.arrays
        plan = Plan(refit_lib, sc.desc)
        for what, v in (("V", a["vertices"]), ("V'", hand_scenes.move(sc))):
            want = refit_ref.refit(a["bvh"], a["facesV"], v)
            assert np.array_equal(bits(plan.refit(a["facesV"], v)), bits(want)), (shape, options, what)
            assert np.array_equal(bits(want[:, [3, 7]]), bits(a["bvh"][:, [3, 7]]))
            if a["bvh"].shape[0] <= 1000:
                assert np.array_equal(bits(refit_ref.refit_slow(a["bvh"], a["facesV"], v)), bits(want)), (shape, options, what)
        plan.close()


@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_cxx_relink_equals_pack_walk(pbr, relink_lib, shape):
    """relinkWalk == packWalk on the refitted tree, byte for byte: every option, V and V', layouts 1 - 3, the ranking whole
    and shortened.  The levels are the tree's height; a chain's share one launch."""
    nodes, height, _ = hand_scenes.EXPECT[shape]
    for options in OPTIONS:
        sc = hand_scenes.scene(pbr, shape, **options)
        a = sc.arrays
        for what, v in (("V", a["vertices"]), ("V'", hand_scenes.move(sc))):
            boxes = refit_ref.refit(a["bvh"], a["facesV"], v)
            for layout in LAYOUTS:
                for hot in HOT:
                    want, got, tables = run(relink_lib, sc.desc, boxes, layout, hot)
                    assert_same_walk(want, got, (shape, options, what, layout, hot))
                    assert tables["levels"] == height
                    if hot is not None:
                        assert tables["hot_per_stream"] == min(hot, nodes - 1)
                    if shape.startswith("chain"):
                        assert tables["launches"] == 1 and tables["containers"] == height
        if options.get("loose") and nodes > 2:
            old, _, _ = run(relink_lib, sc.desc, a["bvh"], 2)
            assert old["bytes"] != want["bytes"], "tight boxes order the children as loose ones do"


def test_chain1400_has_cold_records_in_every_layout(pbr, relink_lib):
    sc = hand_scenes.scene(pbr, "chain1400")
    for layout in LAYOUTS:
        _, _, tables = run(relink_lib, sc.desc, sc.arrays["bvh"], layout)
        assert 0 < tables["hot_per_stream"] < sc.arrays["bvh"].shape[0] - 1, layout


@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_cxx_thick_refit_equals_numpy(pbr, patch_lib, shape):
    """pt_patch_refit_host.hpp against patch_refit_ref.refit, both ways to a leaf's box, on every shape; the scene has a face
    with equal normals, a face without area (where it has two faces), and curved faces whose thick box is larger than the
    tight one (where it has three)."""
    sc, v, n, moved = hand_scenes.phong_case(pbr, shape)
    a = sc.arrays
    tri, nn = a["vertices"][:, :3].reshape(-1, 3, 3), a["normals"][:, :3].reshape(-1, 3, 3)
    assert (nn[-1] == nn[-1][0]).all()
    if len(tri) >= 2:
        assert sc.flat[-2] and not np.cross(tri[-2, 1] - tri[-2, 0], tri[-2, 2] - tri[-2, 0]).any()
    for vertices, normals in ((a["vertices"], a["normals"]), (v, n)):
        want = patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], vertices, normals, ALPHA)
        for from_face_boxes in (0, 1):
            got = cxx_refit(patch_lib, sc.desc, a, vertices, normals, ALPHA, from_face_boxes)
            assert np.array_equal(bits(got), bits(want)), (shape, from_face_boxes)
        assert np.isfinite(want[:, [0, 1, 2, 4, 5, 6]]).all()
        tight = refit_ref.refit(a["bvh"], a["facesV"], vertices)
        assert (want[:, 0:3] <= tight[:, 0:3]).all() and (want[:, 4:7] >= tight[:, 4:7]).all()
        if len(tri) >= 3:                                                # of two faces one has equal normals, the other no area
            assert (want[:, 0:3] < tight[:, 0:3]).any() or (want[:, 4:7] > tight[:, 4:7]).any()
    assert np.array_equal(bits(moved.arrays["bvh"]), bits(want))
    nn = n[:, :3].reshape(-1, 3, 3)
    assert (nn[-1] == nn[-1][0]).all() and not np.array_equal(n, a["normals"])


@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_oracle_walks_find_the_brute_force_hits(pbr, oracle, shape):
    """The oracle in traversals 0 - 3 over tight and loose boxes against Moeller-Trumbore over all faces in float64, for the
    rays the GPU test traces: no ray outside 1e-3 max( 1, t ), none left out, at least half of them hit.  The ordered walk is
    another walk: under tight boxes its per-ray counts differ from the reference order's wherever there is more than one
    leaf — the node counts where a container below node 1 can be skipped, the face tests in the flat shapes (wide7, wide40:
    every leaf is visited whatever the order, only the tests inside it are saved)."""
    for what, sc in hand_scenes.walk_scenes(pbr, shape):
        rays, best = hand_scenes.rays_of(sc), hand_scenes.brute_force_of(sc)
        assert rays.shape == (hand_scenes.RAYS, 6) and best.shape == (hand_scenes.RAYS,)
        assert np.isfinite(best).sum() >= hand_scenes.RAYS // 2
        counts = {}
        for traversal in (0, 1, 2, 3):
            t, face, normal, counts[traversal] = oracle.trace_rays(sc.desc, sc.config(traversal=traversal), rays)
            bad = hand_scenes.outliers(t, best)
            assert bad.size == 0, (shape, what, traversal, [(int(k), float(t[k]), float(best[k])) for k in bad[:4]])
            hit = np.isfinite(t)
            assert (face[hit] >= 0).all() and not sc.flat[face[hit]].any()
        assert np.array_equal(counts[2], counts[3])                      # the compact layout: the same visits
        if what == "tight" and hand_scenes.EXPECT[shape][2] > 1:
            assert not np.array_equal(counts[0], counts[2]), shape
            if not shape.startswith("wide"):
                assert not np.array_equal(counts[0][:, 0], counts[2][:, 0]), shape
        if what == "loose":
            # a ray that hits something visits every node, in every order (but one whose hit lies on the scene's box, where it enters)
            for traversal in (0, 1, 2):
                visited = counts[traversal][np.isfinite(best), 0]
                assert (visited <= hand_scenes.EXPECT[shape][0] - 1).all() and (visited == hand_scenes.EXPECT[shape][0] - 1).mean() > 0.95


@pytest.mark.parametrize("shape", hand_scenes.SHAPES)
def test_oracle_renders_the_scenes_and_their_moved_versions(pbr, oracle, shape):
    """The small image the GPU test renders is finite and sees geometry, for S and for S', lit and unlit."""
    sc = hand_scenes.scene(pbr, shape, degenerate=True, signed_zeros=True)
    _, after = hand_scenes.moved(sc)
    lit = hand_scenes.scene(pbr, shape, degenerate=True, signed_zeros=True, lights=True, brdf=0)
    for what, s, cfg in (("S", sc, sc.cfg), ("S'", after, sc.cfg), ("lit", lit, lit.config(shadow_rays=1, traversal=2))):
        assert pbr.validate_scene(s.desc) == ""
        r = oracle.Renderer(s.desc, cfg, threads=4)
        img = r.render(0, s.seeds, s.px, s.cam)
        assert np.isfinite(img[..., :3]).all(), (shape, what)
        seen = np.isfinite(img[..., 3]).mean()
        assert r.counter_dict()["hits"] > 0 and seen > 0.02, (shape, what, seen)
