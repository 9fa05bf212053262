"""tests/bvh_build_ref.py has to earn trust before the GPU is held to it: its bit tricks against loops, its codes and small
trees against answers worked out by hand, its vectorised builders against the thread-by-thread transcription on every input
family, every tree it builds for the GPU tests against check_flat_tree in full, and the properties the header of
csrc/bvh_build.hpp promises.  No device."""
import numpy as np
import pytest

import bvh_build_cases as cases
import bvh_build_ref as ref
import refit_ref
from flat_tree import check_flat_tree

F32 = np.float32


def same_trees(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def triangles(corners):
    """(vertices, facesV, facesN) of one triangle per (3, 3) entry of corners; facesN row f = (f, f, f, f)."""
    corners = np.asarray(corners, F32)
    m = corners.shape[0]
    vertices = np.zeros((3 * m, 4), F32)
    vertices[:, :3] = corners.reshape(-1, 3)
    facesV = np.zeros((m, 4), np.uint32)
    facesV[:, :3] = np.arange(3 * m).reshape(m, 3)
    return vertices, facesV, np.repeat(np.arange(m, dtype=np.uint32), 4).reshape(m, 4)


def square(x, y, side):
    """Two triangles over [x, x + side] x [y, y + side] in z = 0; each has the square as its box."""
    a, b, c, d = (x, y, 0), (x + side, y, 0), (x + side, y + side, 0), (x, y + side, 0)
    return [[a, b, d], [b, c, d]]


def box_triangle(x0, y0, x1, y1):
    return [(x0, y0, 0), (x1, y0, 0), (x0, y1, 0)]


# ----------------------------------------------------------------------------------------------------------------------
# bits and codes
# ----------------------------------------------------------------------------------------------------------------------
def test_expand_bits13_against_a_bit_loop():
    v = np.arange(8192)
    want = np.zeros(8192, np.uint64)
    for b in range(13):
        want |= ((v >> b) & 1).astype(np.uint64) << np.uint64(3 * b)
    assert np.array_equal(ref.expand_bits13(v), want)
    assert np.array_equal(ref.expand_bits13(v + 8192), want)              # only the low 13 bits count
    assert [ref._spread_slow(int(x)) for x in v[::97]] == [int(x) for x in want[::97]]


def test_codes_worked_out_by_hand():
    assert int(ref.morton_code([1, 0, 0])) == 4
    assert int(ref.morton_code([0, 1, 0])) == 2
    assert int(ref.morton_code([0, 0, 1])) == 1
    assert int(ref.morton_code([2, 0, 0])) == 32
    assert int(ref.morton_code([8191, 8191, 8191])) == 2 ** 39 - 1
    assert int(ref.morton_code([8191, 0, 0])) == sum(4 << (3 * b) for b in range(13))


def test_the_scene_minimum_is_cell_0_and_the_maximum_cell_8191():
    v, fv, _ = cases.soup(300)
    lo, hi = ref.face_boxes(v, fv)
    c = F32(0.5) * (lo + hi)
    q = ref.cells(v, fv)
    assert q.max() == 8191 and q.min() == 0
    for k in range(3):
        assert q[c[:, k].argmin(), k] == 0 and q[c[:, k].argmax(), k] == 8191
    # two faces: one at the minimum of every axis (code 0), one at the maximum (8191 on every axis, not 8192)
    v, fv, _ = triangles([box_triangle(0, 0, 1, 1), [(5, 5, 5), (6, 5, 6), (5, 6, 5)]])
    keys = ref.morton_keys(v, fv)
    assert int(keys[0]) == 0 and int(keys[1]) == ((2 ** 39 - 1) << 24) | 1
    assert ref.keys_slow(v, fv) == [int(k) for k in keys]


def test_cells_by_hand():
    """Centroids 1.5, 2.5 and 4 on an axis whose bounds are 1.5 and 4: u = 0, 0.4, 1 -> cells 0, 3276 (3276.8), 8191."""
    v, fv, _ = triangles([box_triangle(1, 1, 2, 2), box_triangle(2, 1, 3, 2), box_triangle(0, 0, 8, 8)])
    assert ref.cells(v, fv).tolist() == [[0, 0, 0], [3276, 0, 0], [8191, 8191, 0]]


def test_keys_of_duplicated_faces_differ_by_the_face_index_alone():
    for v, fv, _ in (cases.repeated(40), cases.concentric(40)):
        keys = ref.morton_keys(v, fv)
        assert np.unique(keys).size == 40
        assert (keys >> np.uint64(24) == keys[0] >> np.uint64(24)).all()
        assert np.array_equal(keys & np.uint64(0xFFFFFF), np.arange(40, dtype=np.uint64))
        assert np.array_equal(np.sort(keys), keys)                        # so the order is the face order
    v, fv, _ = cases.concentric(40)
    assert (ref.morton_keys(v, fv) >> np.uint64(24) == 0).all()           # no extent on any axis


def test_a_minus_zero_bound_counts_as_zero_extent():
    """Centroids -0.0 and +0.0 on one axis: no extent, cell 0 for both, in both transcriptions.  This does not pin the
    ordered map: with plain min / max the bound may be either zero, the extent is +0.0 either way and c - lo the same, so
    no tree changes by value.  What the map does with -0.0 is asserted here on its own; that it orders NEGATIVE floats is
    held by test_the_ordered_map_orders_floats_of_both_signs and, through the cells, by the wide case."""
    v, fv, _ = triangles([box_triangle(0, 0, 1, 1), box_triangle(3, 0, 4, 1)])
    v[0:3, 2] = -0.0
    assert np.signbit(ref._from_ordered(ref._ordered(np.array([0.0, -0.0], F32)).min()))
    assert ref.cells(v, fv).tolist() == [[0, 0, 0], [8191, 0, 0]]
    assert ref.keys_slow(v, fv) == [int(k) for k in ref.morton_keys(v, fv)]


def test_the_ordered_map_orders_floats_of_both_signs():
    x = np.array([-np.inf, -1000.0, -1.5, -1e-30, -0.0, 0.0, 1e-30, 0.25, 999.0, np.inf], F32)
    image = ref._ordered(x)
    assert (np.diff(image.astype(np.int64)) > 0).all()                    # strictly ascending, -0.0 below +0.0
    assert np.array_equal(ref._from_ordered(image).view(np.uint32), x.view(np.uint32))
    assert [ref._ordered_slow(v) for v in x] == [int(b) for b in image]
    assert ref._ordered_slow(F32(np.inf)) == 0xFF800000 and ref._ordered_slow(F32(-np.inf)) == 0x007FFFFF
    # a map that kept negative floats in bit order would put the bounds of the wide case elsewhere, and with them the cells
    v, fv, _ = cases.wide(90)
    lo, hi = ref.face_boxes(v, fv)
    c = F32(0.5) * (lo + hi)
    assert (c.min(0) < 0).all() and (c.max(0) > 0).all()
    q = ref.cells(v, fv)
    for k in range(3):
        assert q[c[:, k].argmin(), k] == 0 and q[c[:, k].argmax(), k] == 8191


def test_pair_key_array_is_the_scalar_one():
    lo, hi = np.meshgrid(np.arange(0, 900, 7), np.arange(0, 900, 11), indexing="ij")
    want = np.array([[ref.pair_key(int(a), int(b)) for a, b in zip(ra, rb)] for ra, rb in zip(lo, hi)], np.uint32)
    assert np.array_equal(ref._pair_key_array(lo, hi), want)
    assert ref.pair_key(0, 0) == 0 and all(0 <= int(k) < 2 ** 32 for k in want.ravel())


def test_leading_zeros():
    x = np.array([1, 2, 3, 1 << 24, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 0x00F0000000000000], np.uint64)
    assert ref._clz64(x).tolist() == [64 - int(v).bit_length() for v in x]


def test_radius_rule():
    assert [ref.radius_used(k, False) for k in (-1, 0, 1, 3, 64, 65, 200)] == [32, 32, 1, 3, 64, 64, 64]
    assert [ref.radius_used(k, True) for k in (-1, 0, 1, 32, 200)] == [3, 3, 1, 32, 64]


# ----------------------------------------------------------------------------------------------------------------------
# the two transcriptions against each other, and every tree the GPU will be held to against the format
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SMALL))
def test_vectorised_equals_thread_by_thread(name):
    v, fv, fn = cases.SMALL[name]()
    assert fv.shape[0] <= 96
    assert sorted(ref.keys_slow(v, fv)) == [int(k) for k in np.sort(ref.morton_keys(v, fv))]
    for radius in (1, 3, 64):
        assert same_trees(ref.ploc(v, fv, fn, radius), ref.ploc_slow(v, fv, fn, radius)), radius
    assert same_trees(ref.lbvh(v, fv, fn), ref.lbvh_slow(v, fv, fn))


def test_vectorised_equals_thread_by_thread_on_the_cornell_box(pbr):
    v, fv, fn = cases.scene(pbr, "cornell", 0)
    assert fv.shape[0] <= 96
    for radius in (1, 3, 64):
        assert same_trees(ref.ploc(v, fv, fn, radius), ref.ploc_slow(v, fv, fn, radius)), radius
    assert same_trees(ref.lbvh(v, fv, fn), ref.lbvh_slow(v, fv, fn))


@pytest.mark.parametrize("kind", ["sponza", "hairball"])
def test_vectorised_equals_thread_by_thread_on_small_generated_scenes(pbr, kind):
    v, fv, fn = cases.small_scene(pbr, kind)
    assert 80 <= fv.shape[0] <= 96
    for radius in (1, 3, 64):
        assert same_trees(ref.ploc(v, fv, fn, radius), ref.ploc_slow(v, fv, fn, radius)), radius
    assert same_trees(ref.lbvh(v, fv, fn), ref.lbvh_slow(v, fv, fn))


def test_the_rounding_order_of_the_half_area_decides_trees_of_the_skew_case():
    """The skew case is there to hold (x * y + z * y) + x * z to that order: with the sum associated the other way, both
    builders give another tree at every radius.  (The other inputs do not notice.)"""
    v, fv, fn = cases.FULL["skew-120"]()
    want = [ref.ploc(v, fv, fn, radius) for radius in (1, 32)] + [ref.lbvh(v, fv, fn)]

    def other_way(lo, hi):
        e = hi - lo
        return e[..., 0] * e[..., 1] + (e[..., 2] * e[..., 1] + e[..., 0] * e[..., 2])

    # ploc and lbvh look _half_area up as a global of their module at call time: replacing the attribute reaches both
    kept, ref._half_area = ref._half_area, other_way
    try:
        got = [ref.ploc(v, fv, fn, radius) for radius in (1, 32)] + [ref.lbvh(v, fv, fn)]
    finally:
        ref._half_area = kept
    assert not any(same_trees(a, b) for a, b in zip(got, want))
    assert all(same_trees(a, b) for a, b in zip(want, [ref.ploc_slow(v, fv, fn, 1), ref.ploc_slow(v, fv, fn, 32), ref.lbvh_slow(v, fv, fn)]))


def check_every_builder(v, fv, fn):
    trees = [ref.ploc(v, fv, fn, radius) for radius in (1, 3, 32, 64)] + [ref.lbvh(v, fv, fn)]
    for nodes, outV, outN in trees:
        assert nodes.dtype == np.float32 and outV.dtype == np.uint32 and outN.dtype == np.uint32
        assert nodes.shape[0] <= max(2, 2 * fv.shape[0] - 1)              # pbr_bvh_node_capacity
        check_flat_tree(nodes, outV, fv, v, sample=None)
    return trees


@pytest.mark.parametrize("name", list(cases.FULL))
def test_restated_trees_are_flat_trees(name):
    check_every_builder(*cases.FULL[name]())


@pytest.mark.parametrize("kind,triangles_", cases.SCENES)
def test_restated_trees_of_generated_scenes_are_flat_trees(pbr, kind, triangles_):
    check_every_builder(*cases.scene(pbr, kind, triangles_))


def test_check_flat_tree_checks_the_root_box_and_every_node():
    v, fv, fn = cases.soup(300)
    nodes, outV, _ = ref.ploc(v, fv, fn, 32)
    check_flat_tree(nodes, outV, fv, v)
    for sample in (None, (4000, 2000)):
        bad = nodes.copy()
        bad[0, 4] += 1.0                                                  # a root box that is too wide
        with pytest.raises(AssertionError):
            check_flat_tree(bad, outV, fv, v, sample=sample)
    last_leaf = np.nonzero(nodes[:, 3] >= 0)[0][-1]
    last_container = np.nonzero(nodes[:, 3] < 0)[0][-1]
    for i in (last_leaf, last_container):
        bad = nodes.copy()
        bad[i, 0] -= 1.0
        with pytest.raises(AssertionError):
            check_flat_tree(bad, outV, fv, v, sample=None)


# ----------------------------------------------------------------------------------------------------------------------
# known answers
# ----------------------------------------------------------------------------------------------------------------------
def builders(v, fv, fn, radii=(1, 3, 64)):
    for radius in radii:
        yield "ploc %d" % radius, ref.ploc(v, fv, fn, radius)
        yield "ploc_slow %d" % radius, ref.ploc_slow(v, fv, fn, radius)
    yield "lbvh", ref.lbvh(v, fv, fn)
    yield "lbvh_slow", ref.lbvh_slow(v, fv, fn)


def test_two_far_apart_pairs_make_a_root_over_two_leaves_bigger_first():
    """Faces 0, 1: the unit square at the origin; faces 2, 3: a square of side 2 at x = 100.  Morton order 0 1 2 3; each pair
    is one leaf (both builders); the root's children are exchanged, half area 4 > 1."""
    v, fv, fn = triangles(square(0, 0, 1) + square(100, 0, 2))
    want = np.array([[0, 0, 0, -1, 102, 2, 0, -1],
                     [100, 0, 0, 0, 102, 2, 0, 1],
                     [0, 0, 0, 2, 1, 1, 0, 3]], F32)
    for what, (nodes, outV, outN) in builders(v, fv, fn):
        if what.startswith("ploc"):
            assert np.array_equal(nodes, want), what
            assert np.array_equal(outV, fv[[2, 3, 0, 1]]) and np.array_equal(outN, fn[[2, 3, 0, 1]]), what
    want[1:, 3], want[1:, 7] = [2, 0], [3, 1]                             # the radix tree leaves the faces in Morton order
    for what in (ref.lbvh, ref.lbvh_slow):
        nodes, outV, outN = what(v, fv, fn)
        assert np.array_equal(nodes, want)
        assert np.array_equal(outV, fv) and np.array_equal(outN, fn)


def test_small_faces_cluster_before_the_big_one_joins():
    """Face 0 = T, box [0, 8]^2; inside it s1 = face 1 [1, 2] x [1, 2], s2 = face 2 [2.5, 3.5] x [1, 2], s3 = face 3
    [1, 2] x [2, 3].  Centroids (4, 4), (1.5, 1.5), (3, 1.5), (1.5, 2.5): cells (8191, 8191), (0, 0), (4915, 0), (0, 3276);
    x is the higher bit, so the order is s1 s3 s2 T.  Half areas of unions: s1 s3 2, s1 s2 2.5, s3 s2 5, anything with T 64.
    Round 1 (radius 1 and 3 alike: s1 and s3 choose each other, s2 chooses one of them, nobody chooses T): leaf {s1, s3}.
    Round 2: {s1, s3} and s2 (5 < 64): a container, the leaf (area 2) before s2 (area 1).  Round 3: T (64) before it."""
    v, fv, fn = triangles([box_triangle(0, 0, 8, 8), box_triangle(1, 1, 2, 2), box_triangle(2.5, 1, 3.5, 2), box_triangle(1, 2, 2, 3)])
    assert ref.cells(v, fv).tolist() == [[8191, 8191, 0], [0, 0, 0], [4915, 0, 0], [0, 3276, 0]]
    want = np.array([[0, 0, 0, -1, 8, 8, 0, -1],
                     [0, 0, 0, 0, 8, 8, 0, -1],
                     [1, 1, 0, -1, 3.5, 3, 0, -1],
                     [1, 1, 0, 1, 2, 3, 0, 2],
                     [2.5, 1, 0, 3, 3.5, 2, 0, -1]], F32)
    for what, (nodes, outV, outN) in builders(v, fv, fn):
        if what.startswith("ploc"):
            assert np.array_equal(nodes, want), what
            assert np.array_equal(outV, fv[[0, 1, 3, 2]]) and np.array_equal(outN, fn[[0, 1, 3, 2]]), what
    # the radix tree pairs sorted neighbours instead: {s1, s3}, {s2, T}; the bigger leaf first
    want = np.array([[0, 0, 0, -1, 8, 8, 0, -1],
                     [0, 0, 0, 2, 8, 8, 0, 3],
                     [1, 1, 0, 0, 2, 3, 0, 1]], F32)
    for what in (ref.lbvh, ref.lbvh_slow):
        nodes, outV, outN = what(v, fv, fn)
        assert np.array_equal(nodes, want)
        assert np.array_equal(outV, fv[[1, 3, 2, 0]]) and np.array_equal(outN, fn[[1, 3, 2, 0]])


def test_a_miss_link_points_behind_the_subtree():
    """Three unit squares in a row at x = 0, 10, 30 and a fourth single triangle at 70: leaves A B C and the face d.  Round 1
    merges the face pairs (d waits); round 2 A with B (union 11 x 1 < B with C 21 x 1); round 3 {A, B} with C; round 4 d.
    Equal areas keep the position's own cluster first.  Records: root, AB-C container, A-B container, A, B, C, d."""
    v, fv, fn = triangles(square(0, 0, 1) + square(10, 0, 1) + square(30, 0, 1) + [box_triangle(70, 0, 71, 1)])
    nodes, outV, _ = ref.ploc(v, fv, fn, 1)
    assert nodes[:, 3].tolist() == [-1, -1, -1, 0, 2, 4, 6]
    assert nodes[:, 7].tolist() == [-1, 6, 5, 1, 3, 5, -1]
    assert nodes[:, 0].tolist() == [0, 0, 0, 0, 10, 30, 70] and nodes[:, 4].tolist() == [71, 31, 11, 1, 11, 31, 71]
    assert np.array_equal(outV, fv)
    assert same_trees(ref.ploc(v, fv, fn, 1), ref.ploc_slow(v, fv, fn, 1))


@pytest.mark.parametrize("faces", [1, 2])
def test_one_leaf_gets_a_root(faces):
    v, fv, fn = triangles(square(3, 4, 2)[:faces])
    for what, (nodes, outV, outN) in builders(v, fv, fn):
        assert nodes.shape == (2, 8), what
        assert nodes[1].tolist() == [3, 4, 0, 0, 5, 6, 0, 1 if faces == 2 else -1], what
        assert nodes[0].tolist() == [3, 4, 0, -1, 5, 6, 0, -1], what
        assert np.array_equal(outV, fv) and np.array_equal(outN, fn), what


# ----------------------------------------------------------------------------------------------------------------------
# properties
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup-61", "strip-65", "grid-72", "repeated-40", "wide-90"])
def test_a_radius_that_reaches_everywhere_merges_the_smallest_pair_of_all(name):
    """Every round, the pair that is least in (half area of the union, pairKey, lower position, upper position) over ALL
    pairs merges: the progress the device's host loop relies on.  Checked through the `rounds` hook of the vectorised ploc
    alone, on at most 64 faces (radius 64 has to reach across); ploc_slow has no such hook and is held to this only through
    its equality with ploc in test_vectorised_equals_thread_by_thread."""
    v, fv, fn = cases.SMALL[name]()
    count = min(fv.shape[0], 64)                                          # radius 64 has to reach across
    v, fv, fn = v, fv[:count], fn[:count]
    rounds = []
    ref.ploc(v, fv, fn, 64, rounds=rounds)
    assert rounds and rounds[-1][0].shape[0] == 2
    for lo, hi, merging in rounds:
        best = None
        for i in range(lo.shape[0]):
            for j in range(i + 1, lo.shape[0]):
                e = np.maximum(hi[i], hi[j]) - np.minimum(lo[i], lo[j])
                area = F32(F32(e[0] * e[1]) + F32(e[2] * e[1])) + F32(e[0] * e[2])
                entry = (float(area), ref.pair_key(i, j), i, j)
                best = entry if best is None or entry < best else best
        assert [best[2], best[3]] in merging.tolist()
        assert (merging[:, 0] < merging[:, 1]).all()


@pytest.mark.parametrize("name", ["soup-96", "grid-72", "repeated-40", "permuted-77", "tiny-5"])
def test_normals_travel_with_their_faces(name):
    v, fv, fn = cases.SMALL[name]()
    fv, fn = fv.copy(), fn.copy()
    fv[:, 3] = np.arange(fv.shape[0])                                     # tag each face
    fn[:, 3] = np.arange(fv.shape[0])
    for tree in (ref.ploc(v, fv, fn, 3), ref.ploc(v, fv, fn, 64), ref.lbvh(v, fv, fn)):
        order = tree[1][:, 3]
        assert np.array_equal(np.sort(order), np.arange(fv.shape[0]))
        assert np.array_equal(tree[1], fv[order]) and np.array_equal(tree[2], fn[order])


def test_a_radius_above_64_is_64():
    v, fv, fn = cases.soup(300)
    assert same_trees(ref.ploc(v, fv, fn, 200), ref.ploc(v, fv, fn, 64))
    assert not same_trees(ref.ploc(v, fv, fn, 64), ref.ploc(v, fv, fn, 32))
    v, fv, fn = cases.soup(96)
    assert same_trees(ref.ploc_slow(v, fv, fn, 200), ref.ploc(v, fv, fn, 64))
    assert same_trees(ref.ploc_slow(v, fv, fn, 0), ref.ploc(v, fv, fn, 1))


def test_the_face_order_decides_between_equal_codes_only():
    """The permuted soup is the same geometry: the same boxes in the same tree shape wherever the codes differ."""
    v, fv, fn = cases.soup(257)
    _, pv, pn = cases.permuted(257)
    assert np.unique(ref.morton_keys(v, fv) >> np.uint64(24)).size == 257  # no two faces share a cell here
    a, b = ref.ploc(v, fv, fn, 32), ref.ploc(v, pv, pn, 32)
    assert same_trees(a, b)
    assert same_trees(ref.lbvh(v, fv, fn), ref.lbvh(v, pv, pn))


def test_bigger_child_first_everywhere():
    """Every container has two children, the first's half area >= the second's (the device exchanges on a strict >)."""
    v, fv, fn = cases.wide(300)
    for nodes, _, _ in (ref.ploc(v, fv, fn, 32), ref.ploc(v, fv, fn, 1), ref.lbvh(v, fv, fn)):
        area = ref._half_area(nodes[:, 0:3], nodes[:, 4:7])
        leaf, _, _, end, _ = refit_ref.tree_tables(nodes)
        for i in np.nonzero(~leaf)[0]:
            first, second = refit_ref.children(i, end)
            assert area[first] >= area[second], i
