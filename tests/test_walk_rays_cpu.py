"""What tests/test_gpu_walk_rays.py assumes about its inputs, and the oracle's two walks per ray against the reference's own.

  * every class of tests/walk_rays.py holds its defining condition in numpy binary32 — the slab arithmetic of intersectBox and
    the Moeller-Trumbore t restated there, nothing else — and is empty on no scene it is used with;
  * oracle.trace_rays (with a starting t) and oracle.trace_shadow_rays equal every recording of the reference's compiled
    traverse / traverseShadows (tests/golden/refkernel_walk_*.npz) bit for bit: t, face, node visits, face tests — and, where
    the reference's tree exists, a fresh build and run;
  * the oracle's closest-hit walk is what it was on the recordings that were there before;
  * the random rays: at least 95 % per tree are decided in float64 from the inputs alone, and on those the oracle's verdict
    (blocked: t < tLight) has no exception.
"""
import os
import sys

import numpy as np
import pytest

import hand_scenes
import walk_rays as wr
from conftest import same_values, describe_mismatch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_refkernel as mk              # noqa: E402
from oracle import refkernel             # noqa: E402

F = np.float32
WALK_NAMES = sorted(mk.WALK_CASES)
needs_reference = pytest.mark.skipif(not refkernel.available(), reason="the reference's kernel sources only exist in the build container")
RANDOM_TREES, bits, random_scene = wr.RANDOM_TREES, wr.bits, wr.random_scene


def node_boxes(sc):
    bvh = sc.arrays["bvh"]
    return bvh[:, 0:3], bvh[:, 4:7]


def slabs(sc, s, node):
    lo, hi = node_boxes(sc)
    return wr.slab32(lo[node], hi[node], s.rays[:, 0:3], s.rays[:, 3:6])


def lane_nodes(sc, lane):
    """The leaves whose box lies in a lane, in node order."""
    bvh, Y = sc.arrays["bvh"], wr.LANES[lane]
    return [i for i in range(1, bvh.shape[0]) if bvh[i, 3] >= 0 and Y - 1 <= bvh[i, 1] and bvh[i, 5] <= Y + 3]


def face_tri(sc, face):
    a = sc.arrays
    return a["vertices"][a["facesV"][face, :3].astype(np.int64), :3]


# ---- the classes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lights", (False, True))
@pytest.mark.parametrize("anyhit", (False, True))
def test_lanes_classes_hold_their_conditions(pbr, anyhit, lights):
    sc, s = wr.lanes_scene(pbr, lights), wr.lanes_rays(anyhit, lights)
    bvh = sc.arrays["bvh"]
    c = s.classes
    assert all(m.any() for m in c.values())
    assert sc.second > 1 and bvh[sc.second, 3] == -1 and bvh[sc.second, 7] == -1 and bvh[-1, 3] >= 0      # a miss link of -1; the last record is a leaf

    # tFar == EPSILON5 exactly and one place to either side, tNear == tFar, on a leaf box and on a container box
    for lane, node in (("flat_leaf", lane_nodes(sc, "flat_leaf")[0]), ("flat_container", lane_nodes(sc, "flat_container")[0] - 1)):
        assert (bvh[node, 3] >= 0) == (lane == "flat_leaf") and bvh[node, 0] == bvh[node, 4] == 0
        near, far, nans = slabs(sc, s, node)
        for name, e in (("tfar_eps", wr.EPSILON5), ("tfar_eps_up", wr.EPS_UP), ("tfar_eps_down", wr.EPS_DOWN)):
            m = c["%s_%s" % (name, lane)]
            assert m.sum() == 2 and (far[m] == e).all() and (near[m] == far[m]).all() and (nans[m] == 0).all()
    assert wr.EPS_DOWN < wr.EPSILON5 < wr.EPS_UP and bits(wr.EPS_UP) - bits(wr.EPSILON5) == 1 and bits(wr.EPSILON5) - bits(wr.EPS_DOWN) == 1

    # a box met at a corner: the last record
    near, far, _ = slabs(sc, s, bvh.shape[0] - 1)
    assert (near[c["corner"]] == 2).all() and (far[c["corner"]] == 2).all()

    # 0 * inf: NaN terms in one, two and three axes are dropped and the box is missed; a flat box met in its plane is decided by the other axes
    nan_leaf, flat_leaf = lane_nodes(sc, "nan")[0], lane_nodes(sc, "flat_leaf")[0]
    near, far, nans = slabs(sc, s, nan_leaf)
    for k in (1, 2, 3):
        m = c["nan%d" % k]
        assert (nans[m] == k).all() and not wr.box_hit32(near[m], far[m], s.t0[m], False).any()
        assert {bool(v) for v in np.signbit(s.rays[m, 3])} == {False, True}
        # with every component zero a corner's three other planes lie at +-inf: all +inf is tNear == tFar == inf, which the
        # any-hit condition takes for a hit (inf <= inf, inf > EPSILON5) and `ray.t > tNear` culls
        hit_any = wr.box_hit32(near[m], far[m], s.t0[m], True)
        assert hit_any.any() == (k == 3) and (near[m][hit_any] == np.inf).all() and (far[m][hit_any] == np.inf).all()
    near, far, nans = slabs(sc, s, lane_nodes(sc, "nan")[1])                         # the box that is one point: all six terms are NaN
    m = c["nan_all"]
    assert (nans[m] == 3).all() and np.isnan(near[m]).all() and (far[m] == np.inf).all()        # fmin( NaN, INFINITY ): tFar is inf, a min3 of three NaN is NaN
    assert not wr.box_hit32(near[m], far[m], s.t0[m], anyhit).any()
    near, far, nans = slabs(sc, s, flat_leaf)
    m = c["flat_in_plane"]
    assert (nans[m] == 1).all() and (near[m] == 1).all() and (far[m] == 5).all()

    # zero direction components of both signs, on rays that hit
    m = c["zero_signs"]
    assert {(bool(a), bool(b)) for a, b in np.signbit(s.rays[m][:, 4:6])} == {(False, False), (False, True), (True, False), (True, True)}
    assert (s.rays[m][:, 4:6] == 0).all()

    # a ray that misses node 1 / hits it; both ends of the walk
    near, far, _ = slabs(sc, s, 1)
    hits1 = wr.box_hit32(near, far, s.t0, anyhit)
    assert hits1.any() and (~hits1).any()
    near, far, _ = slabs(sc, s, sc.second)
    hits2 = wr.box_hit32(near, far, s.t0, anyhit)
    assert (hits2 & ~hits1).any()         # ... ends on the last record
    assert (~hits2 & hits1).any()         # ... ends through the second container's miss link of -1

    # the two faces of one leaf: the first blocks at t = 2, the second lies nearer; two faces at equal t
    for name, lane, want in (("two_faces_block", "two_face", (2, 1)), ("equal_t", "equal_t", (2, 2))):
        leaf = lane_nodes(sc, lane)[0]
        f0, f1 = int(bvh[leaf, 3]), int(bvh[leaf, 7])
        assert f1 == f0 + 1
        m = c[name]
        near, _, _ = slabs(sc, s, leaf)
        for f, t_want in zip((f0, f1), want):
            t_moved, t, inside = wr.tri_t32(face_tri(sc, f), s.rays[m, 0:3], s.rays[m, 3:6], near[m])
            assert (t == t_want).all() and (t_moved == t).all() and inside.all()

    tie = lane_nodes(sc, "tie")
    far_leaf = lane_nodes(sc, "far_box")[0]
    if anyhit:
        # a face at t == tLight exactly, one place nearer and one farther; a second leaf behind it shows whether the walk went on
        assert len(tie) == 2 and tie[1] > tie[0]
        for name, t_light in (("face_at_tlight", F(2)), ("face_at_tlight_up", wr.up(2)), ("face_at_tlight_down", wr.down(2))):
            m = c[name]
            near, _, _ = slabs(sc, s, tie[0])
            t_moved, t, inside = wr.tri_t32(face_tri(sc, int(bvh[tie[0], 3])), s.rays[m, 0:3], s.rays[m, 3:6], near[m])
            assert (t_moved == 2).all() and (t == 2).all() and inside.all() and (s.t0[m] == t_light).all()
        assert bits(wr.up(2)) - bits(F(2)) == 1 and bits(F(2)) - bits(wr.down(2)) == 1
        assert (s.t0[c["tlight_zero"]] == 0).all() and (0 < s.t0[c["tlight_below_eps"]]).all() and (s.t0[c["tlight_below_eps"]] < wr.EPSILON5).all()
        assert np.isinf(s.t0[c["tlight_inf"]]).all()
        # a box wholly behind the light, holding a face behind the light
        m = c["box_beyond_light"]
        near, far, _ = slabs(sc, s, far_leaf)
        assert (near[m] > s.t0[m]).all() and wr.box_hit32(near[m], far[m], s.t0[m], True).all()
        _, t, inside = wr.tri_t32(face_tri(sc, int(bvh[far_leaf, 3])), s.rays[m, 0:3], s.rays[m, 3:6], near[m])
        assert (t > s.t0[m]).all() and inside.all()
    else:
        # t0 == tNear of a box exactly (culled), one place above (entered) and one below
        cull = lane_nodes(sc, "cull")[0]
        near, far, _ = slabs(sc, s, cull)
        for name, t0, enters in (("t0_at_tnear", F(2), False), ("t0_at_tnear_up", wr.up(2), True), ("t0_at_tnear_down", wr.down(2), False)):
            m = c[name]
            assert (near[m] == 2).all() and (s.t0[m] == t0).all() and wr.box_hit32(near[m], far[m], s.t0[m], False).all() == enters
            assert wr.box_hit32(near[m], far[m], s.t0[m], True).all()
        # the same after a real hit: the face's t equals the later box's tNear
        first, later = lane_nodes(sc, "after_hit")
        m = c["hit_at_later_tnear"]
        near0, _, _ = slabs(sc, s, first)
        _, t, inside = wr.tri_t32(face_tri(sc, int(bvh[first, 3])), s.rays[m, 0:3], s.rays[m, 3:6], near0[m])
        near1, far1, _ = slabs(sc, s, later)
        assert later > first and (t == 2).all() and inside.all() and (near1[m] == t).all() and (far1[m] > near1[m]).all()
        m = c["box_beyond_light"]
        near, far, _ = slabs(sc, s, far_leaf)
        assert not wr.box_hit32(near[m], far[m], s.t0[m], False).any()

    if lights:
        # the orb lies on its lanes' rays and enters at 3.5 exactly; the front lane has a face behind it and, later, one in front
        orbs = sc.arrays["lights"]
        assert (orbs[:, 8] == 2).all() and (orbs[:, 9] == wr.ORB_R).all()
        front = lane_nodes(sc, "orb_front")
        m = c["orb_then_front"]
        t_orb, d2 = wr.sphere_near32(orbs[0, :3], wr.ORB_R, s.rays[m, 0:3], s.rays[m, 3:6])
        assert (t_orb == wr.ORB_NEAR).all() and (d2 == 0).all()
        xs = [float(face_tri(sc, int(bvh[n, 3]))[0, 0]) for n in front]
        assert xs == [6.0, 2.0] and front[1] > front[0]
        if anyhit:
            assert (t_orb < s.t0[m]).all() and (s.t0[m] < 6).all() and (s.t0[m] > 2).all()
            for name, t_light in (("orb_tie", wr.ORB_NEAR), ("orb_tie_up", wr.up(wr.ORB_NEAR)), ("orb_tie_down", wr.down(wr.ORB_NEAR))):
                m = c[name]
                t_orb, _ = wr.sphere_near32(orbs[1, :3], wr.ORB_R, s.rays[m, 0:3], s.rays[m, 3:6])
                assert (t_orb == wr.ORB_NEAR).all() and (s.t0[m] == t_light).all()
            # every other lane's ray passes the orbs at d2 > r
            others = ~(c["orb_then_front"] | c["orb_then_behind"] | c["orb_tie"] | c["orb_tie_up"] | c["orb_tie_down"])
            for orb in orbs:
                _, d2 = wr.sphere_near32(orb[:3], wr.ORB_R, s.rays[others, 0:3], s.rays[others, 3:6])
                assert (d2 > wr.ORB_R).all()


@pytest.mark.parametrize("anyhit", (False, True))
def test_chain_classes_hold_their_conditions(pbr, anyhit):
    """Lane i of the first wave hits the containers behind leaves 0 .. i - 1 and misses the next, whose miss link is -1."""
    sc, s = wr.chain_scene(pbr), wr.chain_rays(anyhit)
    bvh = sc.arrays["bvh"]
    lo, hi = node_boxes(sc)
    c = s.classes
    assert all(m.any() for m in c.values()) and bvh.shape[0] == 603
    assert np.nonzero(c["departures"])[0].tolist() == list(range(64)) and c["copies"].sum() == 64
    assert np.nonzero(c["long_walk"] | c["miss_node1"])[0].tolist() == list(range(64, 128)) and c["long_walk"].sum() == 1
    containers = np.nonzero(bvh[:, 3] == -1)[0][1:]          # behind leaf 0, 1, ...
    assert (bvh[containers, 7] == -1).all() and bvh[-1, 3] >= 0 and bvh[-2, 3] >= 0
    for i in (0, 1, 7, 63):
        ray = s.rays[np.nonzero(c["departures"])[0][i]]
        near, far, nans = wr.slab32(lo[containers], hi[containers], ray[None, 0:3], ray[None, 3:6])
        hit = wr.box_hit32(near, far, F(np.inf), anyhit)
        assert hit[:i].all() and not hit[i:].any() and (nans == 0).all()
    m = c["miss_node1"]
    near, far, _ = wr.slab32(lo[1], hi[1], s.rays[m, 0:3], s.rays[m, 3:6])
    assert not wr.box_hit32(near, far, s.t0[m], anyhit).any()
    # the long walk and the one that ends on the last record hit every container; the latter the last leaf too
    for name, last in (("long_walk", False), ("ends_on_last_record", True)):
        ray = s.rays[c[name]][0]
        near, far, _ = wr.slab32(lo[1:], hi[1:], ray[None, 0:3], ray[None, 3:6])
        hit = wr.box_hit32(near, far, F(np.inf), True)
        assert hit[containers - 1].all() and bool(hit[-1]) == last
    # leaf 0's face lies behind every other face on every ray, and in front of a light at 8 only
    tri0 = face_tri(sc, 0)
    for name in ("blocker_in_first_leaf", "blocker_in_last_leaf") if anyhit else ():
        m = c[name]
        t_moved, t, inside = wr.tri_t32(tri0, s.rays[m, 0:3], s.rays[m, 3:6], np.full(m.sum(), -1, np.float32))
        assert (t == 7).all() and inside.all() and ((t < s.t0[m]).all() == (name == "blocker_in_first_leaf"))


def test_rays_from_the_middle_start_inside_every_box(pbr):
    """... in both walks' sets; the any-hit set's tLight lies among the faces' distances: some rays blocked, some lit (the
    recording of the reference's own walks, refkernel_walk_inside_wide7.npz, shows both)."""
    sc = wr.inside_scene(pbr)
    lo, hi = node_boxes(sc)
    for anyhit in (False, True):
        s = wr.inside_all_rays(sc, anyhit)
        assert s.classes["inside_all"].all() and s.n == 64
        for ray in s.rays:
            near, far, nans = wr.slab32(lo[1:], hi[1:], ray[None, 0:3], ray[None, 3:6])
            assert (near < 0).all() and (far > wr.EPSILON5).all() and (nans == 0).all()
    rec = mk.recorded_walk("inside_wide7")
    blocked = rec["s_t"] < rec["s_tlight"]
    assert blocked.sum() >= 8 and (~blocked).sum() >= 8 and np.isfinite(rec["c_t"]).sum() >= 32
    assert (rec["c_counts"][:, 0] == sc.arrays["bvh"].shape[0] - 1).all()          # every node is entered


# ---- the oracle against the reference's compiled walks ------------------------------------------------------------------------

def oracle_walks(oracle, name):
    sc, rays = mk.walk_scene(name), mk.walk_rays_of(name)
    cfg = sc.config(traversal=0)
    ct, cface, _, ccounts = oracle.trace_rays(sc.desc, cfg, rays["c_rays"], rays["c_t0"])
    st, sface, _, scounts = oracle.trace_shadow_rays(sc.desc, cfg, rays["s_rays"], rays["s_tlight"])
    assert (scounts[:, 0] == 0).all()          # the shadow walk counts no node visits
    return dict(rays, c_t=ct, c_face=cface, c_counts=ccounts, s_t=st, s_face=sface, s_tests=scounts[:, 1])


def assert_same_walks(got, want, what):
    for k in ("c_rays", "c_t0", "s_rays", "s_tlight", "c_t", "s_t"):
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s %s: %s" % (what, k, describe_mismatch(got[k], want[k]))
    for k in ("c_face", "c_counts", "s_face", "s_tests"):
        assert np.array_equal(got[k], want[k]), "%s %s: %d rays differ" % (what, k, (np.asarray(got[k]) != np.asarray(want[k])).reshape(len(got[k]), -1).any(axis=1).sum())


@pytest.mark.parametrize("name", WALK_NAMES)
def test_the_oracle_reproduces_the_recorded_walks(pbr, oracle, name):
    """t as bits, face, node visits and face tests of both walks — and the recorded rays are the constructors' own."""
    rec = mk.recorded_walk(name)
    assert_same_walks(oracle_walks(oracle, name), rec, name)
    assert dict(zip(rec["values_keys"].tolist(), rec["values_values"].tolist())) == mk.walk_values_of(name)
    assert os.path.getsize(os.path.join(os.path.dirname(mk.__file__), "refkernel_walk_%s.npz" % name)) < mk.WALK_SIZE_CAP


def test_the_recorded_walks_show_what_the_classes_are_there_for(pbr):
    """On the reference's own outputs: where the walk stopped, what it recorded."""
    rec = mk.recorded_walk("lanes_lit")
    s = wr.lanes_rays(True, True)
    c, t, tests, t_light, face = s.classes, rec["s_t"], rec["s_tests"], rec["s_tlight"], rec["s_face"]
    blocked = t < t_light
    for name, want_blocked, want_tests in (
            ("two_faces_block", True, 2),            # the second face is tested after the first one blocked ...
            ("face_at_tlight", False, 2), ("face_at_tlight_up", True, 1), ("face_at_tlight_down", False, 2),
            ("tlight_zero", False, 2), ("tlight_below_eps", False, 2), ("tlight_inf", True, 1),
            ("box_beyond_light", False, 1),          # entered and tested, nothing recorded
            ("orb_then_front", True, 2), ("orb_then_behind", False, 1), ("orb_tie", False, 1), ("orb_tie_up", False, 1), ("orb_tie_down", False, 1),
            ("tfar_eps_flat_leaf", False, 0), ("tfar_eps_down_flat_leaf", False, 0), ("tfar_eps_up_flat_leaf", True, 1),
            ("tfar_eps_flat_container", False, 0), ("tfar_eps_down_flat_container", False, 0),
            ("nan1", False, 0), ("nan2", False, 0), ("flat_in_plane", False, 1), ("corner", False, 1)):
        assert (blocked[c[name]] == want_blocked).all() and (tests[c[name]] == want_tests).all(), name
    assert (t[c["two_faces_block"]] == 1).all()                                        # ... and kept: it lies nearer
    assert (t[c["orb_then_behind"]] == 6).all() and (t[c["orb_tie_up"]] == 6).all()    # finite, beyond the light: recorded after the orb reset t
    assert (t[c["orb_tie"]] == wr.ORB_NEAR).all() and (face[c["orb_tie"]] == 0).all()  # tNear < ray.t is strict: no reset on the tie
    assert (tests[c["tfar_eps_up_flat_container"]] >= 1).all()
    closest = mk.recorded_walk("lanes")
    s = wr.lanes_rays(False, False)
    c, tests, face = s.classes, closest["c_counts"][:, 1], closest["c_face"]
    assert tests[c["t0_at_tnear"]].tolist() == [0] and tests[c["t0_at_tnear_up"]].tolist() == [1] and tests[c["t0_at_tnear_down"]].tolist() == [0]
    assert tests[c["hit_at_later_tnear"]].tolist() == [1] and tests[c["box_beyond_light"]].tolist() == [0]
    bvh = wr.lanes_scene(pbr, False).arrays["bvh"]
    assert face[c["equal_t"]].tolist() == [int(bvh[lane_nodes(wr.lanes_scene(pbr, False), "equal_t")[0], 3])]     # the first of two equal t is kept
    chain = mk.recorded_walk("chain")
    s = wr.chain_rays(True)
    c, faces = s.classes, wr.chain_scene(pbr).leaf_faces
    assert (chain["s_tests"][c["blocker_in_first_leaf"]] == 1).all()
    entered = (s.rays[c["blocker_in_last_leaf"], 0] - 0.5).astype(int)
    assert chain["s_tests"][c["blocker_in_last_leaf"]].tolist() == [int(faces[:i + 1].sum()) for i in entered]
    lanes = np.arange(64)
    assert chain["c_counts"][:64, 0].tolist() == (2 * lanes + 2).tolist()              # lane i leaves in visit 2 i + 2


@needs_reference
def test_the_compiled_reference_equals_the_recorded_walks_and_the_oracle(pbr, oracle, tmp_path):
    assert refkernel.build_many([mk.walk_values_of(n) for n in WALK_NAMES]) is not None
    for name in WALK_NAMES:
        fresh = mk.walk_reference_outputs(name, str(tmp_path))
        assert_same_walks(fresh, mk.recorded_walk(name), name + " against the recording")
        assert_same_walks(oracle_walks(oracle, name), fresh, name + ", the oracle against a fresh run")
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("name", ("hand_leaf1", "hand_leaf1_box_edges", "hand_chain300", "plain_suzanne_sa_shadow"))
def test_the_closest_walk_is_unchanged_on_the_earlier_recordings(pbr, oracle, name):
    """orc_trace_rays through its new starting t, left at +inf, against what the reference's traverse recorded before."""
    import make_reference_scenes as mrs
    data, rec = mk.case_inputs(name), mk.recorded(name)
    desc, cfg, cam, keep = mrs.scene_from_fixture(pbr, data)
    for t0 in (None, np.inf, np.full(data["rays"].shape[0], np.inf, np.float32)):
        t, face, normal, counts = oracle.trace_rays(desc, cfg, data["rays"], t0)
        assert np.array_equal(bits(t), bits(rec["ray_t"])) and np.array_equal(face, rec["ray_face"]) and np.array_equal(counts, rec["ray_counts"])
        assert same_values(normal, rec["ray_normal"])


# ---- the random rays ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RANDOM_TREES)
def test_random_rays_are_decided_and_the_oracle_agrees(pbr, oracle, name):
    sc = random_scene(pbr, name)
    if name == "generated":
        assert 1500 <= sc.arrays["bvh"].shape[0] <= 2600
    rays, t_light = wr.random_set(sc)
    decided, blocked, t64, edge = wr.shadow_truth64(sc, rays, t_light)
    share = decided.mean()
    native_share = wr.shadow_truth64(sc, rays, t_light, wr.NATIVE_MARGIN)[0].mean()      # what tests/test_gpu_walk_rays.py decides the native arithmetic on
    print("%s: %d nodes, %d rays, decided %.4f (at the native margin %.4f), blocked %d, lit %d" % (
        name, sc.arrays["bvh"].shape[0], rays.shape[0], share, native_share, (decided & blocked).sum(), (decided & ~blocked).sum()))
    assert rays.shape[0] >= 2048 and share >= 0.95 and native_share >= 0.95
    assert (decided & blocked).sum() >= rays.shape[0] // 8 and (decided & ~blocked).sum() >= rays.shape[0] // 8
    for traversal in (0, 1, 2):
        t, face, _, counts = oracle.trace_shadow_rays(sc.desc, sc.config(traversal=traversal), rays, t_light)
        wrong = decided & ((t < t_light) != blocked)
        assert not wrong.any(), (name, traversal, np.nonzero(wrong)[0][:4].tolist())
