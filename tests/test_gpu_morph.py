"""pbr_set_morph / pbr_update_morph / pbr_update_pose on the GPU: the device's V' and N' equal the numpy restatement
(tests/morph_ref.py) bit for bit, everything behind them equals pbr_update_geometry( V', N' ) — boxes, patches, renders, single rays,
the ordered walks behind the re-link, the temporal history —, the pose is the skin of the morphed rest pose, the rest pose makes
the calls non-cumulative, and every refusal, the overflow found on the device included, leaves the context as it was.

The fixtures at their own size: the pillars' 40 vertices stay below one wave, Suzanne's 603 span three workgroups and are no
multiple of one.  Every fixture's targets (morph_ref.targets_for) hold an empty target, elements in 0, 1, 2, 3 and all other
targets, zero deltas and normal deltas that cancel the normal; Suzanne has one vertex with a run of 66 entries — longer than a
wave is wide — between neighbours with none; the dense variant adds a target that names every element."""
import ctypes
import types

import numpy as np
import pytest

import morph_ref
import patch_refit_ref
import refit_ref
import refit_scenes
import skin_ref
import transform_ref
from conftest import same_values, describe_mismatch
from test_gpu_patch_refit import assert_same_render, bits, rays_for, rendered, with_arrays
from test_gpu_transforms import ALPHA, FIXTURES, SHIFT, device, other, third, same_bits  # noqa: F401 (the three are fixtures)

pytestmark = pytest.mark.gpu

NO_MORPH = {"targets": 0, "vertex_entries": 0, "normal_entries": 0, "device_bytes": 0, "updates": 0, "last_update": 0, "ms": 0.0}
WEIGHTS = "zeros between"                                            # the weight set of the cases that need one
_cases = {}


def case(pbr, name, dense=False):
    """The fixture, its targets, the weight sets, the skin the pose tests use and the restatement's V', N' under WEIGHTS.
    Computed once per case and shared; nobody writes to the arrays."""
    key = (name, dense)
    if key not in _cases:
        sc = refit_scenes.load(pbr, name)
        a = sc.arrays
        c = types.SimpleNamespace(sc=sc, a=a)
        c.vt, c.nt = morph_ref.targets_for(name, a["vertices"], a["normals"], dense)
        c.sets = morph_ref.weights_for(len(c.vt))
        c.w = c.sets[WEIGHTS]
        c.v, c.n = morph_ref.morph(a["vertices"], c.vt, a["normals"], c.nt, c.w)
        c.vb, c.vw, c.nb, c.nw, c.bones = skin_ref.influences_for(name, a["facesV"], a["facesN"], a["vertices"].shape[0], a["normals"].shape[0])
        c.M = transform_ref.matrices_for(c.bones, SHIFT, ("translation of 1e6",))
        _cases[key] = c
    return _cases[key]


def entries(targets):
    return sum(np.asarray(t[0]).size for t in targets)


def info_of(c, with_normals=True, **more):
    v, n = c.a["vertices"].shape[0], c.a["normals"].shape[0]
    info = {"targets": len(c.vt), "vertex_entries": entries(c.vt), "normal_entries": entries(c.nt) if with_normals else 0,
            "device_bytes": morph_ref.expected_bytes(v, c.vt, n, c.nt if with_normals else None), "updates": 0, "last_update": 0, "ms": 0.0}
    info.update(more)
    return info


def geometry_is(device, v, n, what):
    got_v, got_n = device.read_geometry()
    same_bits(got_v, v, what + ": V'")
    same_bits(got_n, n, what + ": N'")


# ---- 1: the morph, the boxes and the patches against the restatements -------------------------------------------------------

@pytest.mark.parametrize("dense", (False, True))
@pytest.mark.parametrize("alpha", (ALPHA, 0.0))
@pytest.mark.parametrize("name", FIXTURES)
def test_morph_boxes_and_patches_equal_the_numpy_restatements(pbr, device, name, alpha, dense):
    c = case(pbr, name, dense)
    a = c.a
    assert not np.array_equal(bits(c.v), bits(a["vertices"])) and not np.array_equal(bits(c.n), bits(a["normals"]))
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=alpha))
    assert device.morph_info() == NO_MORPH
    device.set_morph(c.vt, c.nt)
    assert device.morph_info() == info_of(c)
    faces, normals = a["facesV"].shape[0], a["normals"].shape[0]
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 0, "last_update": False, "alpha": 0.0}
    device.update_morph(c.w)
    geometry_is(device, c.v, c.n, "update_morph")
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], c.v, c.n, alpha), "boxes")
    same_bits(device.read_patches(), patch_refit_ref.pack_patches(a["facesV"], a["facesN"], c.v, c.n), "patches")
    info = device.morph_info()
    assert info["ms"] > 0.0 and device.last_kernel_ms() >= info["ms"]
    assert dict(info, ms=0.0) == info_of(c, updates=1, last_update=1)
    assert device.skin_info()["last_update"] is False and device.transform_info()["last_update"] is False
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 1, "last_update": True,
                                         "alpha": float(np.float32(alpha))}
    assert device.refit_info()["updates"] == 1
    # every weight set, from the same rest pose
    for label, w in c.sets.items():
        device.update_morph(w)
        geometry_is(device, *morph_ref.morph(a["vertices"], c.vt, a["normals"], c.nt, w), label)
    # any other update is no morph update
    device.update_geometry(c.v, c.n)
    assert dict(device.morph_info(), ms=0.0) == info_of(c, updates=1 + len(c.sets), last_update=0)
    # dropping the morph frees it
    device.set_morph(None)
    assert device.morph_info()["targets"] == 0 and device.morph_info()["device_bytes"] == 0
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_morph"):
        device.update_morph(c.w)


# ---- 2: three contexts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", (0, 2, 3))
@pytest.mark.parametrize("name", FIXTURES)
def test_morphed_context_equals_update_geometry_and_a_fresh_upload(pbr, device, other, third, name, traversal):
    """A: set_morph + update_morph( w ).  B: update_geometry( V', N' ).  C: a fresh upload of S' with the nodes A reads back.
    Images, debug images, counters and 4096 single rays are equal; under an ordered walk the re-linked records of A and B are
    the same bytes."""
    c = case(pbr, name)
    cfg = c.sc.config(traversal=traversal, phong_tessellation=ALPHA)
    for dev in (device, other):
        dev.refit_ordered_walk(traversal != 0)
        dev.upload_scene(c.sc.desc)
        dev.configure(cfg)
    device.set_morph(c.vt, c.nt)
    device.update_morph(c.w)
    other.update_geometry(c.v, c.n)
    fresh = with_arrays(c.sc, vertices=c.v, normals=c.n, bvh=device.read_bvh())
    third.upload_scene(fresh.desc)
    third.configure(cfg)
    same_bits(device.read_bvh(), other.read_bvh(), "boxes of A and B")
    same_bits(device.read_patches(), other.read_patches(), "patches of A and B")
    same_bits(device.read_patches(), third.read_patches(), "patches of A and C")
    if traversal:
        assert device.relink_info()["relinked"] and other.relink_info()["relinked"]
        got, want = device.read_walk(), other.read_walk()
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    image = rendered(device, c.sc)
    assert_same_render(image, rendered(other, c.sc), "%s, traversal %d: A against B" % (name, traversal))
    assert_same_render(image, rendered(third, c.sc), "%s, traversal %d: A against C" % (name, traversal))
    assert image[2]["hits"] > 0
    rays = rays_for(c.v)
    mine = device.diag_trace(rays)
    assert np.isfinite(mine[0]).sum() > 200
    for theirs in (other.diag_trace(rays), third.diag_trace(rays)):
        for x, y in zip(mine, theirs):
            assert same_values(x, y)
    assert device.guard_trips() == [0, 0, 0]


# ---- 3: zero weights --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_zero_weights_give_the_rest_pose(pbr, device, other, name):
    c = case(pbr, name, dense=True)
    a = c.a
    for dev in (device, other):
        dev.upload_scene(c.sc.desc)
        dev.configure(c.sc.config(phong_tessellation=ALPHA))
    device.set_morph(c.vt, c.nt)
    device.update_morph(c.w)
    device.update_morph(c.sets["all zero"])
    other.update_geometry(a["vertices"], a["normals"])
    geometry_is(device, a["vertices"], a["normals"], "all weights 0")
    same_bits(device.read_bvh(), other.read_bvh(), "boxes")
    same_bits(device.read_patches(), other.read_patches(), "patches")
    assert_same_render(rendered(device, c.sc), rendered(other, c.sc), "all weights 0 against update_geometry( rest )")


# ---- 4: the rest pose -------------------------------------------------------------------------------------------------------

def test_morph_updates_start_from_the_rest_pose(pbr, device, other):
    """w1 then w2 leaves what w2 alone leaves on a fresh context; an update_vertices, an update_skin or an update_pose in between
    changes nothing of what the next morph update produces, and update_skin ignores the morph; set_morph after an
    update_geometry captures that pose."""
    c = case(pbr, "ref_suzanne_sa")
    a = c.a
    w1, w2 = c.sets["negative"], c.sets["above one"]
    want_v, want_n = morph_ref.morph(a["vertices"], c.vt, a["normals"], c.nt, w2)
    for dev in (device, other):
        dev.upload_scene(c.sc.desc)
        dev.configure(c.sc.config(phong_tessellation=0.0))
        dev.set_morph(c.vt, c.nt)
    device.update_morph(w1)
    device.update_morph(w2)
    other.update_morph(w2)
    geometry_is(device, want_v, want_n, "w1 then w2")
    geometry_is(other, want_v, want_n, "w2 alone")
    same_bits(device.read_bvh(), other.read_bvh())
    same_bits(device.read_patches(), other.read_patches())
    nodes = device.read_bvh()
    device.update_vertices(refit_ref.deform(a["facesV"], a["vertices"], "large", 7))
    device.update_morph(w2)
    geometry_is(device, want_v, want_n, "after an update_vertices in between")
    same_bits(device.read_bvh(), nodes)
    # a skin beside the morph, set on another pose: each call works from its own rest pose
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_skin(c.M)
    geometry_is(device, *skin_ref.skin(want_v, c.vb, c.vw, want_n, c.nb, c.nw, c.M), "update_skin ignores the morph")
    assert device.skin_info()["last_update"] and device.morph_info()["last_update"] == 0
    device.update_morph(w2)
    geometry_is(device, want_v, want_n, "update_morph ignores the skin")
    assert not device.skin_info()["last_update"] and device.morph_info()["last_update"] == 1
    # a new rest pose — the one an update_geometry left
    device.update_geometry(c.v, c.n)
    device.set_morph(c.vt, c.nt)
    assert device.morph_info()["updates"] == 0
    device.update_morph(w1)
    again_v, again_n = morph_ref.morph(c.v, c.vt, c.n, c.nt, w1)
    geometry_is(device, again_v, again_n, "from the captured pose")
    assert not np.array_equal(bits(again_v), bits(morph_ref.positions(a["vertices"], c.vt, w1)))


# ---- 5: the pose ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_pose_is_the_skin_of_the_morphed_rest_pose(pbr, device, other, name):
    c = case(pbr, name)
    a = c.a
    cfg = c.sc.config(phong_tessellation=ALPHA)
    want_v, want_n = skin_ref.skin(c.v, c.vb, c.vw, c.n, c.nb, c.nw, c.M)
    device.upload_scene(c.sc.desc)
    device.configure(cfg)
    device.set_morph(c.vt, c.nt)
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_morph(c.w)
    morphed_nodes = device.read_bvh()                                # of A's morphed geometry: what the second context uploads
    device.update_pose(c.w, c.M)                                     # not cumulative: from the rest pose again
    geometry_is(device, want_v, want_n, "update_pose against the restatements")
    info = device.morph_info()
    assert info["ms"] > 0.0 and dict(info, ms=0.0) == info_of(c, updates=2, last_update=2)
    assert not device.skin_info()["last_update"] and device.skin_info()["updates"] == 0
    # a second context, uploaded with the morphed geometry, skinned
    moved = with_arrays(c.sc, vertices=c.v, normals=c.n, bvh=morphed_nodes)
    other.upload_scene(moved.desc)
    other.configure(cfg)
    other.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    other.update_skin(c.M)
    geometry_is(other, want_v, want_n, "set_skin + update_skin over the morphed upload")
    same_bits(device.read_bvh(), other.read_bvh(), "boxes")
    same_bits(device.read_patches(), other.read_patches(), "patches")
    assert_same_render(rendered(device, c.sc), rendered(other, c.sc), "pose against the skin of the morphed upload")
    # zero weights: the skin alone
    device.update_pose(c.sets["all zero"], c.M)
    other.upload_scene(c.sc.desc)
    other.configure(cfg)
    other.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    other.update_skin(c.M)
    geometry_is(device, *other.read_geometry(), "update_pose( 0, M ) against update_skin( M )")
    geometry_is(device, *skin_ref.skin(a["vertices"], c.vb, c.vw, a["normals"], c.nb, c.nw, c.M), "update_pose( 0, M )")
    same_bits(device.read_bvh(), other.read_bvh(), "boxes")
    # one-hot identity bones: the morph alone
    device.upload_scene(c.sc.desc)
    device.configure(cfg)
    device.set_morph(c.vt, c.nt)
    device.set_skin(*skin_ref.one_hot(np.zeros(a["vertices"].shape[0], np.uint32)), *skin_ref.one_hot(np.zeros(a["normals"].shape[0], np.uint32)), 1)
    device.update_pose(c.w, transform_ref.IDENTITY[None])
    geometry_is(device, c.v, c.n, "update_pose( w, one-hot identity bones )")
    other.upload_scene(c.sc.desc)
    other.configure(cfg)
    other.set_morph(c.vt, c.nt)
    other.update_morph(c.w)
    same_bits(device.read_bvh(), other.read_bvh(), "boxes")
    same_bits(device.read_patches(), other.read_patches(), "patches")
    # the mixed normals: a skin without normal influences morphs them only, a morph without normal targets skins them only
    device.upload_scene(c.sc.desc)
    device.configure(cfg)
    device.set_morph(c.vt, c.nt)
    device.set_skin(c.vb, c.vw, None, None, c.bones)
    device.update_pose(c.w, c.M)
    geometry_is(device, want_v, c.n, "no normal influences")
    device.upload_scene(c.sc.desc)
    device.configure(cfg)
    device.set_morph(c.vt)
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_pose(c.w, c.M)
    geometry_is(device, want_v, skin_ref.normals(a["normals"], c.nb, c.nw, c.M), "no normal targets")


# ---- 6: without normal targets, without usable normals ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ("ref_spheres_schlick", "ref_suzanne_sa"))
def test_without_normal_targets_the_context_s_normals_stay(pbr, device, other, name):
    c = case(pbr, name)
    a = c.a
    cfg = c.sc.config(phong_tessellation=ALPHA)
    kept = patch_refit_ref.perturb_normals(a["normals"], seed=2)
    for dev in (device, other):
        dev.upload_scene(c.sc.desc)
        dev.configure(cfg)
        dev.update_geometry(a["vertices"], kept)                      # the normals the context holds from now on
    device.set_morph(c.vt)
    assert device.morph_info() == info_of(c, with_normals=False)
    device.update_morph(c.w)
    other.update_geometry(c.v)
    geometry_is(device, c.v, kept, "positions alone")
    same_bits(device.read_patches(), patch_refit_ref.pack_patches(a["facesV"], a["facesN"], c.v, kept))
    same_bits(device.read_bvh(), other.read_bvh())
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], c.v, kept, ALPHA))


def test_scene_without_usable_normals_takes_vertex_targets_only(pbr, device):
    c = case(pbr, "ref_pillars_sa")
    bare = with_arrays(c.sc)
    bare.desc.facesN, bare.desc.normals, bare.desc.num_normals = None, None, 0
    device.upload_scene(bare.desc)
    with pytest.raises(pbr.PbrError, match="-1: .*names normal .*the uploaded scene has 0"):
        device.set_morph(c.vt, c.nt)
    # normals there, indices out of range: the count matches, the scene has no patches — PBR_ESTATE
    broken = with_arrays(c.sc)
    wild = c.a["facesN"].copy()
    wild[0, 0] = c.a["normals"].shape[0]
    broken.arrays["facesN"] = wild
    broken.desc.facesN = wild.ctypes.data
    device.upload_scene(broken.desc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_morph: .*without usable vertex normals"):
        device.set_morph(c.vt, c.nt)
    assert device.morph_info() == NO_MORPH
    device.set_morph(c.vt)
    device.update_morph(c.w)
    same_bits(device.read_geometry()[0], c.v)
    same_bits(device.read_bvh(), refit_ref.refit(c.a["bvh"], c.a["facesV"], c.v))


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_as_it_was(pbr, device):
    c = case(pbr, "ref_suzanne_sa")
    a, w, M = c.a, c.w, c.M
    targets = len(c.vt)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_morph before pbr_upload_scene"):
        device.set_morph(c.vt, c.nt)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_morph"):
        device.update_morph(w)
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_morph without a morph: pbr_set_morph"):
        device.update_morph(w)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_pose without a morph: pbr_set_morph"):
        device.update_pose(w, M)
    set_morph = pbr.hip.pbr_set_morph
    vf, vi, vd = morph_ref.lists(c.vt)
    nf, ni, nd = morph_ref.lists(c.nt)

    def raw(*arrays, count=targets, ctx=True):
        return set_morph(device._ctx if ctx else None, *[None if x is None else x.ctypes.data for x in arrays], count)

    def own_refusals():
        """pbr_set_morph's own, in the header's order."""
        assert raw(vf, vi, vd, nf, ni, nd, ctx=False) == -1
        assert raw(vf, vi, vd, None, None, None, count=0) == -1
        assert raw(None, vi, vd, nf, ni, nd) == -1 and raw(vf, None, vd, nf, ni, nd) == -1 and raw(vf, vi, None, nf, ni, nd) == -1
        assert raw(vf, vi, vd, None, ni, nd) == -1 and raw(vf, vi, vd, nf, None, nd) == -1 and raw(vf, vi, vd, nf, ni, None) == -1
        bad = vf.copy()
        bad[0] = 1
        assert raw(bad, vi, vd, nf, ni, nd) == -1
        bad = nf.copy()
        bad[3] = bad[2] - 1
        assert bad[2] > 0 and raw(vf, vi, vd, bad, ni, nd) == -1
        wild = [(i.copy(), d) for i, d in c.vt]
        wild[2][0][5] = a["vertices"].shape[0]
        with pytest.raises(pbr.PbrError, match="-1: .*entry 5 of target 2 names vertex 603, the uploaded scene has 603"):
            device.set_morph(wild, c.nt)
        twice = [(i.copy(), d) for i, d in c.nt]
        twice[3][0][1] = twice[3][0][0]
        with pytest.raises(pbr.PbrError, match="-1: .*target 3 names normal %d twice" % twice[3][0][0]):
            device.set_morph(c.vt, twice)
        for value in (np.nan, np.inf):
            broken = [(i, d.copy()) for i, d in c.vt]
            broken[4][1][7, 1] = value
            with pytest.raises(pbr.PbrError, match="-1: .*the vertex delta of entry 7 of target 4 is not finite"):
                device.set_morph(broken, c.nt)

    own_refusals()
    assert device.morph_info() == NO_MORPH

    device.set_morph(c.vt, c.nt)
    device.update_morph(c.sets["dyadic"])
    before = rendered(device, c.sc)
    geometry, nodes, patches = device.read_geometry(), device.read_bvh(), device.read_patches()
    refits = [1]

    def unchanged(what):
        geometry_is(device, geometry[0], geometry[1], what)
        same_bits(device.read_bvh(), nodes, what)
        same_bits(device.read_patches(), patches, what)
        assert_same_render(rendered(device, c.sc), before, what)
        assert device.morph_info()["updates"] == 1 and device.morph_info()["targets"] == targets and device.refit_info()["updates"] == refits[0], what

    # a refused pbr_set_morph keeps the morph that was set
    own_refusals()
    unchanged("a refused pbr_set_morph")
    update, pose = pbr.hip.pbr_update_morph, pbr.hip.pbr_update_pose
    assert update(None, w.ctypes.data, targets) == -1 and pose(None, w.ctypes.data, targets, M.ctypes.data, c.bones) == -1
    assert update(device._ctx, None, targets) == -1
    unchanged("null weights")
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_morph: %d weights, pbr_set_morph declared %d targets" % (targets - 1, targets)):
        device.update_morph(w[:-1])
    unchanged("another target count")
    for bad in (np.nan, np.inf):
        x = w.copy()
        x[3] = bad
        with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_morph: the weight of target 3 is not finite"):
            device.update_morph(x)
        unchanged("a weight that is not finite")
    # the pose: no skin; then a skin that captured another generation (the update above lies between the two set calls)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_pose without a skin: pbr_set_skin"):
        device.update_pose(w, M)
    unchanged("a pose without a skin")
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_pose: pbr_set_skin and pbr_set_morph captured different geometry"):
        device.update_pose(w, M)
    unchanged("a pose over two generations")
    # both on one generation: the pose's own argument checks
    device.set_morph(c.vt, c.nt)                                     # captures the MORPHED pose, as the skin just did
    device.update_morph(c.sets["all zero"])                          # which is what the context holds; later updates do not part the two
    refits[0] += 1
    unchanged("zero weights over the captured pose")
    assert pose(device._ctx, None, targets, M.ctypes.data, c.bones) == -1 and pose(device._ctx, w.ctypes.data, targets, None, c.bones) == -1
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose: %d weights" % (targets - 1)):
        device.update_pose(w[:-1], M)
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose: 6 matrices, pbr_set_skin declared 7 bones"):
        device.update_pose(w, M[:-1])
    m = M.copy()
    m[3, 11] = np.nan
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose: word 11 of bone 3's matrix is not finite"):
        device.update_pose(w, m)
    x = w.copy()
    x[0] = np.inf
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose: the weight of target 0 is not finite"):     # the weights before the matrices
        device.update_pose(x, m)
    unchanged("the pose's argument checks")
    # finite deltas near 3e38 under weight 2: found on the device.  The rest pose is the captured one, so a morph of its own
    huge = [(np.array([17], np.uint32), np.array([[3e38, 0.0, 0.0]], np.float32)), (np.array([400, 17], np.uint32), np.array([[0.0, -3e38, 0.0], [1.0, 0.0, 0.0]], np.float32))]
    device.set_morph(huge)
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    rest = device.read_geometry()[0]
    for weights in ((2.0, 0.0), (0.0, 2.0), (1.5, 1.5)):
        weights = np.array(weights, np.float32)
        assert morph_ref.not_finite(morph_ref.positions(rest, huge, weights)).any()
        with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_morph: a morphed position is not finite"):
            device.update_morph(weights)
        with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose: a posed position is not finite"):
            device.update_pose(weights, M)
        geometry_is(device, geometry[0], geometry[1], "an overflow found on the device")
        same_bits(device.read_bvh(), nodes)
        assert_same_render(rendered(device, c.sc), before, "an overflow found on the device")
        assert device.morph_info()["updates"] == 0 and device.refit_info()["updates"] == refits[0]
    small = np.array([2e-38, 2e-38], np.float32)                     # and the same morph works under weights that fit
    device.update_morph(small)
    same_bits(device.read_geometry()[0], morph_ref.positions(rest, huge, small))
    assert device.read_geometry()[0][17, 0] == rest[17, 0] + np.float32(2e-38) * np.float32(3e38)
    # pbr_update_geometry's own: an ordered traversal without pbr_refit_ordered_walk
    device.configure(c.sc.config(traversal=2, phong_tessellation=ALPHA))
    held = device.read_geometry()
    for call, arguments in ((device.update_morph, (np.zeros(2, np.float32),)), (device.update_pose, (np.zeros(2, np.float32), M))):
        with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_(morph|pose) while a ray-ordered traversal"):
            call(*arguments)
        geometry_is(device, held[0], held[1], "ordered traversal")
    # set_morph( None ) frees it; a new upload drops it
    device.set_morph(None)
    assert device.morph_info() == dict(NO_MORPH, last_update=1)
    device.set_morph(c.vt, c.nt)
    device.upload_scene(c.sc.desc)
    assert device.morph_info() == NO_MORPH and device.skin_info()["bones"] == 0
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_morph"):
        device.update_morph(w)
    same_bits(device.read_geometry()[0], a["vertices"])


def test_not_nested_tree_takes_a_morph_but_no_update(pbr, device):
    from test_scene_pack_cpu import hand_tree, NOT_NESTED
    desc, keep = hand_tree(pbr, NOT_NESTED)
    vertices = keep[0].arrays()["vertices"]
    device.upload_scene(desc)
    device.set_morph([(np.arange(vertices.shape[0]), np.full((vertices.shape[0], 3), 0.25, np.float32))])
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_morph: .*not properly nested"):
        device.update_morph([1.0])
    same_bits(device.read_geometry()[0], vertices)
    same_bits(device.read_bvh(), keep[1])


# ---- 8: the temporal history ------------------------------------------------------------------------------------------------

def test_temporal_history_follows_a_morph_update_as_it_follows_update_vertices(pbr, device, other):
    """track_motion on; adaptive render + temporal call; move the tall block of the Cornell box; render + temporal call: with
    update_morph( one target that names the block's vertices ) on one context and update_vertices( V' ) on the other,
    `integrated`, `history` and the motion planes are the same bits, and faces no target names report code 1 (UNMOVED)."""
    from test_gpu_temporal import cornell, view, MOVE
    from test_gpu_temporal_motion import step, tall_block, BLOCK_MOVE
    steps = []
    for dev in (device, other):
        sc, cfg, px = cornell(pbr, dev)
        arrays = sc.arrays()
        material, mask = tall_block(arrays)
        block = np.flatnonzero(mask)
        targets = [(np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)), (block, np.tile(np.asarray(BLOCK_MOVE, np.float32) * np.float32(2.0), (block.size, 1)))]
        weights = np.array([3.0, 0.5], np.float32)
        V = morph_ref.positions(arrays["vertices"], targets, weights)
        assert np.array_equal(bits(V[~mask]), bits(arrays["vertices"][~mask])) and not np.array_equal(V[mask], arrays["vertices"][mask])
        dev.temporal_track_motion(True)
        first = step(pbr, dev, px, view(pbr, sc), 0)
        if dev is device:
            dev.set_morph(targets)
            dev.update_morph(weights)
            same_bits(dev.read_geometry()[0], V)
        else:
            dev.update_vertices(V)
        steps.append((first, step(pbr, dev, px, view(pbr, sc, **MOVE), 100, motion=True)))
    (a0, a1), (b0, b1) = steps
    for s, t in ((a0, b0), (a1, b1)):
        assert same_values(s.integrated, t.integrated), describe_mismatch(s.integrated, t.integrated)
        assert same_values(s.history, t.history), describe_mismatch(s.history, t.history)
    assert same_values(a1.motion, b1.motion) and np.array_equal(a1.face, b1.face)
    faces = arrays["facesV"]
    hit = a1.face >= 0
    on_block = hit & (faces[np.where(hit, a1.face, 0), 3] == material)
    code = a1.motion[..., 3]
    assert on_block.any() and (code[on_block] == 2).all() and (hit & ~on_block).any() and (code[hit & ~on_block] == 1).all()


# ---- 9: the tracer ----------------------------------------------------------------------------------------------------------

def test_path_tracer_forwards_the_calls(pbr, gpu_device):
    """PathTracer::setMorph / updateMorph / updatePose: the tracer's frames of the morphed and of the posed scene against a
    context driven by hand."""
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    scene = pbr.HostScene.generate("cornell", 1, 0)
    arrays = scene.arrays()
    count = arrays["vertices"].shape[0]
    rng = np.random.default_rng(17)
    targets = [(np.arange(0, count, 2), rng.uniform(-0.05, 0.05, (len(range(0, count, 2)), 3)).astype(np.float32)),
               (np.arange(count), rng.uniform(-0.05, 0.05, (count, 3)).astype(np.float32))]
    weights = np.array([0.75, -0.5], np.float32)
    bones = np.tile(np.array([0, 1, 1, 0], np.uint32), (count, 1))
    blend = np.where((np.arange(count) % 2 == 0)[:, None], np.array([0.5, 0.5, 0.0, 0.0], np.float32), np.array([0.0, 0.25, 0.0, 0.75], np.float32))
    M = np.stack([transform_ref.IDENTITY, transform_ref.MATRICES[4]])
    morphed = morph_ref.positions(arrays["vertices"], targets, weights)
    posed = skin_ref.positions(morphed, bones, blend, M)
    assert not np.array_equal(bits(morphed), bits(arrays["vertices"])) and not np.array_equal(bits(posed), bits(morphed))
    pt = pbr.PathTracer(gpu_device, 32, 32)
    pt.initOpenCLBuffers(scene)
    pt.setMorph(targets)
    pt.setSkin(bones, blend)
    dev = pbr.Device(gpu_device)
    dev.upload_scene(scene.desc)
    dev.configure(scene.config(32, 32))
    for call, moved in ((lambda: pt.updateMorph(weights), morphed), (lambda: pt.updatePose(weights, M), posed)):
        call()
        assert pt.sampleCount() == 0
        got = pt.generateImages(2)
        cam = pbr.Camera()
        pbr.host.pbrh_pt_camera(pt._h, ctypes.byref(cam))            # the camera the tracer rendered these frames with
        dev.update_geometry(moved)
        dev.reset_accum()
        dev.render(0, pbr.frame_seeds(0, 2), pbr.pixel_dimension(32, 32), cam)
        assert same_values(got, dev.read_output())
    pbr.cfg_reset()
    dev.close()
    pt.close()
