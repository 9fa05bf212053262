"""pbr_update_skin_dq / pbr_update_pose_dq on the GPU: the device's V' and N' equal the numpy restatement (tests/skin_dq_ref.py)
bit for bit, everything behind them equals pbr_update_geometry( V', N' ) — boxes, patches, renders, single rays, the ordered walks
behind the re-link, the temporal history —, the pose is the dq skin of the morphed rest pose, identity bones leave the rest pose,
the rest pose makes the calls non-cumulative, a bone's sign changes no bit, every refusal, the overflow found on the device
included, leaves the context as it was, and a twisting ring keeps the radius the matrix skin loses.

The fixtures at their own size: the pillars' 40 vertices stay below one wave, Suzanne's 603 span three workgroups and are no
multiple of one.  The influences are the matrix skin's (skin_ref.influences_for), the bones skin_dq_ref.dual_quats_for's: an
identity and its negation, a turn of more than 180 degrees, a bone that is not of unit length, translations, rotations."""
import ctypes
import types

import numpy as np
import pytest

import patch_refit_ref
import refit_scenes
import skin_dq_ref
import skin_ref
import transform_ref
from conftest import same_values, describe_mismatch
from test_gpu_patch_refit import assert_same_render, bits, rays_for, rendered, with_arrays
from test_gpu_transforms import ALPHA, FIXTURES, SHIFT, device, other, third, same_bits  # noqa: F401 (the three are fixtures)
from test_gpu_skin import expected_bytes, geometry_is
from test_gpu_morph import case as morph_case

pytestmark = pytest.mark.gpu

NO_DQ = {"updates": 0, "last_update": 0, "ms": 0.0}
FAR = ("translation of 1e6",)
EPS = 2.0 ** -23
_cases = {}


def case(pbr, name, shift=SHIFT, skip=()):
    """The fixture, its influences, a dealing of the bone set over the bones and the restatement's V', N'.  Computed once per
    case and shared; nobody writes to the arrays."""
    key = (name, shift, skip)
    if key not in _cases:
        sc = refit_scenes.load(pbr, name)
        a = sc.arrays
        c = types.SimpleNamespace(sc=sc, a=a)
        c.vb, c.vw, c.nb, c.nw, c.bones = skin_ref.influences_for(name, a["facesV"], a["facesN"], a["vertices"].shape[0], a["normals"].shape[0])
        c.Q = skin_dq_ref.dual_quats_for(c.bones, shift, skip)
        c.v, c.n = skin_dq_ref.skin(a["vertices"], c.vb, c.vw, a["normals"], c.nb, c.nw, c.Q)
        _cases[key] = c
    return _cases[key]


def dq_info(device):
    return dict(device.skin_dq_info(), ms=0.0)


# ---- 1: the skin, the boxes and the patches against the restatements --------------------------------------------------------

@pytest.mark.parametrize("alpha", (ALPHA, 0.0))
@pytest.mark.parametrize("name", FIXTURES)
def test_dq_skin_boxes_and_patches_equal_the_numpy_restatements(pbr, device, name, alpha):
    c = case(pbr, name)
    a = c.a
    assert not np.array_equal(bits(c.v), bits(a["vertices"])) and not np.array_equal(bits(c.n), bits(a["normals"]))
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=alpha))
    assert device.skin_dq_info() == NO_DQ
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    skin = device.skin_info()
    assert skin == {"bones": c.bones, "device_bytes": expected_bytes(c), "updates": 0, "last_update": False, "ms": 0.0} and device.skin_dq_info() == NO_DQ
    device.update_skin_dq(c.Q)
    geometry_is(device, c.v, c.n, "update_skin_dq")
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], c.v, c.n, alpha), "boxes")
    same_bits(device.read_patches(), patch_refit_ref.pack_patches(a["facesV"], a["facesN"], c.v, c.n), "patches")
    info = device.skin_dq_info()
    assert info["ms"] > 0.0 and device.last_kernel_ms() >= info["ms"]
    assert dict(info, ms=0.0) == {"updates": 1, "last_update": 1, "ms": 0.0}
    # to the matrix skin's report a dq update is another kind, and the call allocated nothing
    assert device.skin_info() == skin
    faces, normals = a["facesV"].shape[0], a["normals"].shape[0]
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 1, "last_update": True,
                                         "alpha": float(np.float32(alpha))}
    assert device.refit_info()["updates"] == 1
    device.configure(c.sc.config(phong_tessellation=alpha))          # the state rule: a pbr_update_geometry under this alpha
    # any other update is no dq update; the count stays
    device.update_skin(transform_ref.matrices_for(c.bones, 1))
    assert dq_info(device) == {"updates": 1, "last_update": 0, "ms": 0.0} and device.skin_info()["updates"] == 1 and device.skin_info()["last_update"]
    device.update_skin_dq(c.Q)
    geometry_is(device, c.v, c.n, "update_skin_dq behind an update_skin")
    assert dq_info(device) == {"updates": 2, "last_update": 1, "ms": 0.0} and not device.skin_info()["last_update"]
    # a new skin starts the count again; dropping the skin refuses the call
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    assert device.skin_dq_info() == dict(NO_DQ, last_update=1)
    device.set_skin(None)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_skin_dq without a skin: pbr_set_skin"):
        device.update_skin_dq(c.Q)


# ---- 2: three contexts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", (0, 2, 3))
@pytest.mark.parametrize("name", FIXTURES)
def test_dq_skinned_context_equals_update_geometry_and_a_fresh_upload(pbr, device, other, third, name, traversal):
    """A: set_skin + update_skin_dq( Q ).  B: update_geometry( V', N' ).  C: a fresh upload of S' with the nodes A reads back.
    Images, debug images, counters and 4096 single rays are equal; under an ordered walk the re-linked records of A and B are
    the same bytes."""
    c = case(pbr, name, skip=FAR)
    cfg = c.sc.config(traversal=traversal, phong_tessellation=ALPHA)
    for dev in (device, other):
        dev.refit_ordered_walk(traversal != 0)
        dev.upload_scene(c.sc.desc)
        dev.configure(cfg)
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_skin_dq(c.Q)
    geometry_is(device, c.v, c.n, "update_skin_dq")
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


# ---- 3: the pose ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_pose_dq_is_the_dq_skin_of_the_morphed_rest_pose(pbr, device, other, name):
    m = morph_case(pbr, name)                                         # test_gpu_morph's targets, weights and influences
    a = m.a
    Q = skin_dq_ref.dual_quats_for(m.bones, SHIFT, FAR)
    for dev in (device, other):
        dev.upload_scene(m.sc.desc)
        dev.configure(m.sc.config(phong_tessellation=ALPHA))
        dev.set_skin(m.vb, m.vw, m.nb, m.nw, m.bones)
    device.set_morph(m.vt, m.nt)
    morph = device.morph_info()
    want_v, want_n = skin_dq_ref.pose(a["vertices"], m.vt, m.vb, m.vw, a["normals"], m.nt, m.nb, m.nw, m.w, Q)
    assert not np.array_equal(bits(want_v), bits(skin_dq_ref.positions(a["vertices"], m.vb, m.vw, Q)))
    device.update_pose_dq(m.sets["above one"], Q)
    device.update_pose_dq(m.w, Q)                                     # not cumulative: from the rest pose again
    geometry_is(device, want_v, want_n, "update_pose_dq against the restatements")
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], want_v, want_n, ALPHA), "boxes")
    assert dq_info(device) == {"updates": 2, "last_update": 2, "ms": 0.0} and device.skin_dq_info()["ms"] > 0.0
    assert device.morph_info() == morph and not device.skin_info()["last_update"] and device.skin_info()["updates"] == 0
    # without morph weights it is the dq skin
    device.update_pose_dq(m.sets["all zero"], Q)
    other.update_skin_dq(Q)
    geometry_is(device, *other.read_geometry(), "update_pose_dq( 0, Q ) against update_skin_dq( Q )")
    geometry_is(device, *skin_dq_ref.skin(a["vertices"], m.vb, m.vw, a["normals"], m.nb, m.nw, Q), "update_pose_dq( 0, Q )")
    same_bits(device.read_bvh(), other.read_bvh(), "boxes")
    same_bits(device.read_patches(), other.read_patches(), "patches")
    # with identity bones, under the fixture's weights, it is the morph
    identities = np.tile(skin_dq_ref.IDENTITY, (m.bones, 1))
    identities[1::2] = -identities[1::2]
    device.update_pose_dq(m.w, identities)
    geometry_is(device, m.v, m.n, "update_pose_dq( w, identity bones )")
    device.update_morph(m.w)
    geometry_is(device, m.v, m.n, "update_morph( w )")
    assert dq_info(device) == {"updates": 4, "last_update": 0, "ms": 0.0} and device.morph_info()["last_update"] == 1
    # a morph without normal targets under a skin with normal influences: the normals are dq-skinned unmorphed
    device.upload_scene(m.sc.desc)
    device.configure(m.sc.config(phong_tessellation=ALPHA))
    device.set_skin(m.vb, m.vw, m.nb, m.nw, m.bones)
    device.set_morph(m.vt)
    device.update_pose_dq(m.w, Q)
    geometry_is(device, want_v, skin_dq_ref.normals(a["normals"], m.nb, m.nw, Q), "no normal targets")


# ---- 4: identity bones, the rest pose, the sign of a bone -------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_identity_bones_the_rest_pose_and_the_sign_of_a_bone(pbr, device, name):
    """Identity bones under the fixture's weights — 0.4 + 0.3 + 0.2 + 0.1 and 0.7 + 0.6 among them, which the matrix skin does
    not promise — leave read_geometry at the rest pose bit for bit; Q then Q2 equals Q2 alone; negating one bone changes no bit."""
    c = case(pbr, name)
    a = c.a
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    patches = device.read_patches()
    identities = np.tile(skin_dq_ref.IDENTITY, (c.bones, 1))
    identities[::2] = -identities[::2]
    device.update_skin_dq(skin_dq_ref.dual_quats_for(c.bones, 5))
    device.update_skin_dq(identities)
    geometry_is(device, a["vertices"], a["normals"], "identity bones")
    same_bits(device.read_patches(), patches, "patches under identity bones")
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], a["vertices"], a["normals"], ALPHA), "boxes under identity bones")
    device.update_skin_dq(c.Q)
    geometry_is(device, c.v, c.n, "Q1 then Q2")
    for b, w in ((c.vb, c.vw), (c.nb, c.nw)):
        assert not (skin_dq_ref.hemisphere_dots(b, w, c.Q) == 0).any()
    used = int(c.vb[c.vw != 0].max())
    for k in (0, used):
        flipped = c.Q.copy()
        flipped[k] = -flipped[k]
        device.update_skin_dq(flipped)
        geometry_is(device, c.v, c.n, "bone %d negated" % k)
    # a new rest pose — the one the last update left
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    Q = skin_dq_ref.dual_quats_for(c.bones, 4, FAR)
    device.update_skin_dq(Q)
    geometry_is(device, *skin_dq_ref.skin(c.v, c.vb, c.vw, c.n, c.nb, c.nw, Q), "from the captured pose")


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_as_it_was(pbr, device):
    c = case(pbr, "ref_suzanne_sa", skip=FAR)
    m = morph_case(pbr, "ref_suzanne_sa")
    a, Q = c.a, c.Q
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_skin_dq without a skin: pbr_set_skin"):
        device.update_skin_dq(Q)
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_skin_dq without a skin: pbr_set_skin"):
        device.update_skin_dq(Q)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_pose_dq without a morph: pbr_set_morph"):
        device.update_pose_dq(m.w, Q)
    device.set_morph(m.vt, m.nt)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_pose_dq without a skin: pbr_set_skin"):
        device.update_pose_dq(m.w, Q)
    assert device.skin_dq_info() == NO_DQ
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_skin_dq(skin_dq_ref.dual_quats_for(c.bones, 1, FAR))
    before = rendered(device, c.sc)
    geometry, nodes, patches, counts = device.read_geometry(), device.read_bvh(), device.read_patches(), device.refit_info()["updates"]

    def unchanged(what):
        geometry_is(device, geometry[0], geometry[1], what)
        same_bits(device.read_bvh(), nodes, what)
        same_bits(device.read_patches(), patches, what)
        assert_same_render(rendered(device, c.sc), before, what)
        assert dq_info(device) == {"updates": 1, "last_update": 1, "ms": 0.0} and device.refit_info()["updates"] == counts, what
        assert device.skin_info()["updates"] == 0 and device.morph_info()["updates"] == 0, what

    # the skin captured the uploaded geometry, a second pbr_set_morph the moved one: two generations
    device.set_morph(m.vt, m.nt)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_pose_dq: pbr_set_skin and pbr_set_morph captured different geometry"):
        device.update_pose_dq(m.w, Q)
    unchanged("two generations")
    update = pbr.hip.pbr_update_skin_dq
    assert update(None, Q.ctypes.data, c.bones) == -1
    assert update(device._ctx, None, c.bones) == -1 and b"null dual_quats" in pbr.hip.pbr_last_error(device._ctx)
    unchanged("null dual_quats")
    with pytest.raises(pbr.PbrError, match="-1: .*6 dual quaternions, pbr_set_skin declared 7 bones"):
        device.update_skin_dq(Q[:-1])
    unchanged("another bone count")
    for bad in (np.nan, np.inf):
        q = Q.copy()
        q[3, 6] = bad
        with pytest.raises(pbr.PbrError, match="-1: .*word 6 of bone 3's dual quaternion is not finite"):
            device.update_skin_dq(q)
        unchanged("a word that is not finite")
    q = Q.copy()
    q[2, :4] = 0.0
    with pytest.raises(pbr.PbrError, match="-1: .*the real part of bone 2's dual quaternion is all 0"):
        device.update_skin_dq(q)
    unchanged("an all-zero real part")
    # finite words, a translation that is not: found on the device.  Bone 0 is one that elements follow alone
    q = Q.copy()
    q[0, 4:] = 3e38
    assert skin_dq_ref.refused(q, c.bones) is None and skin_dq_ref.not_finite(skin_dq_ref.positions(a["vertices"], c.vb, c.vw, q)).any()
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_skin_dq: a skinned position is not finite .*found on the device"):
        device.update_skin_dq(q)
    unchanged("an overflow found on the device")
    # pbr_update_geometry's own: an ordered traversal without pbr_refit_ordered_walk
    device.configure(c.sc.config(traversal=2, phong_tessellation=ALPHA))
    before = rendered(device, c.sc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_skin_dq while a ray-ordered traversal"):
        device.update_skin_dq(Q)
    unchanged("ordered traversal")
    # and the calls still work afterwards: the pose on one generation, with its own overflow message
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    device.update_skin_dq(Q)
    geometry_is(device, c.v, c.n, "after the refusals")
    device.upload_scene(c.sc.desc)
    assert device.skin_dq_info() == dict(NO_DQ, last_update=0) and device.skin_info()["bones"] == 0
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.set_morph(m.vt, m.nt)
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose_dq: .*weights, pbr_set_morph declared"):
        device.update_pose_dq(m.w[:-1], Q)
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose_dq: 6 dual quaternions"):
        device.update_pose_dq(m.w, Q[:-1])
    with pytest.raises(pbr.PbrError, match="-1: .*pbr_update_pose_dq: a posed position is not finite .*found on the device"):
        device.update_pose_dq(m.w, q)
    geometry_is(device, a["vertices"], a["normals"], "after a refused pose")
    assert device.skin_dq_info() == NO_DQ
    device.update_pose_dq(m.w, Q)
    geometry_is(device, *skin_dq_ref.pose(a["vertices"], m.vt, c.vb, c.vw, a["normals"], m.nt, c.nb, c.nw, m.w, Q), "the pose after the refusals")


# ---- 6: the temporal history ------------------------------------------------------------------------------------------------

def test_temporal_history_follows_a_dq_update_as_it_follows_update_geometry(pbr, device, other):
    """track_motion on; adaptive render + temporal call; move the tall block of the Cornell box; render + temporal call: with
    update_skin_dq( identity, translation ) under one-hot weights on one context and update_geometry( V' ) on the other,
    `integrated`, `history` and the motion planes are the same bits, the motion path is taken, and faces of the identity bone
    report code 1 (UNMOVED)."""
    from test_gpu_temporal import cornell, view, MOVE
    from test_gpu_temporal_motion import step, tall_block, BLOCK_MOVE
    steps = []
    for dev in (device, other):
        sc, cfg, px = cornell(pbr, dev)
        arrays = sc.arrays()
        material, mask = tall_block(arrays)
        bones, weights = skin_ref.one_hot(mask.astype(np.uint32))
        Q = np.stack([-skin_dq_ref.IDENTITY, skin_dq_ref.dual_quat((1.0, 0.0, 0.0), 0.0, BLOCK_MOVE)])
        V = skin_dq_ref.positions(arrays["vertices"], bones, weights, Q)
        assert np.array_equal(bits(V[~mask]), bits(arrays["vertices"][~mask])) and not np.array_equal(V[mask], arrays["vertices"][mask])
        dev.temporal_track_motion(True)
        first = step(pbr, dev, px, view(pbr, sc), 0)
        if dev is device:
            dev.set_skin(bones, weights)
            dev.update_skin_dq(Q)
            same_bits(dev.read_geometry()[0], V)
        else:
            dev.update_geometry(V)
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


# ---- 7: the twist -----------------------------------------------------------------------------------------------------------

def test_the_twist_keeps_its_radius_on_the_device(pbr, device):
    """Sixteen ring vertices at radius 1 appended to the pillars (no face uses them), blended half and half between the identity
    and a half turn about y: within 4 * 2^-23 of radius 1 after update_skin_dq, below 1e-6 after update_skin with the two
    equivalent matrices."""
    sc = refit_scenes.load(pbr, "ref_pillars_sa")
    count = sc.arrays["vertices"].shape[0]
    angle = np.arange(16) * (2.0 * np.pi / 16.0)
    ring = np.stack([np.cos(angle), np.full(16, 0.5), np.sin(angle), np.ones(16)], axis=1).astype(np.float32)
    scene = with_arrays(sc, vertices=np.concatenate([sc.arrays["vertices"], ring]))
    bones = np.zeros((count + 16, 4), np.uint32)
    weights = np.zeros((count + 16, 4), np.float32)
    weights[:count, 0] = 1.0
    bones[count:, 1], weights[count:, :2] = 1, 0.5
    Q = np.stack([skin_dq_ref.IDENTITY, skin_dq_ref.dual_quat((0.0, 1.0, 0.0), np.pi, (0.0, 0.0, 0.0))])
    M = np.stack([transform_ref.IDENTITY, transform_ref._matrix(np.diag([-1.0, 1.0, -1.0]), (0.0, 0.0, 0.0))])
    assert np.abs(skin_dq_ref.matrix_of(Q) - M).max() < 1e-7
    device.upload_scene(scene.desc)
    device.set_skin(bones, weights)
    device.update_skin_dq(Q)
    v = device.read_geometry()[0]
    same_bits(v, skin_dq_ref.positions(scene.arrays["vertices"], bones, weights, Q), "the ring under the dq skin")
    same_bits(v[:count], sc.arrays["vertices"], "the pillars")
    radius = np.sqrt(v[count:, 0].astype(np.float64) ** 2 + v[count:, 2].astype(np.float64) ** 2)
    assert (np.abs(radius - 1.0) <= 4 * EPS).all(), radius
    device.update_skin(M)
    v = device.read_geometry()[0]
    collapsed = np.sqrt(v[count:, 0].astype(np.float64) ** 2 + v[count:, 2].astype(np.float64) ** 2)
    assert (collapsed < 1e-6).all(), collapsed


# ---- 8: the tracer and the conversion ---------------------------------------------------------------------------------------

def test_path_tracer_forwards_the_calls(pbr, gpu_device):
    """PathTracer::updateSkinDQ: the tracer's frames of the skinned scene against a context driven by hand, the bones made by
    pbr.dual_quats_from_matrices from rigid matrices."""
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    scene = pbr.HostScene.generate("cornell", 1, 0)
    arrays = scene.arrays()
    count = arrays["vertices"].shape[0]
    bones = np.tile(np.array([0, 1, 1, 0], np.uint32), (count, 1))
    weights = np.where((np.arange(count) % 2 == 0)[:, None], np.array([0.5, 0.5, 0.0, 0.0], np.float32), np.array([0.0, 0.25, 0.0, 0.75], np.float32))
    Q = pbr.dual_quats_from_matrices(np.stack([transform_ref.IDENTITY, transform_ref._matrix(transform_ref._rotation((0.0, 1.0, 0.0), 0.2), (0.05, 0.0, -0.05))]))
    assert np.array_equal(bits(Q[0]), bits(skin_dq_ref.IDENTITY))
    with pytest.raises(pbr.PbrError, match="bone 1's matrix is not a rotation"):
        pbr.dual_quats_from_matrices(transform_ref.MATRICES[[0, 4]])
    pt = pbr.PathTracer(gpu_device, 32, 32)
    pt.initOpenCLBuffers(scene)
    pt.setSkin(bones, weights)
    pt.updateSkinDQ(Q)
    assert pt.sampleCount() == 0
    got = pt.generateImages(2)
    dev = pbr.Device(gpu_device)
    dev.upload_scene(scene.desc)
    dev.configure(scene.config(32, 32))
    pbr.cfg_reset()
    moved = skin_dq_ref.positions(arrays["vertices"], bones, weights, Q)
    assert not np.array_equal(bits(moved), bits(arrays["vertices"]))
    dev.update_geometry(moved)
    cam = pbr.Camera()
    pbr.host.pbrh_pt_camera(pt._h, ctypes.byref(cam))
    dev.render(0, pbr.frame_seeds(0, 2), pbr.pixel_dimension(32, 32), cam)
    assert same_values(got, dev.read_output())
    dev.close()
    pt.close()
