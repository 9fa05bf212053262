"""pbr_set_skin / pbr_update_skin on the GPU: the device's V' and N' equal the numpy restatement (tests/skin_ref.py) bit for bit,
everything behind them equals pbr_update_geometry( V', N' ) — boxes, patches, renders, single rays, the ordered walks behind the
re-link, the temporal history —, a one-hot skin equals pbr_update_transforms, the rest pose makes the call non-cumulative, and
every refusal, the overflow found on the device included, leaves the context as it was.

The fixtures at their own size: the pillars' 40 vertices stay below one wave, Suzanne's 603 span three workgroups and are no
multiple of one.  Every fixture's influences (skin_ref.influences_for) hold one-hot elements, blends of two, three and four bones,
zero weights between others and weights that do not sum to 1; the bones are the fixture's parts and one more that nobody uses."""
import ctypes
import types

import numpy as np
import pytest

import patch_refit_ref
import refit_ref
import refit_scenes
import skin_ref
import transform_ref
from conftest import same_values, describe_mismatch
from test_gpu_patch_refit import assert_same_render, bits, rays_for, rendered, with_arrays
from test_gpu_transforms import ALPHA, FIXTURES, SHIFT, device, other, third, same_bits  # noqa: F401 (the three are fixtures)

pytestmark = pytest.mark.gpu

NO_SKIN = {"bones": 0, "device_bytes": 0, "updates": 0, "last_update": False, "ms": 0.0}
_cases = {}


def case(pbr, name, shift=SHIFT, skip=()):
    """The fixture, its influences, a dealing of the matrix set over the bones and the restatement's V', N'.  Computed once per
    case and shared; nobody writes to the arrays."""
    key = (name, shift, skip)
    if key not in _cases:
        sc = refit_scenes.load(pbr, name)
        a = sc.arrays
        c = types.SimpleNamespace(sc=sc, a=a)
        c.vb, c.vw, c.nb, c.nw, c.bones = skin_ref.influences_for(name, a["facesV"], a["facesN"], a["vertices"].shape[0], a["normals"].shape[0])
        c.M = transform_ref.matrices_for(c.bones, shift, skip)
        c.v, c.n = skin_ref.skin(a["vertices"], c.vb, c.vw, a["normals"], c.nb, c.nw, c.M)
        _cases[key] = c
    return _cases[key]


def expected_bytes(c, with_normals=True):
    """pbr_hip_diag.h: 64 V + 48 N + 48 bones + 4."""
    v, n = c.a["vertices"].shape[0], c.a["normals"].shape[0]
    return 64 * v + (48 * n if with_normals else 0) + 48 * c.bones + 4


def geometry_is(device, v, n, what):
    got_v, got_n = device.read_geometry()
    same_bits(got_v, v, what + ": V'")
    same_bits(got_n, n, what + ": N'")


# ---- 1: the skin, the boxes and the patches against the restatements --------------------------------------------------------

@pytest.mark.parametrize("alpha", (ALPHA, 0.0))
@pytest.mark.parametrize("name", FIXTURES)
def test_skin_boxes_and_patches_equal_the_numpy_restatements(pbr, device, name, alpha):
    c = case(pbr, name)
    a = c.a
    assert not np.array_equal(bits(c.v), bits(a["vertices"])) and not np.array_equal(bits(c.n), bits(a["normals"]))
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=alpha))
    assert device.skin_info() == NO_SKIN
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    assert device.skin_info() == {"bones": c.bones, "device_bytes": expected_bytes(c), "updates": 0, "last_update": False, "ms": 0.0}
    faces, normals = a["facesV"].shape[0], a["normals"].shape[0]
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 0, "last_update": False, "alpha": 0.0}
    device.update_skin(c.M)
    geometry_is(device, c.v, c.n, "update_skin")
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], c.v, c.n, alpha), "boxes")
    same_bits(device.read_patches(), patch_refit_ref.pack_patches(a["facesV"], a["facesN"], c.v, c.n), "patches")
    info = device.skin_info()
    assert info["ms"] > 0.0 and device.last_kernel_ms() >= info["ms"]
    assert dict(info, ms=0.0) == {"bones": c.bones, "device_bytes": expected_bytes(c), "updates": 1, "last_update": True, "ms": 0.0}
    assert device.transform_info() == {"parts": 0, "device_bytes": 0, "updates": 0, "last_update": False, "ms": 0.0}
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 1, "last_update": True,
                                         "alpha": float(np.float32(alpha))}
    assert device.refit_info()["updates"] == 1
    device.configure(c.sc.config(phong_tessellation=alpha))          # the state rule: a pbr_update_geometry under this alpha
    # any other update is no skin update
    device.update_geometry(c.v, c.n)
    assert dict(device.skin_info(), ms=0.0) == {"bones": c.bones, "device_bytes": expected_bytes(c), "updates": 1, "last_update": False, "ms": 0.0}
    # dropping the skin frees it
    device.set_skin(None)
    assert device.skin_info()["bones"] == 0 and device.skin_info()["device_bytes"] == 0
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_skin"):
        device.update_skin(c.M)


# ---- 2: three contexts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", (0, 2, 3))
@pytest.mark.parametrize("name", FIXTURES)
def test_skinned_context_equals_update_geometry_and_a_fresh_upload(pbr, device, other, third, name, traversal):
    """A: set_skin + update_skin( M ).  B: update_geometry( V', N' ).  C: a fresh upload of S' with the nodes A reads back.
    Images, debug images, counters and 4096 single rays are equal; under an ordered walk the re-linked records of A and B are
    the same bytes."""
    c = case(pbr, name, skip=("translation of 1e6",))
    cfg = c.sc.config(traversal=traversal, phong_tessellation=ALPHA)
    for dev in (device, other):
        dev.refit_ordered_walk(traversal != 0)
        dev.upload_scene(c.sc.desc)
        dev.configure(cfg)
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_skin(c.M)
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


# ---- 3: a one-hot skin is the rigid call ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_one_hot_skin_equals_set_parts_and_update_transforms(pbr, device, other, name):
    c = case(pbr, name)
    a = c.a
    vertex_part, normal_part, parts = transform_ref.parts_of(name, a["facesV"], a["facesN"], a["vertices"].shape[0], a["normals"].shape[0])
    M = transform_ref.matrices_for(parts, SHIFT)
    vb, vw = skin_ref.one_hot(vertex_part)
    nb, nw = skin_ref.one_hot(normal_part)
    # the 1.0 in slot 2 for every other element, behind zero weights that name other bones
    for b, w, part in ((vb, vw, vertex_part), (nb, nw, normal_part)):
        b[1::2, 2], w[1::2, 2] = part[1::2], 1.0
        b[1::2, 0], w[1::2, 0] = (part[1::2] + 1) % parts, 0.0
    for dev in (device, other):
        dev.upload_scene(c.sc.desc)
        dev.configure(c.sc.config(phong_tessellation=ALPHA))
    device.set_skin(vb, vw, nb, nw, parts)
    device.update_skin(M)
    other.set_parts(vertex_part, normal_part, parts)
    other.update_transforms(M)
    want_v, want_n = other.read_geometry()
    geometry_is(device, want_v, want_n, "one-hot skin against the parts")
    same_bits(want_v, transform_ref.transform(a["vertices"], vertex_part, a["normals"], normal_part, M)[0])
    same_bits(device.read_bvh(), other.read_bvh(), "boxes")
    same_bits(device.read_patches(), other.read_patches(), "patches")


# ---- 4: the rest pose -------------------------------------------------------------------------------------------------------

def test_skin_updates_start_from_the_rest_pose(pbr, device):
    """M1 then M2 leaves what M2 alone leaves; an update_vertices or an update_transforms in between changes nothing of what the
    next skin update produces; all-identity bones bring the rest pose back bit for bit (under dyadic weights: the header promises
    no more); set_skin after an update_geometry captures that pose; a skin and parts set together do not disturb each other."""
    c = case(pbr, "ref_suzanne_sa")
    a = c.a
    vertex_part, normal_part, parts = transform_ref.parts_of("ref_suzanne_sa", a["facesV"], a["facesN"], a["vertices"].shape[0], a["normals"].shape[0])
    Mp = transform_ref.matrices_for(parts, 3)
    parts_v, parts_n = transform_ref.transform(a["vertices"], vertex_part, a["normals"], normal_part, Mp)
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=0.0))
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_skin(transform_ref.matrices_for(c.bones, 1))
    device.update_skin(c.M)
    geometry_is(device, c.v, c.n, "M1 then M2")
    nodes = device.read_bvh()
    device.update_vertices(refit_ref.deform(a["facesV"], a["vertices"], "large", 7))
    device.update_skin(c.M)
    geometry_is(device, c.v, c.n, "after an update_vertices in between")
    same_bits(device.read_bvh(), nodes)
    # parts beside the skin: each call works from its own rest pose and leaves the other's state alone
    device.set_parts(vertex_part, normal_part, parts)                # captures the SKINNED pose as the parts' rest pose
    assert device.skin_info()["updates"] == 3 and device.skin_info()["bones"] == c.bones
    device.update_transforms(Mp)
    moved_v, moved_n = transform_ref.transform(c.v, vertex_part, c.n, normal_part, Mp)
    geometry_is(device, moved_v, moved_n, "parts over the skinned pose")
    assert device.transform_info()["last_update"] and not device.skin_info()["last_update"]
    device.update_skin(c.M)
    geometry_is(device, c.v, c.n, "after an update_transforms in between")
    assert device.skin_info()["last_update"] and not device.transform_info()["last_update"]
    assert device.transform_info()["updates"] == 1 and device.skin_info()["updates"] == 4
    device.update_transforms(Mp)
    geometry_is(device, moved_v, moved_n, "the parts' rest pose is still theirs")
    device.set_parts(None)
    assert device.skin_info()["bones"] == c.bones and device.transform_info()["parts"] == 0
    device.update_skin(c.M)
    geometry_is(device, c.v, c.n, "the skin outlives the parts")
    # a skin set while parts are there, and dropped again: the parts stay
    device.upload_scene(c.sc.desc)
    device.set_parts(vertex_part, normal_part, parts)
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.update_skin(c.M)
    device.set_skin(None)
    assert device.transform_info()["parts"] == parts and device.skin_info() == dict(NO_SKIN, last_update=True)
    device.update_transforms(Mp)
    geometry_is(device, parts_v, parts_n, "the parts outlive the skin")
    # all identities, dyadic weights
    dyadic_v, dyadic_n = c.vw.copy(), c.nw.copy()
    for w in (dyadic_v, dyadic_n):
        w[(w == np.float32(0.4)).any(axis=1)] = (0.5, 0.25, 0.125, 0.125)
        w[(w == np.float32(0.7)).any(axis=1)] = (0.75, 0.25, 0.0, 0.0)
    identities = np.tile(transform_ref.IDENTITY, (c.bones, 1))
    assert transform_ref.is_identity(skin_ref.blend(c.vb, dyadic_v, identities)).all() and not transform_ref.is_identity(skin_ref.blend(c.vb, c.vw, identities)).all()
    device.upload_scene(c.sc.desc)
    device.set_skin(c.vb, dyadic_v, c.nb, dyadic_n, c.bones)
    device.update_skin(c.M)
    geometry_is(device, *skin_ref.skin(a["vertices"], c.vb, dyadic_v, a["normals"], c.nb, dyadic_n, c.M), "dyadic weights")
    device.update_skin(identities)
    geometry_is(device, a["vertices"], a["normals"], "all identities")
    # a new rest pose — the one an update_geometry left
    device.update_geometry(c.v, c.n)
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    assert device.skin_info()["updates"] == 0
    M = transform_ref.matrices_for(c.bones, 4)
    device.update_skin(M)
    want_v, want_n = skin_ref.skin(c.v, c.vb, c.vw, c.n, c.nb, c.nw, M)
    geometry_is(device, want_v, want_n, "from the captured pose")
    assert not np.array_equal(bits(want_v), bits(skin_ref.positions(a["vertices"], c.vb, c.vw, M)))


# ---- 5: without normal influences, without usable normals -------------------------------------------------------------------

@pytest.mark.parametrize("name", ("ref_spheres_schlick", "ref_suzanne_sa"))
def test_without_normal_influences_the_context_s_normals_stay(pbr, device, other, name):
    c = case(pbr, name)
    a = c.a
    cfg = c.sc.config(phong_tessellation=ALPHA)
    kept = patch_refit_ref.perturb_normals(a["normals"], seed=2)
    for dev in (device, other):
        dev.upload_scene(c.sc.desc)
        dev.configure(cfg)
        dev.update_geometry(a["vertices"], kept)                      # the normals the context holds from now on
    device.set_skin(c.vb, c.vw)
    assert device.skin_info()["bones"] == int(c.vb.max()) + 1
    device.set_skin(c.vb, c.vw, None, None, c.bones)
    assert device.skin_info()["device_bytes"] == expected_bytes(c, with_normals=False)
    device.update_skin(c.M)
    other.update_geometry(c.v)
    geometry_is(device, c.v, kept, "positions alone")
    same_bits(device.read_patches(), patch_refit_ref.pack_patches(a["facesV"], a["facesN"], c.v, kept))
    same_bits(device.read_bvh(), other.read_bvh())
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], c.v, kept, ALPHA))


def test_scene_without_usable_normals_takes_vertex_influences_only(pbr, device):
    c = case(pbr, "ref_pillars_sa")
    bare = with_arrays(c.sc)
    bare.desc.facesN, bare.desc.normals, bare.desc.num_normals = None, None, 0
    device.upload_scene(bare.desc)
    with pytest.raises(pbr.PbrError, match="-1: .*6 normals, the uploaded scene has 0"):
        device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    # normals there, indices out of range: the count matches, the scene has no patches — PBR_ESTATE
    broken = with_arrays(c.sc)
    wild = c.a["facesN"].copy()
    wild[0, 0] = c.a["normals"].shape[0]
    broken.arrays["facesN"] = wild
    broken.desc.facesN = wild.ctypes.data
    device.upload_scene(broken.desc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_skin: .*without usable vertex normals"):
        device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    assert device.skin_info() == NO_SKIN
    device.set_skin(c.vb, c.vw, None, None, c.bones)
    device.update_skin(c.M)
    same_bits(device.read_geometry()[0], c.v)
    same_bits(device.read_bvh(), refit_ref.refit(c.a["bvh"], c.a["facesV"], c.v))


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_as_it_was(pbr, device):
    c = case(pbr, "ref_suzanne_sa")
    a, M = c.a, c.M
    count, ncount = a["vertices"].shape[0], a["normals"].shape[0]
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_skin before pbr_upload_scene"):
        device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_skin"):
        device.update_skin(M)
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_skin without a skin: pbr_set_skin"):
        device.update_skin(M)
    set_skin = pbr.hip.pbr_set_skin
    vb, vw, nb, nw = c.vb, c.vw, c.nb, c.nw

    def own_refusals():
        """pbr_set_skin's own, in the header's order."""
        assert set_skin(None, vb.ctypes.data, vw.ctypes.data, count, nb.ctypes.data, nw.ctypes.data, ncount, c.bones) == -1
        assert set_skin(device._ctx, None, vw.ctypes.data, count, nb.ctypes.data, nw.ctypes.data, ncount, c.bones) == -1
        assert set_skin(device._ctx, vb.ctypes.data, None, count, nb.ctypes.data, nw.ctypes.data, ncount, c.bones) == -1
        with pytest.raises(pbr.PbrError, match="-1: .*%d vertices, the uploaded scene has %d" % (count - 1, count)):
            device.set_skin(vb[:-1], vw[:-1], nb, nw, c.bones)
        with pytest.raises(pbr.PbrError, match="-1: .*%d normals, the uploaded scene has %d" % (ncount - 1, ncount)):
            device.set_skin(vb, vw, nb[:-1], nw[:-1], c.bones)
        assert set_skin(device._ctx, vb.ctypes.data, vw.ctypes.data, count, None, nw.ctypes.data, ncount, c.bones) == -1
        assert set_skin(device._ctx, vb.ctypes.data, vw.ctypes.data, count, nb.ctypes.data, None, ncount, c.bones) == -1
        assert set_skin(device._ctx, vb.ctypes.data, vw.ctypes.data, count, nb.ctypes.data, nw.ctypes.data, 0, c.bones) == -1
        assert set_skin(device._ctx, vb.ctypes.data, vw.ctypes.data, count, None, None, 0, 0) == -1
        with pytest.raises(pbr.PbrError, match="-1: .*slot 1 of vertex 0 names bone 6, there are 1 bones"):
            device.set_skin(vb, vw, nb, nw, 1)
        wild = nb.copy()
        slot = int(np.argmax(nw[7] == 0))                            # a slot of weight 0 is checked like the others
        wild[7, slot] = 77
        with pytest.raises(pbr.PbrError, match="-1: .*slot %d of normal 7 names bone 77, there are 7 bones" % slot):
            device.set_skin(vb, vw, wild, nw, c.bones)
        for value in (np.nan, np.inf, -0.5):
            w = vw.copy()
            w[9, 3] = value
            with pytest.raises(pbr.PbrError, match="-1: .*the weight in slot 3 of vertex 9 is "):
                device.set_skin(vb, w, nb, nw, c.bones)
        w = nw.copy()
        w[5] = 0.0
        with pytest.raises(pbr.PbrError, match="-1: .*the four weights of normal 5 are all 0"):
            device.set_skin(vb, vw, nb, w, c.bones)

    assert vw[0, 1] == 0 and vb[0, 1] == 6                           # vertex 0: pattern 0, its slot 1 names the unused bone under weight 0
    own_refusals()
    assert device.skin_info() == NO_SKIN

    device.set_skin(vb, vw, nb, nw, c.bones)
    device.update_skin(transform_ref.matrices_for(c.bones, 1))
    before = rendered(device, c.sc)
    geometry, nodes, patches = device.read_geometry(), device.read_bvh(), device.read_patches()

    def unchanged(what):
        geometry_is(device, geometry[0], geometry[1], what)
        same_bits(device.read_bvh(), nodes, what)
        same_bits(device.read_patches(), patches, what)
        assert_same_render(rendered(device, c.sc), before, what)
        assert device.skin_info()["updates"] == 1 and device.skin_info()["bones"] == c.bones and device.refit_info()["updates"] == 1, what

    # a refused pbr_set_skin keeps the skin that was set
    own_refusals()
    unchanged("a refused pbr_set_skin")
    update = pbr.hip.pbr_update_skin
    assert update(None, M.ctypes.data, c.bones) == -1
    assert update(device._ctx, None, c.bones) == -1
    unchanged("null matrices")
    with pytest.raises(pbr.PbrError, match="-1: .*6 matrices, pbr_set_skin declared 7 bones"):
        device.update_skin(M[:-1])
    unchanged("another bone count")
    for bad in (np.nan, np.inf):
        m = M.copy()
        m[3, 11] = bad
        with pytest.raises(pbr.PbrError, match="-1: .*word 11 of bone 3's matrix is not finite"):
            device.update_skin(m)
        unchanged("a matrix word that is not finite")
    # finite matrices, a product that is not: found on the device
    for rows in (np.diag([3e38, 1.0, 1.0]), [[3e38, 3e38, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]):
        m = M.copy()
        m[2] = transform_ref._matrix(rows, (0.0, 0.0, 0.0))
        assert skin_ref.refused(m) is None and skin_ref.not_finite(skin_ref.positions(a["vertices"], vb, vw, m)).any()
        with pytest.raises(pbr.PbrError, match="-1: .*a skinned position is not finite"):
            device.update_skin(m)
        unchanged("an overflow found on the device")
    # pbr_update_geometry's own: an ordered traversal without pbr_refit_ordered_walk
    device.configure(c.sc.config(traversal=2, phong_tessellation=ALPHA))
    before = rendered(device, c.sc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_skin while a ray-ordered traversal"):
        device.update_skin(M)
    unchanged("ordered traversal")
    # and the call still works afterwards; a singular bone is not refused (bone 6 is the one nobody uses, bone 5 blends in)
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    device.update_skin(M)
    geometry_is(device, c.v, c.n, "after the refusals")
    m = M.copy()
    m[5] = m[6] = 0.0
    device.update_skin(m)
    geometry_is(device, *skin_ref.skin(a["vertices"], vb, vw, a["normals"], nb, nw, m), "singular bones")
    # a new upload drops the skin
    device.upload_scene(c.sc.desc)
    assert device.skin_info() == NO_SKIN
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_skin"):
        device.update_skin(M)
    same_bits(device.read_geometry()[0], a["vertices"])


def test_not_nested_tree_takes_a_skin_but_no_update(pbr, device):
    from test_scene_pack_cpu import hand_tree, NOT_NESTED
    desc, keep = hand_tree(pbr, NOT_NESTED)
    vertices = keep[0].arrays()["vertices"]
    device.upload_scene(desc)
    device.set_skin(*skin_ref.one_hot(np.zeros(vertices.shape[0], np.uint32)))
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_skin: .*not properly nested"):
        device.update_skin(transform_ref.MATRICES[1])
    same_bits(device.read_geometry()[0], vertices)
    same_bits(device.read_bvh(), keep[1])


# ---- 7: the temporal history ------------------------------------------------------------------------------------------------

def test_temporal_history_follows_a_skin_update_as_it_follows_update_vertices(pbr, device, other):
    """track_motion on; adaptive render + temporal call; move the tall block of the Cornell box; render + temporal call: with
    update_skin( identity, translation ) under one-hot weights on one context and update_vertices( V' ) on the other,
    `integrated`, `history` and the motion planes are the same bits, and faces of the identity bone report code 1 (UNMOVED)."""
    from test_gpu_temporal import cornell, view, MOVE
    from test_gpu_temporal_motion import step, tall_block, BLOCK_MOVE
    steps = []
    for dev in (device, other):
        sc, cfg, px = cornell(pbr, dev)
        arrays = sc.arrays()
        material, mask = tall_block(arrays)
        bones, weights = skin_ref.one_hot(mask.astype(np.uint32))
        M = np.stack([transform_ref.IDENTITY, transform_ref._matrix(np.eye(3), BLOCK_MOVE)])
        V = skin_ref.positions(arrays["vertices"], bones, weights, M)
        assert np.array_equal(bits(V[~mask]), bits(arrays["vertices"][~mask])) and not np.array_equal(V[mask], arrays["vertices"][mask])
        dev.temporal_track_motion(True)
        first = step(pbr, dev, px, view(pbr, sc), 0)
        if dev is device:
            dev.set_skin(bones, weights)
            dev.update_skin(M)
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


# ---- 8: the tracer ----------------------------------------------------------------------------------------------------------

def test_path_tracer_forwards_the_calls(pbr, gpu_device):
    """PathTracer::setSkin / updateSkin: the tracer's frames of the skinned scene against a context driven by hand."""
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    scene = pbr.HostScene.generate("cornell", 1, 0)
    arrays = scene.arrays()
    count = arrays["vertices"].shape[0]
    bones = np.tile(np.array([0, 1, 1, 0], np.uint32), (count, 1))
    weights = np.where((np.arange(count) % 2 == 0)[:, None], np.array([0.5, 0.5, 0.0, 0.0], np.float32), np.array([0.0, 0.25, 0.0, 0.75], np.float32))
    M = np.stack([transform_ref.IDENTITY, transform_ref.MATRICES[4]])
    pt = pbr.PathTracer(gpu_device, 32, 32)
    pt.initOpenCLBuffers(scene)
    pt.setSkin(bones, weights)
    pt.updateSkin(M)
    assert pt.sampleCount() == 0
    got = pt.generateImages(2)
    dev = pbr.Device(gpu_device)
    dev.upload_scene(scene.desc)
    dev.configure(scene.config(32, 32))
    pbr.cfg_reset()
    moved = skin_ref.positions(arrays["vertices"], bones, weights, M)
    assert not np.array_equal(bits(moved), bits(arrays["vertices"]))
    dev.update_geometry(moved)
    cam = pbr.Camera()
    pbr.host.pbrh_pt_camera(pt._h, ctypes.byref(cam))
    dev.render(0, pbr.frame_seeds(0, 2), pbr.pixel_dimension(32, 32), cam)
    assert same_values(got, dev.read_output())
    dev.close()
    pt.close()
