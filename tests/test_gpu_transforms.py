"""pbr_set_parts / pbr_update_transforms / pbr_read_geometry on the GPU: the device's V' and N' equal the numpy restatement
(tests/transform_ref.py) bit for bit, everything behind them equals pbr_update_geometry( V', N' ) — boxes, patches, renders,
single rays, the ordered walks behind the re-link, the temporal history —, the rest pose makes the call non-cumulative, and every
refusal, the overflow found on the device included, leaves the context as it was.

The fixtures at their own size: the pillars' 40 vertices stay below one wave, Suzanne's 603 span three workgroups and are no
multiple of one; Suzanne is cut by vertex index % 5, so faces span parts and part 5 is empty."""
import ctypes
import types

import numpy as np
import pytest

import patch_refit_ref
import refit_ref
import refit_scenes
import transform_ref
from conftest import same_values, describe_mismatch
from test_gpu_patch_refit import assert_same_render, bits, rays_for, rendered, with_arrays

pytestmark = pytest.mark.gpu

ALPHA = 0.6
FIXTURES = ("ref_pillars_sa", "ref_spheres_schlick", "ref_suzanne_sa")
SHIFT = 2       # the dealing of the matrix set that gives part 0 the scale and reaches the translation of 1e6 with four parts


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


@pytest.fixture()
def other(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


@pytest.fixture()
def third(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


_cases = {}


def case(pbr, name, shift=SHIFT, skip=()):
    """The fixture, its parts, a dealing of the matrix set and the restatement's V', N'.  Computed once per case and shared;
    nobody writes to the arrays."""
    key = (name, shift, skip)
    if key not in _cases:
        sc = refit_scenes.load(pbr, name)
        a = sc.arrays
        c = types.SimpleNamespace(sc=sc, a=a)
        c.vertex_part, c.normal_part, c.parts = transform_ref.parts_of(name, a["facesV"], a["facesN"], a["vertices"].shape[0], a["normals"].shape[0])
        c.M = transform_ref.matrices_for(c.parts, shift, skip)
        c.v, c.n = transform_ref.transform(a["vertices"], c.vertex_part, a["normals"], c.normal_part, c.M)
        _cases[key] = c
    return _cases[key]


def same_bits(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), what + ": " + describe_mismatch(got, want)


def expected_bytes(c, with_normals=True):
    v, n = c.a["vertices"].shape[0], c.a["normals"].shape[0]
    return 36 * v + (20 * n if with_normals else 0) + 96 * c.parts + 4


# ---- 1: pbr_read_geometry ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_read_geometry_returns_what_the_context_holds(pbr, device, name):
    c = case(pbr, name)
    a = c.a
    device.upload_scene(c.sc.desc)
    v, n = device.read_geometry()
    same_bits(v, a["vertices"], "uploaded vertices")
    same_bits(n, a["normals"], "uploaded normals (the host copy)")
    device.update_geometry(c.v, c.n)
    v, n = device.read_geometry()
    same_bits(v, c.v, "after update_geometry")
    same_bits(n, c.n, "after update_geometry")
    moved = refit_ref.deform(a["facesV"], a["vertices"], "small", 5)
    device.upload_scene(c.sc.desc)
    device.update_vertices(moved)
    v, n = device.read_geometry()
    same_bits(v, moved, "after update_vertices")
    same_bits(n, a["normals"], "after update_vertices: the upload's normals")
    # count only, and too little room
    nv, nn = ctypes.c_uint32(), ctypes.c_uint32()
    read = pbr.hip.pbr_read_geometry
    assert read(device._ctx, None, 0, ctypes.byref(nv), None, 0, ctypes.byref(nn)) == 0
    assert (nv.value, nn.value) == (a["vertices"].shape[0], a["normals"].shape[0])
    room = np.zeros_like(a["vertices"])
    assert read(device._ctx, room.ctypes.data, nv.value - 1, ctypes.byref(nv), None, 0, ctypes.byref(nn)) == -1
    assert read(device._ctx, room.ctypes.data, nv.value, None, None, 0, ctypes.byref(nn)) == -1
    assert read(device._ctx, room.ctypes.data, nv.value, ctypes.byref(nv), None, 0, ctypes.byref(nn)) == 0
    same_bits(room, moved, "vertices alone")


def test_read_geometry_without_usable_normals_and_without_a_scene(pbr, device):
    c = case(pbr, "ref_pillars_sa")
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_read_geometry before pbr_upload_scene"):
        device.read_geometry()
    bare = with_arrays(c.sc)
    bare.desc.facesN, bare.desc.normals, bare.desc.num_normals = None, None, 0
    device.upload_scene(bare.desc)
    v, n = device.read_geometry()
    same_bits(v, c.a["vertices"])
    assert n.shape == (0, 4)


# ---- 2: the transform, the boxes and the patches against the restatements ---------------------------------------------------

@pytest.mark.parametrize("alpha", (ALPHA, 0.0))
@pytest.mark.parametrize("name", FIXTURES)
def test_transform_boxes_and_patches_equal_the_numpy_restatements(pbr, device, name, alpha):
    c = case(pbr, name)
    a = c.a
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=alpha))
    assert device.transform_info() == {"parts": 0, "device_bytes": 0, "updates": 0, "last_update": False, "ms": 0.0}
    device.set_parts(c.vertex_part, c.normal_part, c.parts)
    assert device.transform_info() == {"parts": c.parts, "device_bytes": expected_bytes(c), "updates": 0, "last_update": False, "ms": 0.0}
    faces, normals = a["facesV"].shape[0], a["normals"].shape[0]
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 0, "last_update": False, "alpha": 0.0}
    device.update_transforms(c.M)
    v, n = device.read_geometry()
    same_bits(v, c.v, "V'")
    same_bits(n, c.n, "N'")
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], c.v, c.n, alpha), "boxes")
    same_bits(device.read_patches(), patch_refit_ref.pack_patches(a["facesV"], a["facesN"], c.v, c.n), "patches")
    info = device.transform_info()
    assert info["ms"] > 0.0 and device.last_kernel_ms() >= info["ms"]
    assert dict(info, ms=0.0) == {"parts": c.parts, "device_bytes": expected_bytes(c), "updates": 1, "last_update": True, "ms": 0.0}
    assert device.patch_refit_info() == {"patches": True, "device_bytes": 40 * faces + 16 * normals, "updates": 1, "last_update": True,
                                         "alpha": float(np.float32(alpha))}
    assert device.refit_info()["updates"] == 1
    device.configure(c.sc.config(phong_tessellation=alpha))          # the state rule: a pbr_update_geometry under this alpha
    # any other update is no transform
    device.update_geometry(c.v, c.n)
    assert dict(device.transform_info(), ms=0.0) == {"parts": c.parts, "device_bytes": expected_bytes(c), "updates": 1, "last_update": False, "ms": 0.0}
    # dropping the parts frees them
    device.set_parts(None)
    assert device.transform_info()["parts"] == 0 and device.transform_info()["device_bytes"] == 0
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_parts"):
        device.update_transforms(c.M)


# ---- 3: three contexts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", (0, 2, 3))
@pytest.mark.parametrize("name", FIXTURES)
def test_transformed_context_equals_update_geometry_and_a_fresh_upload(pbr, device, other, third, name, traversal):
    """A: set_parts + update_transforms( M ).  B: update_geometry( V', N' ).  C: a fresh upload of S' with the nodes A reads
    back.  Images, debug images, counters and 4096 single rays are equal; under an ordered walk the re-linked records of A and
    B are the same bytes."""
    c = case(pbr, name, skip=("translation of 1e6",))
    cfg = c.sc.config(traversal=traversal, phong_tessellation=ALPHA)
    for dev in (device, other):
        dev.refit_ordered_walk(traversal != 0)
        dev.upload_scene(c.sc.desc)
        dev.configure(cfg)
    device.set_parts(c.vertex_part, c.normal_part, c.parts)
    device.update_transforms(c.M)
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


# ---- 4 + 5: the rest pose ---------------------------------------------------------------------------------------------------

def test_transforms_start_from_the_rest_pose(pbr, device):
    """M1 then M2 leaves what M2 alone leaves; all identities bring the rest pose back bit for bit; an update_vertices in between
    changes nothing of what the next transform produces; set_parts after an update_geometry captures that pose."""
    c = case(pbr, "ref_suzanne_sa")
    a = c.a
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=0.0))
    device.set_parts(c.vertex_part, c.normal_part, c.parts)
    device.update_transforms(transform_ref.matrices_for(c.parts, 1))
    device.update_transforms(c.M)
    v, n = device.read_geometry()
    same_bits(v, c.v, "M1 then M2")
    same_bits(n, c.n, "M1 then M2")
    nodes = device.read_bvh()
    device.update_vertices(refit_ref.deform(a["facesV"], a["vertices"], "large", 7))
    device.update_transforms(c.M)
    v, n = device.read_geometry()
    same_bits(v, c.v, "after an update_vertices in between")
    same_bits(n, c.n, "after an update_vertices in between")
    same_bits(device.read_bvh(), nodes)
    device.update_transforms(np.tile(transform_ref.IDENTITY, (c.parts, 1)))
    v, n = device.read_geometry()
    same_bits(v, a["vertices"], "all identities")
    same_bits(n, a["normals"], "all identities")
    assert device.transform_info()["updates"] == 4
    # 5: a new rest pose — the one an update_geometry left
    device.update_geometry(c.v, c.n)
    device.set_parts(c.vertex_part, c.normal_part, c.parts)
    assert device.transform_info()["updates"] == 0
    M = transform_ref.matrices_for(c.parts, 4)
    device.update_transforms(M)
    want_v, want_n = transform_ref.transform(c.v, c.vertex_part, c.n, c.normal_part, M)
    v, n = device.read_geometry()
    same_bits(v, want_v, "from the captured pose")
    same_bits(n, want_n, "from the captured pose")
    assert not np.array_equal(bits(want_v), bits(transform_ref.positions(a["vertices"], c.vertex_part, M)))


# ---- 6: without normal parts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("ref_spheres_schlick", "ref_suzanne_sa"))
def test_without_normal_parts_the_context_s_normals_stay(pbr, device, other, name):
    c = case(pbr, name)
    a = c.a
    cfg = c.sc.config(phong_tessellation=ALPHA)
    kept = patch_refit_ref.perturb_normals(a["normals"], seed=2)
    for dev in (device, other):
        dev.upload_scene(c.sc.desc)
        dev.configure(cfg)
        dev.update_geometry(a["vertices"], kept)                      # the normals the context holds from now on
    device.set_parts(c.vertex_part)
    assert device.transform_info()["parts"] == int(c.vertex_part.max()) + 1
    device.set_parts(c.vertex_part, None, c.parts)
    assert device.transform_info()["device_bytes"] == expected_bytes(c, with_normals=False)
    device.update_transforms(c.M)
    other.update_geometry(c.v)
    v, n = device.read_geometry()
    same_bits(v, c.v)
    same_bits(n, kept)
    same_bits(device.read_patches(), patch_refit_ref.pack_patches(a["facesV"], a["facesN"], c.v, kept))
    same_bits(device.read_bvh(), other.read_bvh())
    same_bits(device.read_bvh(), patch_refit_ref.refit(a["bvh"], a["facesV"], a["facesN"], c.v, kept, ALPHA))


def test_scene_without_usable_normals_takes_vertex_parts_only(pbr, device):
    c = case(pbr, "ref_pillars_sa")
    bare = with_arrays(c.sc)
    bare.desc.facesN, bare.desc.normals, bare.desc.num_normals = None, None, 0
    device.upload_scene(bare.desc)
    with pytest.raises(pbr.PbrError, match="-1: .*6 normals, the uploaded scene has 0"):
        device.set_parts(c.vertex_part, c.normal_part, c.parts)
    # normals there, indices out of range: the count matches, the scene has no patches — PBR_ESTATE
    broken = with_arrays(c.sc)
    wild = c.a["facesN"].copy()
    wild[0, 0] = c.a["normals"].shape[0]
    broken.arrays["facesN"] = wild
    broken.desc.facesN = wild.ctypes.data
    device.upload_scene(broken.desc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_parts: .*without usable vertex normals"):
        device.set_parts(c.vertex_part, c.normal_part, c.parts)
    assert device.transform_info()["parts"] == 0
    device.set_parts(c.vertex_part, None, c.parts)
    device.update_transforms(c.M)
    same_bits(device.read_geometry()[0], c.v)
    same_bits(device.read_bvh(), refit_ref.refit(c.a["bvh"], c.a["facesV"], c.v))


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_as_it_was(pbr, device):
    c = case(pbr, "ref_suzanne_sa")
    a, M = c.a, c.M
    count = a["vertices"].shape[0]
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_parts before pbr_upload_scene"):
        device.set_parts(c.vertex_part, c.normal_part, c.parts)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_parts"):
        device.update_transforms(M)
    device.upload_scene(c.sc.desc)
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_transforms without parts: pbr_set_parts"):
        device.update_transforms(M)
    # pbr_set_parts' own
    set_parts = pbr.hip.pbr_set_parts
    vp, npart = c.vertex_part, c.normal_part
    assert set_parts(device._ctx, None, count, npart.ctypes.data, npart.shape[0], c.parts) == -1
    assert set_parts(device._ctx, vp.ctypes.data, count, None, npart.shape[0], c.parts) == -1
    assert set_parts(device._ctx, vp.ctypes.data, count, npart.ctypes.data, 0, c.parts) == -1
    assert set_parts(device._ctx, vp.ctypes.data, count, None, 0, 0) == -1
    with pytest.raises(pbr.PbrError, match="-1: .*%d vertices, the uploaded scene has %d" % (count - 1, count)):
        device.set_parts(vp[:-1], npart, c.parts)
    with pytest.raises(pbr.PbrError, match="-1: .*%d normals" % (npart.shape[0] - 1)):
        device.set_parts(vp, npart[:-1], c.parts)
    with pytest.raises(pbr.PbrError, match="-1: .*vertex 4 is in part 4, there are 4 parts"):
        device.set_parts(vp, npart, 4)
    wild = npart.copy()
    wild[7] = 77
    with pytest.raises(pbr.PbrError, match="-1: .*normal 7 is in part 77, there are 6 parts"):
        device.set_parts(vp, wild, c.parts)
    assert device.transform_info()["parts"] == 0

    device.set_parts(vp, npart, c.parts)
    device.update_transforms(transform_ref.matrices_for(c.parts, 1))
    before = rendered(device, c.sc)
    geometry, nodes, patches = device.read_geometry(), device.read_bvh(), device.read_patches()

    def unchanged(what):
        v, n = device.read_geometry()
        same_bits(v, geometry[0], what)
        same_bits(n, geometry[1], what)
        same_bits(device.read_bvh(), nodes, what)
        same_bits(device.read_patches(), patches, what)
        assert_same_render(rendered(device, c.sc), before, what)
        assert device.transform_info()["updates"] == 1 and device.refit_info()["updates"] == 1, what

    # a refused pbr_set_parts keeps the parts that were set
    with pytest.raises(pbr.PbrError, match="-1: .*vertex 4 is in part 4"):
        device.set_parts(vp, npart, 4)
    unchanged("a refused pbr_set_parts")
    update = pbr.hip.pbr_update_transforms
    assert update(None, M.ctypes.data, c.parts) == -1
    assert update(device._ctx, None, c.parts) == -1
    unchanged("null matrices")
    with pytest.raises(pbr.PbrError, match="-1: .*5 matrices, pbr_set_parts declared 6 parts"):
        device.update_transforms(M[:-1])
    unchanged("another part count")
    for bad in (np.nan, np.inf):
        m = M.copy()
        m[3, 11] = bad
        with pytest.raises(pbr.PbrError, match="-1: .*word 11 of part 3's matrix is not finite"):
            device.update_transforms(m)
        unchanged("a matrix word that is not finite")
    m = M.copy()
    m[5] = 0.0                                                       # the part nobody is in is checked like the others
    with pytest.raises(pbr.PbrError, match="-1: .*part 5's matrix has determinant 0"):
        device.update_transforms(m)
    unchanged("a singular matrix")
    m[5] = transform_ref._matrix(np.diag([1e30, 1e30, 1.0]), (0.0, 0.0, 0.0))
    with pytest.raises(pbr.PbrError, match="-1: .*part 5's matrix"):
        device.update_transforms(m)
    unchanged("cofactors that are not finite")
    # finite matrices, a product that is not: found on the device
    for rows in (np.diag([3e38, 1.0, 1.0]), [[3e38, 3e38, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]):
        m = M.copy()
        m[2] = transform_ref._matrix(rows, (0.0, 0.0, 0.0))
        assert transform_ref.refused(m) is None and transform_ref.not_finite(transform_ref.positions(a["vertices"], vp, m)).any()
        with pytest.raises(pbr.PbrError, match="-1: .*a transformed position is not finite"):
            device.update_transforms(m)
        unchanged("an overflow found on the device")
    # pbr_update_geometry's own: an ordered traversal without pbr_refit_ordered_walk
    device.configure(c.sc.config(traversal=2, phong_tessellation=ALPHA))
    before = rendered(device, c.sc)
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_transforms while a ray-ordered traversal"):
        device.update_transforms(M)
    unchanged("ordered traversal")
    # and the call still works afterwards
    device.configure(c.sc.config(phong_tessellation=ALPHA))
    device.update_transforms(M)
    same_bits(device.read_geometry()[0], c.v)
    # a new upload drops the parts
    device.upload_scene(c.sc.desc)
    assert device.transform_info() == {"parts": 0, "device_bytes": 0, "updates": 0, "last_update": False, "ms": 0.0}
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_set_parts"):
        device.update_transforms(M)
    same_bits(device.read_geometry()[0], a["vertices"])


def test_not_nested_tree_takes_parts_but_no_transform(pbr, device):
    from test_scene_pack_cpu import hand_tree, NOT_NESTED
    desc, keep = hand_tree(pbr, NOT_NESTED)
    vertices = keep[0].arrays()["vertices"]
    device.upload_scene(desc)
    same_bits(device.read_geometry()[0], vertices)
    device.set_parts(np.zeros(vertices.shape[0], np.uint32))
    with pytest.raises(pbr.PbrError, match="-3: .*pbr_update_transforms: .*not properly nested"):
        device.update_transforms(transform_ref.MATRICES[1])
    same_bits(device.read_geometry()[0], vertices)
    same_bits(device.read_bvh(), keep[1])


# ---- 8: the temporal history ------------------------------------------------------------------------------------------------

def test_temporal_history_follows_a_transform_as_it_follows_update_vertices(pbr, device, other):
    """track_motion on; adaptive render + temporal call; move the tall block of the Cornell box; render + temporal call: with
    update_transforms( identity, translation ) on one context and update_vertices( V' ) on the other, `integrated`, `history`
    and the motion planes are the same bits, and faces of the identity part report code 1 (UNMOVED)."""
    from test_gpu_temporal import cornell, view, MOVE
    from test_gpu_temporal_motion import step, tall_block, BLOCK_MOVE
    steps = []
    for dev in (device, other):
        sc, cfg, px = cornell(pbr, dev)
        arrays = sc.arrays()
        material, mask = tall_block(arrays)
        part = mask.astype(np.uint32)
        M = np.stack([transform_ref.IDENTITY, transform_ref._matrix(np.eye(3), BLOCK_MOVE)])
        V = transform_ref.positions(arrays["vertices"], part, M)
        assert np.array_equal(bits(V[~mask]), bits(arrays["vertices"][~mask])) and not np.array_equal(V[mask], arrays["vertices"][mask])
        dev.temporal_track_motion(True)
        first = step(pbr, dev, px, view(pbr, sc), 0)
        if dev is device:
            dev.set_parts(part)
            dev.update_transforms(M)
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


def test_path_tracer_forwards_the_calls(pbr, gpu_device):
    """PathTracer::setParts / updateTransforms: the tracer's frames of the moved scene against a context driven by hand."""
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    scene = pbr.HostScene.generate("cornell", 1, 0)
    arrays = scene.arrays()
    part = (np.arange(arrays["vertices"].shape[0]) % 2).astype(np.uint32)
    M = np.stack([transform_ref.IDENTITY, transform_ref.MATRICES[4]])
    pt = pbr.PathTracer(gpu_device, 32, 32)
    pt.initOpenCLBuffers(scene)
    pt.setParts(part)
    pt.updateTransforms(M)
    assert pt.sampleCount() == 0
    got = pt.generateImages(2)
    dev = pbr.Device(gpu_device)
    dev.upload_scene(scene.desc)
    dev.configure(scene.config(32, 32))
    pbr.cfg_reset()
    dev.update_geometry(transform_ref.positions(arrays["vertices"], part, M))
    cam = pbr.Camera()
    pbr.host.pbrh_pt_camera(pt._h, ctypes.byref(cam))
    dev.render(0, pbr.frame_seeds(0, 2), pbr.pixel_dimension(32, 32), cam)
    assert same_values(got, dev.read_output())
    dev.close()
    pt.close()
