"""The device refit against the REFERENCE'S OWN COMPILED CODE, from the recorded dumps alone (tests/golden/refhost_*.npz,
tests/refhost_fixture.py): after pbr_update_geometry / pbr_update_vertices with the unchanged geometry, every node's box is the
box the reference's BVH builder and MathHelp::triCalcAABB gave that node, and the patch records are those of the reference's
ObjParser arrays.  Every scene is uploaded with LOOSE boxes — each node's is the whole scene's — so a box that equals the
reference's afterwards is one the device computed.  refitPatches< true > and refitSubtrees< true > are held to triCalcAABB's
output directly by 257 hand-made faces, one per leaf: one past a workgroup, with the faces where the definition has corners."""
import numpy as np
import pytest

import hand_scenes
import patch_refit_ref
import refhost_fixture as rf
import refit_scenes
from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

PHONG = ("refhost_suzanne_a1.0", "refhost_spheres_a0.6", "refhost_pillars_a0.6")
FLAT = ("refhost_suzanne", "refhost_pillars")


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def padded(a):
    out = np.zeros((a.shape[0], 4), np.float32)
    out[:, :3] = a
    return out


def scene_of(pbr, arrays):
    """A refit_scenes.Scene over `arrays` with hand_scenes' config and camera; the boxes uploaded are loose."""
    base = hand_scenes.make(pbr, "leaf1")
    a = {k: np.ascontiguousarray(arrays[k]) for k in refit_scenes.ARRAYS}
    a["bvh"] = hand_scenes.loose_boxes(a["bvh"], a["vertices"])
    return refit_scenes.Scene(pbr, a, base.cfg, base.cam, base.px, base.seeds)


def shipped(pbr, name):
    d = rf.load(name)
    sc = scene_of(pbr, d)
    assert not same_values(sc.arrays["bvh"], d["bvh"])                                     # loose: nothing to copy from
    return d, sc, rf.flatten(d)


def assert_reference_boxes(got, d, want):
    """Node for node: the boxes of the nodes the flattening keeps, and the .w words it writes."""
    boxes = d["ref_tree_boxes"][want.kept]
    assert got.shape == want.bvh.shape
    assert same_values(got[:, 0:3], boxes[:, 0:3]), "bbMin: " + describe_mismatch(got[:, 0:3], boxes[:, 0:3])
    assert same_values(got[:, 4:7], boxes[:, 3:6]), "bbMax: " + describe_mismatch(got[:, 4:7], boxes[:, 3:6])
    assert np.array_equal(bits(got[:, [3, 7]]), bits(want.bvh[:, [3, 7]]))


@pytest.mark.parametrize("name", PHONG)
def test_update_geometry_gives_the_references_thick_boxes(pbr, device, name):
    d, sc, want = shipped(pbr, name)
    alpha = rf.alpha_of(d)
    assert alpha > 0.0 and d["facesV"].shape[0] <= 1082
    device.upload_scene(sc.desc)
    device.configure(sc.config(phong_tessellation=alpha))
    device.update_geometry(d["vertices"], d["normals"])
    assert_reference_boxes(device.read_bvh(), d, want)
    patches = patch_refit_ref.pack_patches(want.facesV, want.facesN, padded(d["ref_vertices"]), padded(d["ref_normals"]))
    assert np.array_equal(bits(device.read_patches()), bits(patches))
    assert device.patch_refit_info()["alpha"] == np.float32(alpha)


@pytest.mark.parametrize("name", FLAT)
def test_update_vertices_gives_the_references_boxes(pbr, device, name):
    d, sc, want = shipped(pbr, name)
    assert rf.alpha_of(d) == 0.0
    device.upload_scene(sc.desc)
    device.configure(sc.config(phong_tessellation=0.0))
    device.update_vertices(d["vertices"])
    assert_reference_boxes(device.read_bvh(), d, want)


def one_face_per_leaf(count):
    """A balanced binary tree over `count` leaves of one face each, in hand_scenes' tree notation."""
    nested = lambda n: 1 if n == 1 else [nested(n - n // 2), nested(n // 2)]
    return hand_scenes._linked(hand_scenes._sized(nested(count)))


def face_case_scene(pbr):
    f = rf.load("refhost_face_cases")
    count = f["corners"].shape[0]
    bvh, faces = hand_scenes.nodes_of(one_face_per_leaf(count))
    assert faces == count == 257 and bvh.shape[0] == 2 * count - 1
    vertices, normals = np.zeros((3 * count, 4), np.float32), np.zeros((3 * count, 4), np.float32)
    vertices[:, :3], normals[:, :3] = f["corners"].reshape(-1, 3), f["normals"].reshape(-1, 3)
    facesV = np.zeros((count, 4), np.uint32)
    facesV[:, :3] = np.arange(3 * count).reshape(count, 3)
    arrays = {"bvh": bvh, "facesV": facesV, "facesN": facesV.copy(), "vertices": vertices, "normals": normals,
              "materials": np.array(hand_scenes.MATERIALS[1], np.float32), "lights": np.zeros((0, 12), np.float32)}
    return f, scene_of(pbr, arrays)


@pytest.mark.parametrize("k", (0, 1, 2))
def test_hand_made_faces_get_tricalcaabbs_boxes(pbr, device, k):
    """Every leaf's box is triCalcAABB's for its face, across the workgroup edge (257 faces); every container's the exact
    bound of the reference's boxes below it; no box word is NaN."""
    f, sc = face_case_scene(pbr)
    alpha, want = float(f["alphas"][k]), f["boxes"][k]
    device.upload_scene(sc.desc)
    device.configure(sc.config(phong_tessellation=alpha))
    device.update_geometry(sc.arrays["vertices"], sc.arrays["normals"])
    got = device.read_bvh()
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got[:, [3, 7]]), bits(sc.arrays["bvh"][:, [3, 7]]))
    leaf, end, _ = rf.unflatten(got)
    face = got[leaf, 3].astype(np.int64)
    assert np.array_equal(face, np.arange(257)) and (got[leaf, 7] == -1).all()
    bad = ~((got[leaf, 0:3] == want[face, 0:3]).all(axis=1) & (got[leaf, 4:7] == want[face, 3:6]).all(axis=1))
    assert not bad.any(), (alpha, f["labels"][face[bad]].tolist(), got[leaf][bad], want[face[bad]])
    first = np.cumsum(leaf) - leaf                                                        # leaves before node i = its first face
    for i in np.nonzero(~leaf)[0]:
        below = want[first[i]:first[i] + int(leaf[i:end[i]].sum())]
        assert same_values(got[i, 0:3], below[:, 0:3].min(0)) and same_values(got[i, 4:7], below[:, 3:6].max(0)), i
