"""Regenerates tests/golden/refhost_*.npz (container only: needs the reference's tree and oracle/_ref/refhost_dump).

    python tests/golden/make_refhost.py

What is stored is DATA the reference's own compiled host code produced (oracle/refhost.py: its loaders, its BVH builder and
MathHelp::triCalcAABB, built unmodified), next to what this repository's loader and builder make of the same files:

  refhost_<model>[_a<alpha>][_noskip].npz
      ref_*   the dump of `refhost_dump scene` (oracle/refhost/dump.cpp has the record list): ObjParser's arrays and objects,
              every material_t and light_t field, the BVH from getRoot() depth first (left child first) with every leaf's Tri
              records, and the three sizes
      bvh, facesV, facesN, vertices, normals, materials (Shirley-Ashikhmin layout), materials_schlick, lights, sky_light
              the wire arrays (and pbr_config.sky_light) host/model_io.cpp + host/bvh_builder.cpp produce for the same file and settings, taken as
              make_reference_scenes.inputs_of takes them — the GPU tests upload these and need neither reference nor dumper
      settings_keys / settings_values   the Cfg overrides of the case
      A fixture that would not stay below SIZE_CAP in one file (the two 8 k-face models) lies in three, every array still in
      full: <name>.npz (what the parsers read, sizes, settings), <name>_tree.npz (the tree and its Tris), <name>_wire.npz.
  refhost_face_cases.npz
      corners, normals (N, 3, 3), labels, alphas and boxes (alphas, N, 6): hand-made faces and triCalcAABB's boxes for them

Every model is loaded with render.shadow_rays = 1, the only way the reference's ObjParser reads a .lights file at all
(a model without one switches the key back off by itself).
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

REFERENCE_MODELS = "/root/reference/resources/models/testing/"
MODELS = ("pillars", "suzanne", "spheres", "applejack2", "applejack3", "squirrel-mirror", "squirrels")

# fixture name: (obj file, Cfg overrides beyond config.json's defaults)
CASES = {"refhost_" + m: (m + ".obj", {}) for m in MODELS}
CASES.update({
    "refhost_suzanne_a1.0": ("suzanne.obj", {"render.phong_tessellation": 1.0}),
    "refhost_spheres_a0.6": ("spheres.obj", {"render.phong_tessellation": 0.6}),
    "refhost_pillars_a0.6": ("pillars.obj", {"render.phong_tessellation": 0.6}),
    "refhost_suzanne_noskip": ("suzanne.obj", {"bvh.skip_ahead": False}),
})
WIRE = ("bvh", "facesV", "facesN", "vertices", "normals", "materials", "lights")
SIZE_CAP = 407087         # bytes: the largest fixture committed before these (ref_applejack2_sa.npz); every file stays below
TREE = ("ref_tree_nodes", "ref_tree_boxes", "ref_tri_face", "ref_tri_normals", "ref_tri_boxes")
FACE_ALPHAS = (0.0, 0.5, 1.0)
FACE_COUNT = 257          # one past a workgroup of 256


def alpha_of(name):
    return float(CASES[name][1].get("render.phong_tessellation", 0.0))


def reference_dump(name, scratch):
    """{"ref_" + record: array} of one case, from the compiled reference."""
    from oracle import refhost
    obj, overrides = CASES[name]
    dump = refhost.dump_scene(REFERENCE_MODELS, obj, scratch, **dict(overrides, **{"render.shadow_rays": 1}))
    return {"ref_" + k: (np.array(v, dtype=str) if isinstance(v, list) else v) for k, v in dump.items()}


def wire_arrays(pbr, name):
    """The seven wire arrays of this repository's loader + builder for one case, and the Schlick layout of the materials."""
    obj, overrides = CASES[name]
    out = {}
    for brdf in (1, 0):
        pbr.cfg_reset()
        pbr.cfg_set(**dict(overrides, **{"render.shadow_rays": 1, "render.brdf": brdf}))
        sc = pbr.HostScene.load_obj(REFERENCE_MODELS, obj)
        arr = sc.arrays()
        arr["lights"] = arr["lights"][: sc.desc.num_lights]
        if brdf == 1:
            out.update({k: arr[k] for k in WIRE})
            out["sky_light"] = np.array(list(sc.config(8, 8).sky_light), np.float32)      # pbr_config's, from the .mtl
        else:
            assert all(np.array_equal(out[k].view(np.uint32), arr[k].view(np.uint32)) for k in WIRE if k != "materials")
            out["materials_schlick"] = arr["materials"]
    pbr.cfg_reset()
    return out


def settings_of(name):
    overrides = CASES[name][1]
    keys = sorted(overrides)
    return {"settings_keys": np.array(keys, dtype=str), "settings_values": np.array([float(overrides[k]) for k in keys], np.float64)}


def save(name, data):
    """One file, or three where one would reach SIZE_CAP; returns the paths written."""
    for suffix in ("", "_tree", "_wire"):
        if os.path.exists(os.path.join(HERE, name + suffix + ".npz")):
            os.remove(os.path.join(HERE, name + suffix + ".npz"))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    if os.path.getsize(path) < SIZE_CAP:
        return [path]
    wire = WIRE + ("materials_schlick", "sky_light")
    parts = {"": {k: v for k, v in data.items() if k not in TREE + wire}, "_tree": {k: data[k] for k in TREE}, "_wire": {k: data[k] for k in wire}}
    paths = [os.path.join(HERE, name + suffix + ".npz") for suffix in parts]
    for out, part in zip(paths, parts.values()):
        np.savez_compressed(out, **part)
        assert os.path.getsize(out) < SIZE_CAP, out
    return paths


# ---- hand-made faces ---------------------------------------------------------------------------------------------------

def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def face_cases():
    """(corners, normals, labels): (N, 3, 3) float32 twice and N names; N = FACE_COUNT, filled up with copies of the ordinary
    face.  The 1e-6 of the cases is triCalcAABB's test on t = ( n1 - n2 ) + ( n2 - n3 ): every |t.k| <= 0.000001f means
    'equal normals'."""
    tri = np.array([[0.25, 0.0, 0.5], [1.5, 0.25, 0.0], [0.5, 1.25, 0.75]])
    up = _unit(np.cross(tri[1] - tri[0], tri[2] - tri[0]))
    lean = [_unit(up + 0.3 * np.array(d)) for d in ([1, 0, 0.5], [-0.5, 1, 0], [0, -1, -0.5])]
    eps = np.float32(1e-6)
    z = [0.0, 0.0, 1.0]
    cases = [
        ("ordinary", tri, lean),
        ("equal normals", tri, [up, up, up]),
        # n1 and n3 differ by less than / exactly / more than the test's 1e-6 in x (t = n1 - n3 up to rounding)
        ("normals differ by 5e-7", tri, [[5e-7, 0, 1], z, z]),
        ("normals differ by 2e-6", tri, [[2e-6, 0, 1], z, z]),
        ("normals differ by 1e-3 in z only", tri, [[0, 0, 1.001], z, z]),
        # differences that cancel in t: n1 = n3, n2 far away — the patch is curved, the reference's test cannot see it
        ("n1 = n3, n2 leaning", tri, [lean[0], lean[1], lean[0]]),
        ("n1 = n3, n2 opposite", tri, [up, -up, up]),
        ("two equal corners", [tri[0], tri[0], tri[2]], lean),
        ("three equal corners", [tri[0], tri[0], tri[0]], lean),
        ("collinear corners", [tri[0], tri[0] + [0.25, 0.125, -0.125], tri[0] + [0.5, 0.25, -0.25]], lean),
        ("opposite normals", tri, [up, -up, lean[2]]),
        ("all normals opposite to the face", tri, [-lean[0], -lean[1], -lean[2]]),
        ("one zero normal", tri, [[0, 0, 0], lean[1], lean[2]]),
        ("all zero normals", tri, [[0, 0, 0]] * 3),
        ("corners at 1e6", tri * 1e6, lean),
        ("corners near 1e6", tri + 1e6, lean),
        ("corners at 1e-6", tri * 1e-6, lean),
        ("in the plane z = 0", [[0.25, 0.0, 0.0], [1.5, 0.25, 0.0], [0.5, 1.25, 0.0]], [_unit([0.3, 0.1, 1]), _unit([-0.2, 0.3, 1]), _unit([0, -0.3, 1])]),
        ("in the plane x = -0", [[-0.0, 0.25, 0.0], [-0.0, 1.5, 0.25], [-0.0, 0.5, 1.25]], [_unit([1, 0.3, 0.1]), _unit([1, -0.2, 0.3]), _unit([1, 0, -0.3])]),
        ("unnormalised normals", tri, [3.0 * lean[0], 0.25 * lean[1], lean[2]]),
    ]
    assert np.float32(5e-7) <= eps < np.float32(2e-6)
    labels = [c[0] for c in cases] + ["ordinary"] * (FACE_COUNT - len(cases))
    corners = np.array([c[1] for c in cases] + [tri] * (FACE_COUNT - len(cases)), np.float64).astype(np.float32)
    normals = np.array([c[2] for c in cases] + [lean] * (FACE_COUNT - len(cases)), np.float64).astype(np.float32)
    assert corners.shape == normals.shape == (FACE_COUNT, 3, 3)
    return corners, normals, labels


def face_fixture(scratch):
    from oracle import refhost
    corners, normals, labels = face_cases()
    boxes = np.stack([refhost.dump_faces(corners, normals, a, scratch) for a in FACE_ALPHAS])
    return {"corners": corners, "normals": normals, "labels": np.array(labels, dtype=str), "alphas": np.array(FACE_ALPHAS, np.float32), "boxes": boxes}


if __name__ == "__main__":
    import pbr_loader
    from oracle import refhost

    if refhost.build() is None:
        sys.exit("the reference's sources are not on this machine")
    pbr = pbr_loader.load()
    with tempfile.TemporaryDirectory() as scratch:
        for name in CASES:
            data = reference_dump(name, scratch)
            data.update(wire_arrays(pbr, name))
            data.update(settings_of(name))
            paths = save(name, data)
            print("%-26s tree %5d nodes %5d leaves depth %2d, wire %5d nodes %5d faces, bytes %s" % (
                name, *data["ref_sizes"][0], data["bvh"].shape[0], data["facesV"].shape[0], [os.path.getsize(p) for p in paths]))
        path = os.path.join(HERE, "refhost_face_cases.npz")
        np.savez_compressed(path, **face_fixture(scratch))
        print("%-26s %d faces x %d alphas, %d bytes" % ("refhost_face_cases", FACE_COUNT, len(FACE_ALPHAS), os.path.getsize(path)))
