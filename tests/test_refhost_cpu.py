"""The host replicas and the thick face box against the REFERENCE'S OWN COMPILED CODE.  CPU only.

tests/golden/refhost_*.npz record what the reference's loaders, its BVH builder and MathHelp::triCalcAABB — compiled unmodified
(oracle/refhost.py) — produce for its seven shipped models and for hand-made faces, next to the wire arrays this repository's
loader (host/model_io.cpp) and builder replica (host/bvh_builder.cpp) make of the same files.  From the fixtures alone, here:
loader arrays, materials, lights, tree topology, every box, face order and miss links equal the reference's; the thick face
box in numpy (patch_refit_ref.face_boxes) and on the host (ptp::faceBox) equals triCalcAABB's.  Where the reference and the
dumper exist, the dumper and this repository's loader + builder still reproduce the fixtures.

Values are compared with conftest.same_values: bit for bit, except that -0 equals +0 (a box bound that is a zero keeps
whichever zero a fold met first, and the reference's nested min / max and the refit's running fold meet them in another
order); index arrays with array_equal.

material_t fields that do NOT reach a wire array, and so are recorded in the fixtures but compared with nothing: mtlName (but
for the material called sky_light, whose Kd becomes pbr_config.sky_light — compared), Ka, Ns, illum and light.  light_t's
lightName does not reach the wire either; radius does only for an orb (type 2).
"""
import os
import sys
import tempfile

import numpy as np
import pytest

import flat_tree
import patch_refit_ref
import refhost_fixture as rf
from conftest import REFERENCE_MODELS, ROOT, same_values
from test_patch_refit_cpu import cxx_face_boxes, driver  # noqa: F401  (driver: the host unit's fixture)

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_refhost  # noqa: E402

from oracle import refhost  # noqa: E402

NAMES = tuple(make_refhost.CASES)
PHONG = tuple(n for n in NAMES if make_refhost.alpha_of(n) > 0.0)
# ref_material_floats columns (oracle/refhost/dump.cpp): Ka, Kd, Ks four words each, then d, Ni, Ns, rough, p, nu, nv, Rs, Rd
KA, KD, KS, D, NI, NS, ROUGH, P, NU, NV, RS, RD = slice(0, 4), slice(4, 8), slice(8, 12), 12, 13, 14, 15, 16, 17, 18, 19, 20

needs_reference = pytest.mark.skipif(not (os.path.isdir(REFERENCE_MODELS) and os.path.exists(refhost.BINARY)),
                                     reason="the reference's tree and the dumper built from it only exist in the build container")


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 and a.dtype.kind in "fiu" else a


def same_record(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(words(a), words(b))


def padded(a):
    out = np.zeros((a.shape[0], 4), np.float32)
    out[:, :3] = a
    return out


def sorted_rows(a):
    a = np.ascontiguousarray(a)
    return a[np.lexsort(a.T[::-1])]


# ---- where the reference exists: the fixtures are still what its code and this repository's produce -----------------------

@needs_reference
@pytest.mark.parametrize("name", NAMES)
def test_dumper_and_host_library_reproduce_the_fixture(cfg_defaults, name):
    """Every record of the dump and every wire array, byte for byte."""
    d = rf.load(name)
    with tempfile.TemporaryDirectory() as scratch:
        now = make_refhost.reference_dump(name, scratch)
    now.update(make_refhost.wire_arrays(cfg_defaults, name))
    now.update(make_refhost.settings_of(name))
    assert sorted(now) == sorted(d)
    for k in now:
        assert same_record(now[k], d[k]), k


@needs_reference
def test_dumper_reproduces_the_face_cases():
    d = rf.load("refhost_face_cases")
    with tempfile.TemporaryDirectory() as scratch:
        now = make_refhost.face_fixture(scratch)
    assert sorted(now) == sorted(d)
    for k in now:
        assert same_record(now[k], d[k]), k


def test_fixtures_hold_the_cases_asked_for():
    """Seven models at alpha 0, suzanne at 1.0, spheres and pillars at 0.6, suzanne without skip-ahead; the sizes the reference
    printed for them; 257 hand-made faces at alpha 0, 0.5 and 1."""
    sizes = {n: tuple(int(v) for v in rf.load(n)["ref_sizes"][0][:2]) for n in NAMES}
    assert sizes["refhost_suzanne"] == (1243, 622) and sizes["refhost_suzanne_a1.0"] == (1231, 616)
    assert sizes["refhost_pillars"] == (55, 28) and sizes["refhost_spheres"] == (919, 460)
    assert sizes["refhost_suzanne_noskip"] == (1243, 622)
    assert len(NAMES) == 11 and sorted(PHONG) == ["refhost_pillars_a0.6", "refhost_spheres_a0.6", "refhost_suzanne_a1.0"]
    d = rf.load("refhost_suzanne")
    assert d["ref_facesV"].shape[0] == 1082 and len(d["ref_object_names"]) == 10 and int(d["ref_tree_nodes"][:, rf.SKIP_NEXT_LEFT].sum()) == 166
    assert int(rf.load("refhost_suzanne_noskip")["ref_tree_nodes"][:, rf.SKIP_NEXT_LEFT].sum()) == 0
    f = rf.load("refhost_face_cases")
    assert f["corners"].shape == f["normals"].shape == (257, 3, 3) and f["boxes"].shape == (3, 257, 6)
    assert f["alphas"].tolist() == [0.0, 0.5, 1.0]
    for name in NAMES + ("refhost_face_cases",):
        files = rf.files_of(name)
        assert len(files) == (3 if "applejack" in name else 1)                            # 8 k faces do not fit one file under the cap
        for path in files:
            assert os.path.getsize(path) < make_refhost.SIZE_CAP, path                    # the largest fixture before these


# ---- the loader -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_loader_arrays_equal_objparsers(name):
    d = rf.load(name)
    assert same_values(d["vertices"], padded(d["ref_vertices"])) and same_values(d["normals"], padded(d["ref_normals"]))
    assert np.array_equal(words(d["vertices"]), words(padded(d["ref_vertices"])))        # parsed numbers: the very bits
    assert np.array_equal(words(d["normals"]), words(padded(d["ref_normals"])))
    # (v0, v1, v2, material, n0, n1, n2) of every face, as multisets: the builder only reorders
    faces = d["ref_facesV"].shape[0]
    assert d["ref_facesVN"].shape[0] == d["ref_facesMtl"].shape[0] == faces == d["facesV"].shape[0] == d["facesN"].shape[0]
    want = np.concatenate([d["ref_facesV"], d["ref_facesMtl"].astype(np.uint32), d["ref_facesVN"]], axis=1)
    got = np.concatenate([d["facesV"], d["facesN"][:, :3]], axis=1)
    assert np.array_equal(sorted_rows(got), sorted_rows(want))
    assert (d["facesN"][:, 3] == 0).all()
    # objects: consecutive face ranges over all faces, one normal triple per face
    r = d["ref_object_ranges"]
    assert np.array_equal(r[:, 0], np.concatenate([[0], np.cumsum(r[:, 1])[:-1]])) and r[:, 1].sum() == faces
    assert np.array_equal(r[:, 1], r[:, 2]) and len(d["ref_object_names"]) == r.shape[0]


@pytest.mark.parametrize("name", NAMES)
def test_materials_equal_material_t(name):
    """pbr_material_sa: d, Ni, nu, nv, Rs, Rd, -, -, rgbDiff = Kd, rgbSpec = Ks (16 words); pbr_material_schlick: d, Ni, p,
    rough, rgbDiff, rgbSpec (12 words) — include/pbr_hip.h.  A key the .mtl omits has MtlParser::getEmptyMaterial's default in
    the dump, so the defaults are compared with everything else.  The two spare words of the Shirley-Ashikhmin record, which
    the reference leaves unwritten, are zero here."""
    d = rf.load(name)
    m = d["ref_material_floats"]
    count = m.shape[0]
    assert count > 0 and d["materials"].shape == (count, 16) and d["materials_schlick"].shape == (count, 12)
    zero = np.zeros((count, 1), np.float32)
    col = lambda k: m[:, k:k + 1]
    want_sa = np.concatenate([col(D), col(NI), col(NU), col(NV), col(RS), col(RD), zero, zero, m[:, KD], m[:, KS]], axis=1)
    want_schlick = np.concatenate([col(D), col(NI), col(P), col(ROUGH), m[:, KD], m[:, KS]], axis=1)
    assert np.array_equal(words(d["materials"]), words(want_sa))
    assert np.array_equal(words(d["materials_schlick"]), words(want_schlick))
    # every face's material index names a material, or is -1 (no usemtl before it)
    assert ((d["ref_facesMtl"] >= -1) & (d["ref_facesMtl"] < count)).all()
    # sky_light: the Kd of the material of that name, else white (PathTracer.cpp:468-474, :497-503, :514-516)
    names = d["ref_material_names"].tolist()
    sky = m[names.index("sky_light"), KD] if "sky_light" in names else np.array([1, 1, 1, 0], np.float32)
    assert np.array_equal(words(d["sky_light"][:3]), words(sky[:3])) and d["sky_light"][3] == 0.0
    assert d["ref_material_ints"].shape == (count, 2)


def test_material_defaults_and_flags_are_in_the_fixtures():
    """The shipped .mtl files omit keys and set `light`: the dump has getEmptyMaterial's defaults (MtlParser.cpp: Ns 100, Ni 1,
    d 1, illum 2, light 0, rough 1, p 1, nu 0, nv 0, Rs 0, Rd 1, white Ka / Kd / Ks) where a key is missing — so
    test_materials_equal_material_t holds the wire arrays to them — and both values of the flag occur."""
    floats = np.concatenate([rf.load(n)["ref_material_floats"] for n in NAMES])
    ints = np.concatenate([rf.load(n)["ref_material_ints"] for n in NAMES])
    for column, default in ((ROUGH, 1.0), (P, 1.0), (NU, 0.0), (NV, 0.0), (RS, 0.0), (RD, 1.0), (NI, 1.0), (D, 1.0)):
        assert (floats[:, column] == default).any() and (floats[:, column] != default).any(), column
    assert set(ints[:, 1].tolist()) == {0, 1} and (ints[:, 0] == 2).any()
    assert (floats[:, [3, 7, 11]] == 0.0).all()                                           # the colours' .w


@pytest.mark.parametrize("name", NAMES)
def test_lights_equal_light_t(name):
    """pbr_light: pos, rgb, data = ( type, orb radius, 0, 0 ) (PathTracer.cpp:387-428)."""
    d = rf.load(name)
    lf, types = d["ref_light_floats"], d["ref_light_types"][:, 0]
    assert d["lights"].shape == (lf.shape[0], 12) and (lf.shape[0] == 1) == ("suzanne" in name)
    assert np.isin(types, (1, 2)).all()
    data = np.zeros((lf.shape[0], 4), np.float32)
    data[:, 0] = types
    data[:, 1] = np.where(types == 2, lf[:, 8], np.float32(0.0))
    assert np.array_equal(words(d["lights"]), words(np.concatenate([lf[:, 0:8], data], axis=1)))


# ---- the tree ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_tree_equals_the_references(name):
    d = rf.load(name)
    t = d["ref_tree_nodes"].astype(np.int64)
    nodes, leaves, depth = (int(v) for v in d["ref_sizes"][0])
    assert t.shape[0] == nodes == 2 * leaves - 1 and int((t[:, rf.FACES] > 0).sum()) == leaves and int(t[:, rf.DEPTH].max()) == depth
    assert ((t[:, rf.FACES] > 0) == (t[:, rf.LEFT] == rf.NONE)).all() and (t[:, rf.FACES] <= 2).all()
    want = rf.flatten(d)
    bvh = d["bvh"]
    # the node count, after the nodes PathTracer drops for skipNextLeft
    skipped = int(t[:, rf.SKIP_NEXT_LEFT].sum())
    assert bvh.shape[0] == want.kept.size == nodes - skipped
    assert (skipped > 0) == ("noskip" not in name)
    # this repository's tree, from its depth-first order, leaf flags and links alone, is the reference's tree without those nodes
    leaf, end, parent = rf.unflatten(bvh)
    assert np.array_equal(leaf, t[want.kept, rf.FACES] > 0)
    assert np.array_equal(parent, want.parent)
    if rf.alpha_of(d) == 0.0:
        flat_tree.check_flat_tree(bvh, d["facesV"], d["facesV"], d["vertices"], sample=None)
    # every bbMin and bbMax
    boxes = d["ref_tree_boxes"][want.kept]
    assert same_values(bvh[:, 0:3], boxes[:, 0:3]) and same_values(bvh[:, 4:7], boxes[:, 3:6])
    # every leaf holds the same one or two faces in the same order; facesV / facesN in leaf order are the leaves' Tri sequence
    assert np.array_equal(words(bvh[:, 3]), words(want.bvh[:, 3]))
    assert np.array_equal(words(bvh[leaf, 7]), words(want.bvh[leaf, 7]))
    assert np.array_equal(d["facesV"], want.facesV) and np.array_equal(d["facesN"], want.facesN)
    assert np.array_equal(d["facesV"][:, :3], d["ref_tri_face"][want.tri, :3])
    assert np.array_equal(d["facesN"][:, :3], d["ref_tri_normals"][want.tri, :3])
    assert np.array_equal(want.tri, np.arange(want.tri.size)), "skip-ahead drops containers only"
    # a container's miss link: the right sibling's id - numSkipsToHere
    assert np.array_equal(words(bvh[~leaf, 7]), words(want.bvh[~leaf, 7]))
    assert np.array_equal(end[~leaf & (bvh[:, 7] != -1)], bvh[~leaf & (bvh[:, 7] != -1), 7].astype(np.int64))


def test_skip_ahead_only_drops_nodes():
    """With and without bvh.skip_ahead the reference builds the same tree, flags apart; the flat arrays differ by the dropped
    nodes and the links counted without them."""
    on, off = rf.load("refhost_suzanne"), rf.load("refhost_suzanne_noskip")
    for k in ("ref_tree_boxes", "ref_tri_face", "ref_tri_normals", "ref_tri_boxes"):
        assert same_record(on[k], off[k]), k
    same = [rf.ID, rf.DEPTH, rf.PARENT, rf.LEFT, rf.RIGHT, rf.FACES]
    assert np.array_equal(on["ref_tree_nodes"][:, same], off["ref_tree_nodes"][:, same])
    assert (off["ref_tree_nodes"][:, rf.SKIPS_TO_HERE] == 0).all()
    assert np.array_equal(on["facesV"], off["facesV"]) and off["bvh"].shape[0] - on["bvh"].shape[0] == 166


def test_suzanne_known_answer_from_the_fixture():
    """What tests/test_host_bvh.py's (622, 1243) cites: the reference's own builder gives suzanne.obj 622 leaves and 1243 nodes."""
    assert tuple(int(v) for v in rf.load("refhost_suzanne")["ref_sizes"][0][:2]) == (1243, 622)


# ---- the boxes --------------------------------------------------------------------------------------------------------------

def tri_arrays(d):
    """(facesV, facesN, vertices, normals) of the dump's Tris over ObjParser's arrays, in the dump's order."""
    return d["ref_tri_face"], d["ref_tri_normals"], padded(d["ref_vertices"]), padded(d["ref_normals"])


@pytest.mark.parametrize("name", NAMES)
def test_tri_boxes_numpy_and_host_unit(driver, name):  # noqa: F811
    """Every Tri box of every fixture: patch_refit_ref.face_boxes and ptp::faceBox equal triCalcAABB's at the fixture's alpha;
    at alpha 0 that box is the exact bound of the three corners."""
    d = rf.load(name)
    alpha = rf.alpha_of(d)
    args = tri_arrays(d)
    want_lo, want_hi = d["ref_tri_boxes"][:, 0:3], d["ref_tri_boxes"][:, 3:6]
    lo, hi = patch_refit_ref.face_boxes(*args, alpha)
    assert same_values(lo, want_lo) and same_values(hi, want_hi)
    lo, hi = cxx_face_boxes(driver, *args, alpha)
    assert same_values(lo, want_lo) and same_values(hi, want_hi)
    corners = args[2][args[0][:, :3].astype(np.int64), :3]
    tight = same_values(corners.min(1), want_lo) and same_values(corners.max(1), want_hi)
    assert tight == (alpha == 0.0 or "pillars" in name)                                  # the pillars' faces have equal normals
    assert (want_lo <= corners.min(1)).all() and (want_hi >= corners.max(1)).all()


def face_case_arrays(f):
    count = f["corners"].shape[0]
    vertices, normals = np.zeros((3 * count, 4), np.float32), np.zeros((3 * count, 4), np.float32)
    vertices[:, :3], normals[:, :3] = f["corners"].reshape(-1, 3), f["normals"].reshape(-1, 3)
    faces = np.zeros((count, 4), np.uint32)
    faces[:, :3] = np.arange(3 * count).reshape(count, 3)
    return faces, faces.copy(), vertices, normals


@pytest.mark.parametrize("k", (0, 1, 2))
def test_hand_made_faces_numpy_and_host_unit(driver, k):  # noqa: F811
    f = rf.load("refhost_face_cases")
    alpha = float(f["alphas"][k])
    want = f["boxes"][k]
    assert not np.isnan(want).any(), f["labels"][np.isnan(want).any(axis=1)]
    args = face_case_arrays(f)
    for what, (lo, hi) in (("numpy", patch_refit_ref.face_boxes(*args, alpha)), ("host unit", cxx_face_boxes(driver, *args, alpha))):
        bad = ~((lo == want[:, 0:3]).all(axis=1) & (hi == want[:, 3:6]).all(axis=1))
        assert not bad.any(), (what, alpha, f["labels"][bad].tolist(), lo[bad], hi[bad], want[bad])


def test_what_the_reference_does_with_the_hand_made_faces():
    """Recorded behaviour of triCalcAABB, from the fixture: which faces get a box beyond their corners' bound at alpha 0.5.  Equal
    normals and normals within 1e-6 do not; normals whose differences cancel in ( n1 - n2 ) + ( n2 - n3 ) — n1 = n3 with n2
    anywhere — do not either, although the patch is curved: the reference's test cannot see them, and the replica follows it.
    A face without area does not grow here: its raised corners and apex are NaN and enter no min / max, and its edge points stay
    inside (at alpha 1 the face with two equal corners grows by its edge points alone).  No box word is NaN."""
    f = rf.load("refhost_face_cases")
    labels = f["labels"].tolist()
    corners = f["corners"]
    grown = lambda boxes: ~((boxes[:, 0:3] == corners.min(1)).all(axis=1) & (boxes[:, 3:6] == corners.max(1)).all(axis=1))
    named = len(set(labels))
    assert labels[named:] == ["ordinary"] * (257 - named) and labels.index("ordinary") == 0
    stay = {"equal normals", "normals differ by 5e-7", "n1 = n3, n2 leaning", "n1 = n3, n2 opposite", "two equal corners",
            "three equal corners", "collinear corners", "all zero normals"}
    half = grown(f["boxes"][1])
    assert {l for l, g in zip(labels[:named], half[:named]) if not g} == stay and half[named:].all()
    full = grown(f["boxes"][2])
    assert full[labels.index("two equal corners")] and not full[labels.index("n1 = n3, n2 opposite")] and not full[labels.index("equal normals")]
    assert not grown(f["boxes"][0]).any()                                                  # alpha 0: the corners' bound
    for boxes in f["boxes"]:
        assert not np.isnan(boxes).any()
        assert (boxes[:, 0:3] <= corners.min(1)).all() and (boxes[:, 3:6] >= corners.max(1)).all()
        assert (boxes[named:] == boxes[0]).all()                                           # the copies: the same box 237 times
