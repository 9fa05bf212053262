"""The six update calls one after the other on one context that has parts, a skin and a morph set at once: every kind directly
behind every kind, a refused update in the middle, and a pbr_set_*( 0 ) behind an update of its kind.

Each kind of move owns a rest pose, a staging buffer and a flag word, and an accepted update swaps its staging buffer with the
context's vertices — so after an update a kind's staging buffer is what the context's vertices were, left there by whichever kind
ran before.  Whatever ran before, the next update must start from its own rest pose, write the bits its numpy restatement gives,
leave boxes and patches that equal pbr_update_geometry's, and be the one update the four info calls report as the last.

The two smallest fixtures: nothing here depends on size (the sizes have their tests in test_gpu_transforms.py, test_gpu_skin.py
and test_gpu_morph.py)."""
import types

import numpy as np
import pytest

import morph_ref
import patch_refit_ref
import refit_ref
import refit_scenes
import skin_ref
import transform_ref
from test_gpu_morph import NO_MORPH, geometry_is
from test_gpu_skin import NO_SKIN
from test_gpu_transforms import device, other, same_bits  # noqa: F401 (the two are fixtures)

FIXTURES = ("ref_pillars_sa", "ref_spheres_schlick")
NO_PARTS = {"parts": 0, "device_bytes": 0, "updates": 0, "last_update": False, "ms": 0.0}
# V pbr_update_vertices, G pbr_update_geometry, T pbr_update_transforms, S pbr_update_skin, M pbr_update_morph, P pbr_update_pose:
# 37 calls in which each of the 36 ordered pairs stands side by side once
SEQUENCE = "GGTTSSMMPPVVGSPGMVTMGPTPSVSGVMTVPMSTG"
OVERFLOW = transform_ref._matrix([[3e38, 3e38, 3e38], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], (0.0, 0.0, 0.0))
_cases = {}


def test_the_sequence_holds_every_ordered_pair():
    assert len(SEQUENCE) == 37 and {SEQUENCE[i:i + 2] for i in range(36)} == {a + b for a in "VGTSMP" for b in "VGTSMP"}


def case(pbr, name):
    """The fixture with parts, influences and targets, and the pose the parts capture: they are set one update_geometry later
    than the skin and the morph, so their rest pose is another one.  Computed once and shared; nobody writes to the arrays."""
    if name not in _cases:
        sc = refit_scenes.load(pbr, name)
        a = sc.arrays
        c = types.SimpleNamespace(sc=sc, a=a)
        V, N = a["vertices"].shape[0], a["normals"].shape[0]
        c.vertex_part, c.normal_part, c.parts = transform_ref.parts_of(name, a["facesV"], a["facesN"], V, N)
        c.vb, c.vw, c.nb, c.nw, c.bones = skin_ref.influences_for(name, a["facesV"], a["facesN"], V, N)
        c.vt, c.nt = morph_ref.targets_for(name, a["vertices"], a["normals"])
        c.sets = list(morph_ref.weights_for(len(c.vt)).values())
        c.parts_v = refit_ref.deform(a["facesV"], a["vertices"], "small", 11)
        c.parts_n = patch_refit_ref.perturb_normals(a["normals"], seed=11)
        _cases[name] = c
    return _cases[name]


def prepared(c, device, other):
    """Both uploaded and configured; on `device` a skin and a morph on the upload's pose, one update_geometry, parts on that one."""
    for dev in (device, other):
        dev.upload_scene(c.sc.desc)
        dev.configure(c.sc.config(phong_tessellation=0.0))              # pbr_update_vertices is part of the sequence
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.set_morph(c.vt, c.nt)
    device.update_geometry(c.parts_v, c.parts_n)
    device.set_parts(c.vertex_part, c.normal_part, c.parts)
    return types.SimpleNamespace(refits=1, geometry=1, T=0, S=0, MP=0, last="G", n=c.parts_n)


def arguments(c, kind, i):
    """The i-th call's arguments — they change from call to call — and the restatement's ( V', N' or None: the normals stay )
    from that kind's own rest pose."""
    a = c.a
    w = c.sets[i % len(c.sets)] * np.float32(1.0 + 0.25 * (i // len(c.sets)))
    if kind == "V":
        v = refit_ref.deform(a["facesV"], a["vertices"], "large" if i % 2 else "small", 20 + i)
        return (v,), v, None
    if kind == "G":
        v, n = refit_ref.deform(a["facesV"], a["vertices"], "small", 20 + i), patch_refit_ref.perturb_normals(a["normals"], seed=20 + i)
        return (v, n), v, n
    if kind == "T":
        M = transform_ref.matrices_for(c.parts, i)
        return (M,), *transform_ref.transform(c.parts_v, c.vertex_part, c.parts_n, c.normal_part, M)
    M = transform_ref.matrices_for(c.bones, i, ("translation of 1e6",))
    if kind == "S":
        return (M,), *skin_ref.skin(a["vertices"], c.vb, c.vw, a["normals"], c.nb, c.nw, M)
    morphed = morph_ref.morph(a["vertices"], c.vt, a["normals"], c.nt, w)
    if kind == "M":
        return (w,), *morphed
    return (w, M), *skin_ref.skin(morphed[0], c.vb, c.vw, morphed[1], c.nb, c.nw, M)


def call(dev, kind):
    return {"V": dev.update_vertices, "G": dev.update_geometry, "T": dev.update_transforms, "S": dev.update_skin, "M": dev.update_morph, "P": dev.update_pose}[kind]


def infos(dev):
    t, s, m, p, r = dev.transform_info(), dev.skin_info(), dev.morph_info(), dev.patch_refit_info(), dev.refit_info()
    return {"T": (t["updates"], t["last_update"]), "S": (s["updates"], s["last_update"]), "MP": (m["updates"], m["last_update"]),
            "geometry": (p["updates"], p["last_update"]), "refits": r["updates"]}


def expected_infos(state):
    return {"T": (state.T, state.last == "T"), "S": (state.S, state.last == "S"), "MP": (state.MP, {"M": 1, "P": 2}.get(state.last, 0)),
            "geometry": (state.geometry, state.last != "V"), "refits": state.refits}


def step(c, device, other, state, kind, i):
    """One accepted call on `device`, pbr_update_geometry with the restatement's arrays on `other`, and everything the call
    promises."""
    what = "call %d (%s after %s)" % (i, kind, state.last)
    args, v, n = arguments(c, kind, i)
    patches = device.read_patches()
    call(device, kind)(*args)
    state.n = state.n if n is None else n
    state.refits += 1
    state.geometry += kind != "V"
    state.T, state.S, state.MP, state.last = state.T + (kind == "T"), state.S + (kind == "S"), state.MP + (kind in "MP"), kind
    geometry_is(device, v, state.n, what)
    other.update_geometry(v, state.n)
    same_bits(device.read_bvh(), other.read_bvh(), what + ": boxes")
    # pbr_update_vertices alone leaves the patches as they were
    same_bits(device.read_patches(), patches if kind == "V" else other.read_patches(), what + ": patches")
    assert infos(device) == expected_infos(state), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_every_kind_after_every_other(pbr, device, other, name):
    c = case(pbr, name)
    state = prepared(c, device, other)
    assert infos(device) == expected_infos(state)
    for i, kind in enumerate(SEQUENCE):
        step(c, device, other, state, kind, i)
    assert state.refits == 38 and (state.T, state.S, state.MP) == (6, 6, 12)
    for info in (device.transform_info(), device.skin_info(), device.morph_info()):
        assert info["ms"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_a_refused_update_in_the_middle_changes_nothing(pbr, device, other, name):
    """Finite matrices whose product with the rest pose is not: the refusal the device finds, behind an accepted update of
    another kind and in front of one."""
    c = case(pbr, name)
    a = c.a
    state = prepared(c, device, other)
    w = c.sets[1]
    parts_m, bones_m = np.tile(OVERFLOW, (c.parts, 1)), np.tile(OVERFLOW, (c.bones, 1))
    assert transform_ref.refused(parts_m) is None and skin_ref.refused(bones_m) is None
    assert transform_ref.not_finite(transform_ref.positions(c.parts_v, c.vertex_part, parts_m)).any()
    assert transform_ref.not_finite(skin_ref.positions(a["vertices"], c.vb, c.vw, bones_m)).any()
    assert transform_ref.not_finite(skin_ref.positions(morph_ref.positions(a["vertices"], c.vt, w), c.vb, c.vw, bones_m)).any()
    refusals = (("T", (parts_m,), "pbr_update_transforms: a transformed position is not finite", "M", "S"),
                ("S", (bones_m,), "pbr_update_skin: a skinned position is not finite", "T", "P"),
                ("P", (w, bones_m), "pbr_update_pose: a posed position is not finite", "S", "T"))
    for i, (kind, args, message, before, after) in enumerate(refusals):
        step(c, device, other, state, before, 3 * i)
        geometry, nodes, patches, held = device.read_geometry(), device.read_bvh(), device.read_patches(), infos(device)
        times = device.transform_info()["ms"], device.skin_info()["ms"], device.morph_info()["ms"]
        with pytest.raises(pbr.PbrError, match="-1: .*" + message) as refused:
            call(device, kind)(*args)
        assert "found on the device" in str(refused.value)
        what = "a refused " + kind
        geometry_is(device, geometry[0], geometry[1], what)
        same_bits(device.read_bvh(), nodes, what)
        same_bits(device.read_patches(), patches, what)
        assert infos(device) == held == expected_infos(state), what
        assert (device.transform_info()["ms"], device.skin_info()["ms"], device.morph_info()["ms"]) == times, what
        step(c, device, other, state, after, 3 * i + 1)


@pytest.mark.gpu
def test_dropping_a_kind_behind_its_update_keeps_the_last_update(pbr, device, other):
    """pbr_set_*( 0 ) frees the kind and resets its counters, not what the last update was; a new upload does."""
    c = case(pbr, "ref_pillars_sa")
    state = prepared(c, device, other)
    step(c, device, other, state, "T", 0)
    device.set_parts(None)
    state.T = 0
    assert device.transform_info() == dict(NO_PARTS, last_update=True)
    step(c, device, other, state, "S", 1)
    assert device.transform_info() == NO_PARTS
    device.set_skin(None)
    state.S = 0
    assert device.skin_info() == dict(NO_SKIN, last_update=True)
    step(c, device, other, state, "M", 2)
    assert device.skin_info() == NO_SKIN
    device.set_morph(None)
    assert device.morph_info() == dict(NO_MORPH, last_update=1)
    assert device.patch_refit_info()["last_update"] is True and device.refit_info()["updates"] == state.refits
    # the pose reports 2, and the dropped skin is not its update
    device.set_skin(c.vb, c.vw, c.nb, c.nw, c.bones)
    device.set_morph(c.vt, c.nt)
    device.update_pose(c.sets[1], transform_ref.matrices_for(c.bones, 1, ("translation of 1e6",)))
    device.set_skin(None)
    assert device.skin_info() == NO_SKIN
    device.set_morph(None)
    assert device.morph_info() == dict(NO_MORPH, last_update=2)
    device.upload_scene(c.sc.desc)
    assert device.transform_info() == NO_PARTS and device.skin_info() == NO_SKIN and device.morph_info() == NO_MORPH
    assert device.patch_refit_info()["last_update"] is False and device.refit_info()["updates"] == 0
