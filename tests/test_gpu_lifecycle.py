"""A context that is used again after everything it can hold was allocated, that drops one kind of move among three, and that is
destroyed with everything live.

Every buffer of the context belongs to one of two lifetimes — the scene's and the configuration's — or to one of the three kinds
of move, and is given back when that lifetime ends.  What is left behind must not show: a context that has held the tables of
every update kind, the re-link, the adaptive render, the temporal history with its motion planes and the focus chain renders the
next scene at the next size bit for bit as a context that never held any of it, and reports the same.

The two smallest fixtures of test_gpu_update_sequence.py and its helpers; images of 16 x 16 (2 x 2 tiles) and 24 x 16."""
import pytest

import skin_dq_ref
from test_gpu_morph import NO_MORPH
from test_gpu_skin import NO_SKIN
from test_gpu_skin_dq import FAR, NO_DQ
from test_gpu_transforms import device, other, same_bits  # noqa: F401 (the two are fixtures)
from test_gpu_update_sequence import FIXTURES, NO_PARTS, arguments, call, case, prepared

pytestmark = pytest.mark.gpu

A, B = FIXTURES
TRAVERSAL = 2                       # eight orders: an update re-links them while pbr_refit_ordered_walk is on
FRAMES = 4
NO_RELINK_TABLES = {"table_bytes": 0, "levels": 0}
LAST_RELINK = ("launches", "relinked", "ms")
_reference = {}


def seeds(pbr):
    return pbr.frame_seeds(0, FRAMES)


def render_b(pbr, dev):
    """configure( 24 x 16 ), upload B, render: what the context shows of it."""
    c = case(pbr, B)
    dev.configure(c.sc.config(width=24, height=16, traversal=TRAVERSAL, phong_tessellation=0.0))
    dev.upload_scene(c.sc.desc)
    dev.render(0, seeds(pbr), pbr.pixel_dimension(24, 16), c.sc.cam)
    relink = dev.relink_info()
    return {"output": dev.read_output(), "debug": dev.read_debug(), "counters": dev.counters(), "geometry": dev.read_geometry(),
            "transform": dev.transform_info(), "skin": dev.skin_info(), "skin_dq": dev.skin_dq_info(), "morph": dev.morph_info(),
            "patches": {k: dev.patch_refit_info()[k] for k in ("device_bytes", "updates")},
            "relink_tables": {k: relink[k] for k in NO_RELINK_TABLES}, "last_relink": {k: relink[k] for k in LAST_RELINK}, "refits": dev.refit_info()["updates"],
            "refit": {k: v for k, v in dev.refit_info().items() if k != "upload_ms"}, "scene_bytes": dev.scene_bytes()}


def reference(pbr, gpu_device):
    """B on a context that only configured, uploaded and rendered.  Computed once and shared; nobody writes to the arrays."""
    if not _reference:
        dev = pbr.Device(gpu_device)
        _reference.update(render_b(pbr, dev))
        dev.close()
    return _reference


def same_as_reference(got, want, what):
    for key in ("output", "debug"):
        same_bits(got[key], want[key], "%s: %s" % (what, key))
    for got_array, want_array, key in zip(got["geometry"], want["geometry"], ("vertices", "normals")):
        same_bits(got_array, want_array, "%s: %s" % (what, key))
    for key in ("counters", "transform", "skin", "skin_dq", "morph", "patches", "relink_tables", "refits", "refit", "scene_bytes"):
        assert got[key] == want[key], "%s: %s" % (what, key)


def everything_live(pbr, dev, spare):
    """On `dev`: scene A under a ray-ordered traversal with the re-link on; parts, a skin and a morph with normals; one update of
    each of the eight kinds; an adaptive render; temporal denoising on the static and on the motion path; a depth-of-field render."""
    c = case(pbr, A)
    px, cam, s = pbr.pixel_dimension(16, 16), c.sc.cam, seeds(pbr)
    dev.refit_ordered_walk(True)
    dev.temporal_track_motion(True)
    prepared(c, dev, spare)
    dev.configure(c.sc.config(width=16, height=16, traversal=TRAVERSAL, phong_tessellation=0.0))
    for i, kind in enumerate("VGTSMP"):
        call(dev, kind)(*arguments(c, kind, i)[0])
        assert dev.relink_info()["relinked"], kind
    Q = skin_dq_ref.dual_quats_for(c.bones, 1, FAR)
    dev.update_skin_dq(Q)
    dev.update_pose_dq(c.sets[1], Q)
    dev.render_adaptive(0, s, px, cam, 2, 2, FRAMES, 0.05)
    dev.denoise_temporal(px, cam)
    dev.update_vertices(arguments(c, "V", 1)[1])                        # the history's positions are kept, the next call follows the faces
    dev.render_adaptive(0, s, px, cam, 2, 2, FRAMES, 0.05)
    dev.denoise_temporal(px, cam)
    assert (dev.temporal_motion()[1] >= 0).any()
    focus = pbr.Camera.from_buffer_copy(cam)
    focus.focusPoint[0], focus.focusPoint[1] = 8, 8
    dev.render_dof(0, s, px, focus)
    assert dev.last_focus_chain_ms() > 0.0
    # all of it is there
    infos = dev.transform_info(), dev.skin_info(), dev.morph_info(), dev.patch_refit_info()
    assert all(info["device_bytes"] > 0 and info["updates"] > 0 for info in infos)
    assert dev.skin_dq_info()["updates"] == 2 and dev.relink_info()["table_bytes"] > 0 and dev.refit_info()["updates"] == 10
    assert dev.scene_bytes()["walk_streams"] > 0


def test_a_context_that_held_everything_renders_the_next_scene_as_a_fresh_one(pbr, gpu_device, device, other):
    """Image, debug image, counters, geometry and every info call as on a fresh context — but for what pbr_diag_relink_info says of
    the LAST UPDATE's re-link (launches, relinked, ms): that is no property of the scene, no upload has ever reset it, and a fresh
    context reports 0 / False / 0.0 there.  It is held to what it was before the upload, so that it does not move unnoticed."""
    want = reference(pbr, gpu_device)
    everything_live(pbr, device, other)
    last_relink = {k: device.relink_info()[k] for k in LAST_RELINK}
    got = render_b(pbr, device)
    same_as_reference(got, want, "after everything was allocated")
    assert got["last_relink"] == last_relink and last_relink["relinked"] and last_relink["launches"] > 0
    assert want["last_relink"] == {"launches": 0, "relinked": False, "ms": 0.0}
    assert got["transform"] == NO_PARTS and got["skin"] == NO_SKIN and got["skin_dq"] == NO_DQ and got["morph"] == NO_MORPH
    assert got["patches"] == {"device_bytes": 0, "updates": 0} and got["relink_tables"] == NO_RELINK_TABLES and got["refits"] == 0


def test_dropping_a_kind_leaves_the_other_two_and_the_geometry(pbr, device, other):
    c = case(pbr, A)
    prepared(c, device, other)
    info = {"T": device.transform_info, "S": device.skin_info, "M": device.morph_info}
    drop = {"T": device.set_parts, "S": device.set_skin, "M": device.set_morph}
    empty = {"T": dict(NO_PARTS, last_update=True), "S": dict(NO_SKIN, last_update=True), "M": dict(NO_MORPH, last_update=1)}
    for i, kind in enumerate("TSM"):
        call(device, kind)(*arguments(c, kind, i)[0])
        assert info[kind]()["device_bytes"] > 0 and info[kind]()["updates"] == 1
        others = {k: info[k]() for k in "TSM" if k != kind}
        geometry, nodes, patches, refit = device.read_geometry(), device.read_bvh(), device.read_patches(), device.refit_info()
        drop[kind](None)
        assert info[kind]() == empty[kind], kind
        assert {k: info[k]() for k in "TSM" if k != kind} == others, kind
        for got, held, what in zip(device.read_geometry(), geometry, ("vertices", "normals")):
            same_bits(got, held, "dropping %s: %s" % (kind, what))
        same_bits(device.read_bvh(), nodes, "dropping %s: boxes" % kind)
        same_bits(device.read_patches(), patches, "dropping %s: patches" % kind)
        assert device.refit_info() == refit, kind


def test_a_context_is_destroyed_with_everything_live(pbr, gpu_device, device, other):
    want = reference(pbr, gpu_device)
    everything_live(pbr, device, other)
    device.close()
    after = pbr.Device(gpu_device)
    try:
        same_as_reference(render_b(pbr, after), want, "a context created after the destroyed one")
    finally:
        after.close()
