"""A round of the two-paths kernel (csrc/pt_dual.hpp, pathTracingDual, plan 6) outside its hand-written loop: the node
phase takes the walks' masks and the slots' own cursor, leaf word and tNear as its operands, its test is wave-uniform, and
the node stream's address is read once per launch and held in scalar registers across rounds.  The shapes at which that
bookkeeping can go wrong, every one with plan 6 pinned and against the CPU oracle at tolerance 0 — image, debug image and the
four counters:

  fewer units than slots   8 x 8 px x 1 frame: slot B never gets work and stays MODE_DONE from the start
  mixed slot use           8 x 8 x 3 frames: lanes with one slot used and lanes with two
  refill                   16 x 8 x 64 frames: slots are refilled through nextSlot
  no cold lane             the Cornell scene, whose tree is resident as a whole: the global loads issue with EXEC = 0
  no resident lane         knob lds_slots = 0: every lane is cold
  hand-made trees          tests/hand_scenes.py: the root's only child is a leaf (walks of one visit — the walk starts at
                           node 1, so this is the tree whose walk begins on a leaf), one-face leaves only, two-face leaves only
                           (a leaf phase in every round)
  all six variants         BRDF 0 and 1 x { no lights, lights, lights + shadow rays }: each is its own register allocation
  chained flavour          pbr_render_dof with the focus point at the centre
  state across launches    two renders in one context, then another scene uploaded into it: nothing held over a launch
                           may outlive it

One oracle render per scene and size, shared by the cases that use it."""
import numpy as np
import pytest

import hand_scenes
import refit_ref
import refit_scenes
from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

DUAL = 6
STAGED = 1016            # records the two-paths kernel stages at most (its path slots take the rest of the LDS)

# kind, seed, triangles: the generated scenes of test_gpu_node_phase_fetch_order.py
CORNELL = ("cornell", 1, 0)
MID = ("hairball", 3, 2400)         # 2012 records: cold and resident lanes in plan 6

_references = {}


def reference(pbr, oracle, scene, w, h, frames, brdf=1, lights=False, shadow=False, focus=None):
    """The scene, what a render of it needs, and the oracle's image, debug image and counters — computed once."""
    key = (scene, w, h, frames, brdf, lights, shadow, focus)
    if key in _references:
        return _references[key]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3, "render.brdf": brdf})
    sc = pbr.HostScene.generate(*scene)
    cfg, cam, px = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h)
    pbr.cfg_reset()
    desc, keep = sc.desc, None
    if lights:
        # an orb light and a point light (as tests/test_gpu_parity.py has them); shadow rays walk the tree once more
        keep = np.zeros((2, 12), np.float32)
        keep[0] = [0.1, 1.6, 0.2, 0, 4.0, 3.5, 3.0, 0, 2, 0.12, 0, 0]
        keep[1] = [-0.5, 0.4, 0.6, 0, 1, 1, 1, 0, 1, 0, 0, 0]
        desc = pbr.SceneDesc.from_buffer_copy(sc.desc)
        desc.lights, desc.num_lights = keep.ctypes.data, 2
    cfg.shadow_rays = 1 if shadow else 0
    if focus is not None:
        cam = pbr.Camera.from_buffer_copy(cam)
        cam.focusPoint[0], cam.focusPoint[1] = focus
    seeds = pbr.frame_seeds(0, frames)
    ref = oracle.Renderer(desc, cfg, threads=8)
    image = ref.render(0, seeds, px, cam)
    image.setflags(write=False)
    debug = np.array(ref.debug, copy=True)
    debug.setflags(write=False)
    counters = dict(ref.counter_dict())
    assert counters["hits"] > 0
    _references[key] = (sc, keep, desc, cfg, cam, px, seeds, (image, debug, counters))
    return _references[key]


def assert_same_render(dev, want, what=""):
    image, debug, counters = want
    got = dev.read_output()
    assert same_values(got, image), "%s image: %s" % (what, describe_mismatch(got, image))
    got = dev.read_debug()
    assert same_values(got, debug), "%s debug image: %s" % (what, describe_mismatch(got, debug))
    assert dev.counters() == counters, what


def check(pbr, oracle, gpu_device, scene, w, h, frames, lds_slots=None, dof=False, **variant):
    _, _, desc, cfg, cam, px, seeds, want = reference(pbr, oracle, scene, w, h, frames, **variant)
    dev = pbr.Device(gpu_device)
    try:
        dev.pin_plan(DUAL)
        if lds_slots is not None:
            dev.set_knob("lds_slots", lds_slots)
        dev.upload_scene(desc)
        dev.configure(cfg)
        if dof:
            dev.render_dof(0, seeds, px, cam)
        else:
            dev.render(0, seeds, px, cam)
        assert dev.last_plan()[0] == pbr.Device.PLAN_NAMES[DUAL]
        assert_same_render(dev, want, "%s %d x %d x %d" % (scene[0], w, h, frames))
        return desc
    finally:
        dev.close()


@pytest.mark.parametrize("w,h,frames", [
    (8, 8, 1),        # 64 units: fewer than slots
    (8, 8, 3),        # lanes with one slot used and lanes with two
    (16, 8, 64),      # refill through nextSlot
])
def test_few_units_mixed_slots_and_refill_bit_exact(pbr, oracle, gpu_device, w, h, frames):
    desc = check(pbr, oracle, gpu_device, MID, w, h, frames)
    assert desc.num_nodes > STAGED          # cold and resident lanes both


def test_no_cold_lane_bit_exact(pbr, oracle, gpu_device):
    desc = check(pbr, oracle, gpu_device, CORNELL, 64, 64, 3)
    assert desc.num_nodes <= STAGED         # the tree fits LDS whole: the global loads issue with an empty EXEC


def test_no_resident_lane_bit_exact(pbr, oracle, gpu_device):
    check(pbr, oracle, gpu_device, MID, 64, 64, 3, lds_slots=0)


@pytest.mark.parametrize("brdf", [0, 1])
@pytest.mark.parametrize("lights,shadow", [(False, False), (True, False), (True, True)])
def test_all_six_variants_bit_exact(pbr, oracle, gpu_device, lights, shadow, brdf):
    check(pbr, oracle, gpu_device, CORNELL, 64, 64, 4, brdf=brdf, lights=lights, shadow=shadow)


def test_chained_flavour_bit_exact(pbr, oracle, gpu_device):
    check(pbr, oracle, gpu_device, CORNELL, 64, 64, 4, dof=True, focus=(32, 32))


# ---- hand-made trees ----------------------------------------------------------------------------------------------------

def only_leaves_of(pbr, faces_per_leaf, leaves=33):
    """A balanced tree whose every leaf has `faces_per_leaf` faces, as hand_scenes.make builds a scene under a named tree."""
    def balanced(n):
        return faces_per_leaf if n == 1 else [balanced(n - n // 2), balanced(n // 2)]
    spec = hand_scenes._linked(hand_scenes._sized(balanced(leaves)))
    assert all(arg == faces_per_leaf for kind, arg in spec if kind == "l")
    bvh, faces = hand_scenes.nodes_of(spec)
    facesV, facesN, vertices, normals, flat = hand_scenes.geometry(faces, hand_scenes.SEED)
    arrays = {"bvh": refit_ref.refit(bvh, facesV, vertices), "facesV": facesV, "facesN": facesN, "vertices": vertices, "normals": normals,
              "materials": np.array(hand_scenes.MATERIALS[1], np.float32), "lights": np.zeros((0, 12), np.float32)}
    cfg = pbr.Config.from_buffer_copy(hand_scenes.scene(pbr, "leaf1").cfg)
    sc = refit_scenes.Scene(pbr, arrays, cfg, hand_scenes.camera(pbr, vertices, flat),
                            pbr.pixel_dimension(hand_scenes.WIDTH, hand_scenes.HEIGHT), pbr.frame_seeds(0, hand_scenes.FRAMES))
    return sc


_hand = {}


def hand_made(pbr, oracle, name):
    if name not in _hand:
        sc = only_leaves_of(pbr, int(name[4:])) if name.startswith("only") else hand_scenes.scene(pbr, name)
        ref = oracle.Renderer(sc.desc, sc.cfg, threads=8)
        image = ref.render(0, sc.seeds, sc.px, sc.cam)
        counters = dict(ref.counter_dict())
        assert counters["hits"] > 0
        _hand[name] = (sc, (image, np.array(ref.debug, copy=True), counters))
    return _hand[name]


@pytest.mark.parametrize("name", ["leaf1", "leaf2", "only1", "only2", "cut255"])
def test_hand_made_trees_bit_exact(pbr, oracle, gpu_device, name):
    """leaf1 / leaf2: every walk is one visit, of a leaf.  only1 / only2: 33 leaves of one face / of two faces each under a
    balanced tree; cut255: 128 two-face leaves."""
    sc, want = hand_made(pbr, oracle, name)
    if name == "cut255":
        assert all(arg == 2 for kind, arg in hand_scenes.tree(name) if kind == "l")
    dev = pbr.Device(gpu_device)
    try:
        dev.pin_plan(DUAL)
        dev.upload_scene(sc.desc)
        dev.configure(sc.cfg)
        dev.render(0, sc.seeds, sc.px, sc.cam)
        assert dev.last_plan()[0] == pbr.Device.PLAN_NAMES[DUAL]
        assert_same_render(dev, want, name)
        assert dev.guard_trips() == [0, 0, 0]
    finally:
        dev.close()


# ---- state across launches ------------------------------------------------------------------------------------------------

def test_nothing_held_over_a_launch_outlives_it(pbr, oracle, gpu_device):
    """Two renders in one context, then a second scene uploaded into the same context and a render: its bits come out."""
    _, _, desc, cfg, cam, px, seeds, want = reference(pbr, oracle, MID, 64, 64, 3)
    _, _, desc2, cfg2, cam2, px2, seeds2, want2 = reference(pbr, oracle, CORNELL, 64, 64, 3)
    assert not same_values(want[0], want2[0])
    dev = pbr.Device(gpu_device)
    try:
        dev.pin_plan(DUAL)
        dev.upload_scene(desc)
        dev.configure(cfg)
        for launch in range(2):
            dev.reset_accum()
            c0 = dev.counters()
            dev.render(0, seeds, px, cam)
            assert dev.last_plan()[0] == pbr.Device.PLAN_NAMES[DUAL]
            got = dev.read_output()
            assert same_values(got, want[0]), "launch %d: %s" % (launch, describe_mismatch(got, want[0]))
            assert same_values(dev.read_debug(), want[1]), launch
            c1 = dev.counters()
            assert {k: c1[k] - c0[k] for k in c1} == want[2], launch
        dev.upload_scene(desc2)
        dev.configure(cfg2)
        dev.reset_accum()
        c0 = dev.counters()
        dev.render(0, seeds2, px2, cam2)
        assert dev.last_plan()[0] == pbr.Device.PLAN_NAMES[DUAL]
        got = dev.read_output()
        assert same_values(got, want2[0]), "second scene: %s" % describe_mismatch(got, want2[0])
        assert same_values(dev.read_debug(), want2[1])
        c1 = dev.counters()
        assert {k: c1[k] - c0[k] for k in c1} == want2[2]
    finally:
        dev.close()
