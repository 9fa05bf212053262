"""The hand-scheduled node phases (pt_kernel.hpp nodePhaseAsm / nodePhaseAsmCompact, pt_dual.hpp nodePhaseDualPipe) request
the cold records of a visit first and the LDS-resident ones second.  The shapes at which that order can go wrong — a visit
whose lanes are all cold, all resident, both or neither; a phase that ends on its first or on its last possible visit; a
lane whose two walks are both empty — against the CPU oracle, bit for bit: image, debug image and the four counters.
Small generated scenes at 64 x 64, three frames in one pbr_render; one oracle render per scene, shared by its cases."""
import numpy as np
import pytest

from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = 3
WHOLE_TREE = 1 << 20        # knob lds_slots: a cap, so anything above the tree's size stages all of it
PLANS = (0, 1, 2, 3, 4, 5, 6)
MOST_OF_MID = 1700

# name -> (kind, seed, triangles, configuration keys, traversal, lights + shadow rays, every ray misses)
SCENES = {
    # 35 records: resident as a whole in every plan
    "cornell": ("cornell", 1, 0, {"render.max_depth": 3}, 0, False, False),
    # 2012 records: more than the 1016 the two-paths kernel stages, resident as a whole in the other plans; with the knob
    # at MOST_OF_MID a few hundred more than the staged prefix in every plan
    "mid": ("hairball", 3, 2400, {"render.max_depth": 3}, 0, False, False),
    # 6729 records: more than any plan stages
    "large": ("sponza", 4, 6000, {"render.max_depth": 3}, 0, False, False),
    "mid_brdf0": ("hairball", 3, 2400, {"render.max_depth": 3, "render.brdf": 0}, 0, False, False),
    "lit_brdf1": ("cornell", 1, 0, {"render.max_depth": 3, "render.brdf": 1}, 0, True, False),
    "lit_brdf0": ("cornell", 1, 0, {"render.max_depth": 3, "render.brdf": 0}, 0, True, False),
    "mid_ordered": ("hairball", 3, 2400, {"render.max_depth": 3}, 2, False, False),
    "mid_compact": ("hairball", 3, 2400, {"render.max_depth": 3}, 3, False, False),
    "large_compact": ("sponza", 4, 6000, {"render.max_depth": 3}, 3, False, False),
    "mid_all_miss": ("hairball", 3, 2400, {"render.max_depth": 3}, 0, False, True),
}

_references = {}


def reference(pbr, oracle, name):
    """The scene, what a render of it needs, and the oracle's image, debug image and counters — computed once."""
    if name in _references:
        return _references[name]
    kind, seed, triangles, keys, traversal, lit, miss = SCENES[name]
    pbr.cfg_reset()
    pbr.cfg_set(**keys)
    sc = pbr.HostScene.generate(kind, seed, triangles)
    cfg, cam, px = sc.config(W, H), sc.camera(), pbr.pixel_dimension(W, H)
    cfg.traversal = traversal
    desc, lights = sc.desc, None
    if lit:
        # an orb light and a point light; shadow rays walk the tree with the any-hit node phase
        lights = np.zeros((2, 12), np.float32)
        lights[0] = [0.1, 1.6, 0.2, 0, 4.0, 3.5, 3.0, 0, 2, 0.12, 0, 0]
        lights[1] = [-0.5, 0.4, 0.6, 0, 1, 1, 1, 0, 1, 0, 0, 0]
        desc = pbr.SceneDesc.from_buffer_copy(sc.desc)
        desc.lights, desc.num_lights = lights.ctypes.data, 2
        cfg.shadow_rays = 1
    if miss:
        # the eye far behind the scene, looking on along the same axis: no ray meets a box
        cam.eye.x += 1000.0 * cam.w.x
        cam.eye.y += 1000.0 * cam.w.y
        cam.eye.z += 1000.0 * cam.w.z
    seeds = pbr.frame_seeds(0, FRAMES)
    ref = oracle.Renderer(desc, cfg, threads=8)
    image = ref.render(0, seeds, px, cam)
    image.setflags(write=False)
    debug = np.array(ref.debug, copy=True)
    debug.setflags(write=False)
    counters = dict(ref.counter_dict())
    if miss:
        assert counters["hits"] == 0 and counters["tris"] == 0
    else:
        assert counters["hits"] > 0
    _references[name] = (sc, desc, lights, cfg, cam, px, seeds, image, debug, counters)
    return _references[name]


def check(pbr, oracle, gpu_device, name, plan, lds_slots=None, ph_park=None):
    sc, desc, lights, cfg, cam, px, seeds, image, debug, counters = reference(pbr, oracle, name)
    dev = pbr.Device(gpu_device)
    try:
        dev.pin_plan(plan)
        if lds_slots is not None:
            dev.set_knob("lds_slots", lds_slots)
        if ph_park is not None:
            dev.set_knob("ph_park", ph_park)
        dev.upload_scene(desc)
        dev.configure(cfg)
        dev.render(0, seeds, px, cam)
        assert dev.last_plan()[0] == pbr.Device.PLAN_NAMES[plan]
        got = dev.read_output()
        assert same_values(got, image), describe_mismatch(got, image)
        assert same_values(dev.read_debug(), debug)
        assert dev.counters() == counters
    finally:
        dev.close()


def test_the_scenes_have_the_sizes_the_cases_rely_on(pbr, oracle):
    assert reference(pbr, oracle, "cornell")[1].num_nodes < 64
    assert MOST_OF_MID + 200 <= reference(pbr, oracle, "mid")[1].num_nodes <= MOST_OF_MID + 500
    assert reference(pbr, oracle, "large")[1].num_nodes > 5200           # a block's share of LDS holds at most 5112 records


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name,lds_slots", [
    ("cornell", 0), ("cornell", WHOLE_TREE),                 # every visit all cold / all resident
    ("mid", 0), ("mid", 8), ("mid", MOST_OF_MID), ("mid", None),                   # visits with both kinds, one kind, neither
    ("large", 8), ("large", None),
])
def test_cold_and_resident_mixes_bit_exact(pbr, oracle, gpu_device, name, lds_slots, plan):
    check(pbr, oracle, gpu_device, name, plan, lds_slots)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("lds_slots", [0, 8, None])
def test_brdf_0_bit_exact(pbr, oracle, gpu_device, lds_slots, plan):
    check(pbr, oracle, gpu_device, "mid_brdf0", plan, lds_slots)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("lds_slots", [0, 4, None])
@pytest.mark.parametrize("name", ["lit_brdf1", "lit_brdf0"])
def test_two_lights_and_shadow_rays_bit_exact(pbr, oracle, gpu_device, name, lds_slots, plan):
    check(pbr, oracle, gpu_device, name, plan, lds_slots)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("lds_slots", [0, 8, None])
def test_ordered_walk_bit_exact(pbr, oracle, gpu_device, lds_slots, plan):
    check(pbr, oracle, gpu_device, "mid_ordered", plan, lds_slots)


@pytest.mark.parametrize("plan", PLANS[:6])                  # (compact records have no two-paths kernel)
@pytest.mark.parametrize("name,lds_slots", [("mid_compact", 0), ("mid_compact", 8), ("mid_compact", None), ("large_compact", None)])
def test_compact_record_walk_bit_exact(pbr, oracle, gpu_device, name, lds_slots, plan):
    check(pbr, oracle, gpu_device, name, plan, lds_slots)


@pytest.mark.parametrize("plan", [2, 4, 6])
@pytest.mark.parametrize("ph_park", [1, 128])                # a phase ends on its first / on its last possible visit
@pytest.mark.parametrize("lds_slots", [8, None])
def test_phase_length_extremes_bit_exact(pbr, oracle, gpu_device, lds_slots, ph_park, plan):
    check(pbr, oracle, gpu_device, "mid", plan, lds_slots, ph_park)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("lds_slots", [0, None])
def test_every_ray_misses_bit_exact(pbr, oracle, gpu_device, lds_slots, plan):
    check(pbr, oracle, gpu_device, "mid_all_miss", plan, lds_slots)
