"""pbr_render_dof: the frames of a render WITH a focus point in one call.  What a frame reads of its predecessor — the
first-hit distance of its own pixel and of the focus pixel — is walked ahead of the launch by the focus chain
(csrc/pt_chain.hpp); the frames then run through pbr_render's frame-parallel launch.  The contract is pbr_render's:
bit-identical to n x { pbr_render_frame ; pbr_accumulate }, .w included — so every comparison here is `same_values`
(tolerance 0) against the CPU oracle's frame-by-frame render and against the device's own per-frame sequence; counters
and debug image equal to the oracle's show that the pre-pass's walks are not counted."""
import os
from importlib import import_module

import numpy as np
import pytest

from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

PLANS = ["refill-lean", "refill-wide", "phased-lean", "phased-wide", "phased-mid", "refill-mid", "phased-dual"]


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def make_scene(pbr, kind="cornell", seed=1, triangles=0, **cfg):
    pbr.cfg_reset()
    pbr.cfg_set(**cfg)
    return pbr.HostScene.generate(kind, seed, triangles)


def lit_desc(pbr, sc):
    """The scene with one orb light above the Cornell box's hole and one point light (as tests/test_gpu_parity.py has it)."""
    lights = np.zeros((2, 12), np.float32)
    lights[0] = [0.1, 1.6, 0.2, 0, 4.0, 3.5, 3.0, 0, 2, 0.12, 0, 0]
    lights[1] = [-0.5, 0.4, 0.6, 0, 1, 1, 1, 0, 1, 0, 0, 0]
    desc = pbr.SceneDesc.from_buffer_copy(sc.desc)
    desc.lights, desc.num_lights = lights.ctypes.data, 2
    return desc, lights


def focused(pbr, cam, x, y):
    cam = pbr.Camera.from_buffer_copy(cam)
    cam.focusPoint[0], cam.focusPoint[1] = x, y
    return cam


def per_frame(dev, seeds, px, cam, first=0):
    """The sequence pbr_render_dof replaces: render_frame + accumulate per frame; the result as imageOut."""
    for k, seed in enumerate(seeds):
        n = first + k
        dev.render_frame(float(seed), float(np.float32(n) / np.float32(n + 1)), px, cam)
        dev.accumulate()
    dev.accumulate()
    return dev.read_output()


def check_against_oracle(pbr, oracle, dev, desc, cfg, cam, px, frames, what=""):
    seeds = pbr.frame_seeds(0, frames)
    ref = oracle.Renderer(desc, cfg, threads=8)
    want = ref.render(0, seeds, px, cam)
    dev.upload_scene(desc)
    dev.configure(cfg)
    dev.render_dof(0, seeds, px, cam)
    got = dev.read_output()
    assert same_values(got, want), "%s: %s" % (what, describe_mismatch(got, want))
    assert dev.counters() == ref.counter_dict(), what
    assert same_values(dev.read_debug(), ref.debug), what
    return got, ref


@pytest.mark.parametrize("frames", [4, 9])
def test_render_dof_is_the_frame_by_frame_sequence(pbr, oracle, device, frames):
    sc = make_scene(pbr, **{"render.max_depth": 4})
    w, h = 64, 64
    cfg, px = sc.config(w, h), pbr.pixel_dimension(w, h)
    cam = focused(pbr, sc.camera(), 20, 30)
    got, ref = check_against_oracle(pbr, oracle, device, sc.desc, cfg, cam, px, frames)
    plain = oracle.Renderer(sc.desc, cfg, threads=8).render(0, pbr.frame_seeds(0, frames), px, sc.camera())
    assert not same_values(plain, ref.image)                       # the lens did something
    assert device.last_focus_chain_ms() > 0.0
    device.reset_accum()
    own = per_frame(device, pbr.frame_seeds(0, frames), px, cam)
    assert same_values(got, own), describe_mismatch(got, own)


def test_render_dof_continues(pbr, oracle, device):
    """Two calls of 4 and 5 frames == one of 9: the second call's chain starts at imageIn.w, which the first call left."""
    sc = make_scene(pbr, **{"render.max_depth": 4})
    w, h = 64, 64
    cfg, px, seeds = sc.config(w, h), pbr.pixel_dimension(w, h), pbr.frame_seeds(0, 9)
    cam = focused(pbr, sc.camera(), 20, 30)
    want = oracle.Renderer(sc.desc, cfg, threads=8).render(0, seeds, px, cam)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.render_dof(0, seeds[:4], px, cam)
    device.render_dof(4, seeds[4:], px, cam)
    got = device.read_output()
    assert same_values(got, want), describe_mismatch(got, want)


@pytest.mark.parametrize("case", ["schlick", "samples2", "shadow-orb", "outside", "miss"])
def test_render_dof_variants(pbr, oracle, device, case):
    """Both BRDFs, two samples per frame (the second sample's camera ray reads the same two distances), shadow rays with an
    orb light (traverse with LIGHTS in the chain), a focus point outside the image (clamped to the edge) and one on a pixel
    whose camera ray misses everything (t = inf, taken as 1000)."""
    keys = {"render.max_depth": 4}
    if case == "schlick":
        keys["render.brdf"] = 0
    if case == "samples2":
        keys["render.samples"] = 2
    w, h = 64, 64
    focus = (20, 30)
    if case == "miss":
        sc = make_scene(pbr, "sponza", 4, 3000, **keys)
    else:
        sc = make_scene(pbr, **keys)
    cfg, px = sc.config(w, h), pbr.pixel_dimension(w, h)
    desc, keep = sc.desc, None
    if case == "shadow-orb":
        desc, keep = lit_desc(pbr, sc)
        cfg.shadow_rays = 1
    if case == "outside":
        focus = (w + 9, h + 3)
    if case == "miss":
        first = oracle.Renderer(desc, cfg, threads=8).render(0, pbr.frame_seeds(0, 1), px, sc.camera())
        missed = np.argwhere(np.isinf(first[..., 3]))
        assert len(missed) > 0, "this scene has no camera ray that misses: the case needs another scene"
        focus = (int(missed[0][1]), int(missed[0][0]))
    cam = focused(pbr, sc.camera(), *focus)
    got, ref = check_against_oracle(pbr, oracle, device, desc, cfg, cam, px, 5, case)
    plain = oracle.Renderer(desc, cfg, threads=8).render(0, pbr.frame_seeds(0, 5), px, sc.camera())
    assert not same_values(plain, ref.image), case


@pytest.mark.parametrize("plan", range(7))
def test_render_dof_in_every_plan(pbr, oracle, device, plan):
    sc = make_scene(pbr, **{"render.max_depth": 4})
    w, h = 64, 64
    cfg, px = sc.config(w, h), pbr.pixel_dimension(w, h)
    device.pin_plan(plan)
    check_against_oracle(pbr, oracle, device, sc.desc, cfg, focused(pbr, sc.camera(), 20, 30), px, 5, PLANS[plan])


@pytest.mark.parametrize("traversal", [1, 2, 3])
def test_render_dof_in_the_ray_ordered_walks(pbr, oracle, device, traversal):
    sc = make_scene(pbr, "sponza", 4, 6000, **{"render.max_depth": 3})
    w, h = 64, 48
    cfg, px = sc.config(w, h), pbr.pixel_dimension(w, h)
    cfg.traversal = traversal
    check_against_oracle(pbr, oracle, device, sc.desc, cfg, focused(pbr, sc.camera(), 30, 20), px, 4, "traversal %d" % traversal)


@pytest.mark.parametrize("traversal", [0, 2])
def test_render_dof_in_native_arithmetic(pbr, device, traversal):
    """arith = native has no oracle image to be bit-identical to; all plans of the mode render the same bits, so the
    yardstick is the device's own per-frame sequence — in three plans."""
    sc = make_scene(pbr, **{"render.max_depth": 4})
    w, h = 64, 64
    cfg, px, seeds = sc.config(w, h), pbr.pixel_dimension(w, h), pbr.frame_seeds(0, 5)
    cfg.arith, cfg.traversal = 1, traversal
    cam = focused(pbr, sc.camera(), 20, 30)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    want = per_frame(device, seeds, px, cam)
    for plan in (0, 4, 6):
        device.pin_plan(plan)
        device.reset_accum()
        device.render_dof(0, seeds, px, cam)
        got = device.read_output()
        assert same_values(got, want), "%s: %s" % (PLANS[plan], describe_mismatch(got, want))


def test_render_dof_across_tile_shards(pbr, oracle, gpu_device):
    """tile_world = 3: ONE set_focus_depth per call, every rank walks the focus pixel's chain itself."""
    sc = make_scene(pbr, **{"render.max_depth": 3})
    w, h, world = 64, 48, 3
    cfg, px, seeds = sc.config(w, h), pbr.pixel_dimension(w, h), pbr.frame_seeds(0, 6)
    cam = focused(pbr, sc.camera(), 37, 22)
    ref = oracle.Renderer(sc.desc, cfg, threads=8)
    ranks = []
    try:
        for r in range(world):
            dev = pbr.Device(gpu_device)
            c = pbr.Config.from_buffer_copy(cfg)
            c.tile_world, c.tile_rank = world, r
            dev.upload_scene(sc.desc)
            dev.configure(c)
            ranks.append(dev)
        with pytest.raises(pbr.PbrError, match="pbr_set_focus_depth"):
            ranks[0].render_dof(0, seeds[:4], px, cam)
        for first, part in ((0, seeds[:4]), (4, seeds[4:])):
            owners = [dev.get_focus_depth(37, 22) for dev in ranks]
            assert sum(owned for _, owned in owners) == 1
            depth = [t for t, owned in owners if owned][0]          # the "broadcast": once per call
            got = np.zeros((h, w, 4), np.float32)
            for dev in ranks:
                dev.set_focus_depth(depth)
                dev.render_dof(first, part, px, cam)
                got += dev.read_output()                              # other ranks' tiles read 0
            want = ref.render(first, part, px, cam)
            assert same_values(got, want), "from frame %d: %s" % (first, describe_mismatch(got, want))
        with pytest.raises(pbr.PbrError, match="pbr_set_focus_depth"):   # the value was consumed by the call
            ranks[1].render_dof(6, seeds[:2], px, cam)
    finally:
        for dev in ranks:
            dev.close()


def test_render_dof_chunked(pbr, oracle, device):
    """chunk_frames = 3: nine frames as three launch pairs, each behind its own chain; the chain crosses the boundary
    through imageIn.w (and, for the focus pixel, through the chain's own last value)."""
    sc = make_scene(pbr, **{"render.max_depth": 4})
    w, h = 64, 64
    cfg, px, seeds = sc.config(w, h), pbr.pixel_dimension(w, h), pbr.frame_seeds(0, 9)
    cam = focused(pbr, sc.camera(), 20, 30)
    device.pin_plan(4)
    got, ref = check_against_oracle(pbr, oracle, device, sc.desc, cfg, cam, px, 9, "unchunked")
    assert device.last_trace()[1] == 1
    device.set_knob("chunk_frames", 3)
    device.reset_accum()
    device.render_dof(0, seeds, px, cam)
    assert device.last_trace()[1] == 3
    chunked = device.read_output()
    assert same_values(chunked, got), describe_mismatch(chunked, got)
    assert device.counters() == ref.counter_dict()


@pytest.mark.parametrize("layout", [0, 1])
def test_render_dof_in_both_table_layouts(pbr, oracle, device, layout):
    sc = make_scene(pbr, **{"render.max_depth": 4})
    w, h = 64, 64
    cfg, px = sc.config(w, h), pbr.pixel_dimension(w, h)
    device.set_knob("chain_layout", layout)
    check_against_oracle(pbr, oracle, device, sc.desc, cfg, focused(pbr, sc.camera(), 20, 30), px, 5, "layout %d" % layout)


def test_render_keeps_refusing_and_render_dof_without_focus_is_render(pbr, device):
    sc = make_scene(pbr, **{"render.max_depth": 4})
    w, h = 64, 64
    cfg, cam, px, seeds = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h), pbr.frame_seeds(0, 4)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    with pytest.raises(pbr.PbrError, match="pbr_render needs focusPoint < 0"):
        device.render(0, seeds, px, focused(pbr, cam, 20, 30))
    device.render(0, seeds, px, cam)
    want, counted = device.read_output(), device.counters()
    device.reset_accum()
    device.render_dof(0, seeds, px, cam)
    got = device.read_output()
    assert same_values(got, want), describe_mismatch(got, want)
    assert device.counters() == counted
    assert device.last_focus_chain_ms() == 0.0


def test_render_dof_refuses_phong_tessellation(pbr, device, tmp_path):
    """The Phong-tessellation plan has an intersection of its own, which the chain does not walk: refused, and the message
    names the per-frame sequence that renders it."""
    from test_gpu_parity import smooth_scene
    sc = smooth_scene(pbr, tmp_path, **{"render.max_depth": 3, "render.brdf": 1, "render.phong_tessellation": 0.6})
    w, h = 32, 32
    cfg, cam, px = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    with pytest.raises(pbr.PbrError, match="pbr_render_frame"):
        device.render_dof(0, pbr.frame_seeds(0, 2), px, focused(pbr, cam, 10, 10))


def test_render_dof_at_full_size(pbr, oracle, device):
    """BASELINE configs[3] (Sponza-class, 1920 x 1080), 8 frames with the focus point at the image centre: a 16-row band
    against the oracle (the band holds the focus pixel: the oracle needs no other row), the whole frame against the
    device's per-frame sequence."""
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 3})
    sc = pbr.HostScene.generate("sponza", 2, 260000)
    w, h, frames = 1920, 1080, 8
    cfg, px, seeds = sc.config(w, h), pbr.pixel_dimension(w, h), pbr.frame_seeds(0, frames)
    cam = focused(pbr, sc.camera(), w // 2, h // 2)
    rows = (h // 2 - 8, h // 2 + 8)
    band = slice(rows[0], rows[1])
    ref = oracle.Renderer(sc.desc, cfg, threads=os.cpu_count() or 8)
    for k, seed in enumerate(seeds):
        out = ref.render_frame(float(seed), float(np.float32(k) / np.float32(k + 1)), px, cam, rows=rows)
        ref.image[band] = out[band]
    assert np.isfinite(ref.image[band][..., 3]).any()
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.render_dof(0, seeds, px, cam)
    got = device.read_output()
    assert same_values(got[band], ref.image[band]), describe_mismatch(got[band], ref.image[band])
    device.reset_accum()
    own = per_frame(device, seeds, px, cam)
    assert same_values(got, own), describe_mismatch(got, own)


def test_multi_render_with_a_focus_point(pbr, gpu_device):
    """The multi driver: ONE MultiDevice.render call with a focus point on 3 contexts == the single context's per-frame
    sequence (one focus hand-over for the whole call)."""
    multi = import_module(pbr.__name__ + ".multi")
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4})
    sc = pbr.HostScene.generate("cornell", 0, 0)
    w, h, frames = 96, 64, 5
    cfg, px, seeds = sc.config(w, h), pbr.pixel_dimension(w, h), pbr.frame_seeds(0, frames)
    cam = focused(pbr, sc.camera(), 40, 30)
    cam.lense[0], cam.lense[1] = 0.05, 1.8
    dev = pbr.Device(gpu_device)
    try:
        dev.upload_scene(sc.desc)
        dev.configure(cfg)
        for k in range(frames):
            dev.render_frame(float(seeds[k]), k / (k + 1.0), px, cam)
            dev.accumulate()
        dev.accumulate()
        want = dev.read_output()
    finally:
        dev.close()
    m = multi.MultiDevice([gpu_device] * 3, multi.PEER_COPY)
    try:
        m.upload_scene(sc.desc)
        m.configure(cfg)
        m.render(0, seeds, px, cam)
        got = m.read_full(1)
        assert same_values(got, want), describe_mismatch(got, want)
    finally:
        m.close()
