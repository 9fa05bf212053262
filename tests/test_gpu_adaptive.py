"""pbr_render_adaptive: rounds of frames over the 8x8 tiles that have not converged (csrc/pt_adaptive.hpp,
pt_adaptive_host.hpp).  The contract is exact: a tile that stopped after c frames holds, .w included, what
pbr_render( first_count, c, seeds[:c] ) holds there, and the error estimate that stops it is a fixed binary32 algorithm —
so every comparison here is `same_values` (tolerance 0): the device's frames-per-tile map and error estimates against
tests/adaptive_ref.py fed with the CPU oracle's per-frame colours, every tile of the image against the oracle's prefix image
of that tile's count.

The mixed cases (MIXED, 128 x 96 = 192 tiles, min_frames 4, round_frames 4, max_frames 20: tests after 4, 8, 12, 16, 20
frames) have their thresholds chosen on the CPU, from the oracle and the restatement alone, such that tiles stop in at
least three distinct rounds, >= 10 % of the tiles stop at min_frames and >= 10 % reach max_frames; `check_mixed` asserts
that of the reference side before it looks at the device.  Chosen thresholds and the restatement's histograms
{frames: tiles}:
    cornell-schlick  (Cornell box, BRDF 0)                          0.125  {4: 26, 8: 10, 12: 12, 16: 1, 20: 143}
    cornell-sa       (Cornell box, BRDF 1)                          0.2    {4: 32, 8: 9, 12: 14, 16: 20, 20: 117}
    sky              (Cornell box from ( 0.9, 1, 6.5 ): 150 of the  0.1    {4: 157, 8: 4, 12: 2, 16: 2, 20: 27}
                      192 tiles show only the sky, BRDF 1)
"""
import ctypes

import numpy as np
import pytest

import adaptive_ref
from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

PLANS = ["refill-lean", "refill-wide", "phased-lean", "phased-wide", "phased-mid", "refill-mid", "phased-dual"]
W, H = 128, 96
MIN, ROUND, MAX = 4, 4, 20
MIXED = {"cornell-schlick": (0, 0.125, False), "cornell-sa": (1, 0.2, False), "sky": (1, 0.1, True)}   # BRDF, threshold, far camera


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def mixed_scene(pbr, case, w=W, h=H, **more):
    brdf, threshold, far = MIXED[case]
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4, "render.brdf": brdf})
    sc = pbr.HostScene.generate("cornell", 1, 0)
    cfg, cam, px = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h)
    for key, value in more.items():
        setattr(cfg, key, value)
    if far:
        cam.eye.x, cam.eye.z = 0.9, 6.5          # the box in the middle of the frame, the sky around it
    return sc, cfg, cam, px, threshold


class Reference:
    """The oracle stepped frame by frame: prefix[c] = the image after c frames, colours[k] = frame k's finalColor (a frame
    rendered onto a zero image with weight 0 is fc + ( 0 - fc ) * 0 = fc), debug[k] = frame k's debug image."""

    def __init__(self, pbr, oracle, desc, cfg, cam, px, frames, first=0):
        acc, single = oracle.Renderer(desc, cfg, threads=16), oracle.Renderer(desc, cfg, threads=16)
        self.pbr, self.w, self.h = pbr, int(cfg.width), int(cfg.height)
        self.prefix, self.colours, self.debug = {0: acc.image.copy()}, [], []
        self.samples = int(cfg.samples)
        for k, seed in enumerate(pbr.frame_seeds(first, frames)):
            n = first + k
            acc.image = acc.render_frame(float(seed), float(np.float32(n) / np.float32(n + 1)), px, cam)
            self.prefix[k + 1] = acc.image.copy()
            self.colours.append(pbr.tiles.to_tile_major(single.render_frame(float(seed), 0.0, px, cam)))
            self.debug.append(single.debug.copy())
        self.colours = np.stack(self.colours)

    def decide(self, min_frames, round_frames, max_frames, threshold):
        frames, error, rounds = adaptive_ref.run(self.colours, min_frames, round_frames, max_frames, threshold)
        shape = (self.h // 8, self.w // 8)
        return frames.reshape(shape), error.reshape(shape), rounds

    def per_pixel(self, tile_map):
        return np.kron(tile_map, np.ones((8, 8), tile_map.dtype))

    def compose(self, frames, images):
        """The image whose every tile is images[c] there, c = the tile's frame count."""
        count = self.per_pixel(frames)
        out = np.zeros((self.h, self.w, 4), np.float32)
        for c in np.unique(frames):
            out[count == c] = images[int(c)][count == c]
        return out

    def counted(self, frames):
        """nodes / tris / paths of exactly the units a frames map says were traced (the debug image holds a unit's node and
        face-test counts / 1265 and / 1082: exact integers below 2^23 come back by rounding)."""
        count = self.per_pixel(frames)
        nodes = tris = 0
        for k, dbg in enumerate(self.debug):
            traced = count > k
            nodes += int(np.rint(dbg[..., 1][traced].astype(np.float64) * 1265.0).sum())
            tris += int(np.rint(dbg[..., 0][traced].astype(np.float64) * 1082.0).sum())
        return {"nodes": nodes, "tris": tris, "paths": int(count.sum()) * self.samples}


def histogram(frames):
    return {int(c): int(n) for c, n in zip(*np.unique(frames, return_counts=True))}


def assert_mixed(frames, what):
    """The condition on the INPUTS of a mixed case, asserted of the restatement's map: it decides something."""
    hist, tiles = histogram(frames), frames.size
    assert len(hist) >= 3, "%s: tiles stop in %d distinct rounds only: %r" % (what, len(hist), hist)
    assert hist.get(MIN, 0) * 10 >= tiles, "%s: fewer than 10 %% of the tiles stop at min_frames: %r" % (what, hist)
    assert hist.get(MAX, 0) * 10 >= tiles, "%s: fewer than 10 %% of the tiles reach max_frames: %r" % (what, hist)


def render_adaptive(pbr, dev, px, cam, threshold, first=0, lo=MIN, step=ROUND, hi=MAX):
    dev.render_adaptive(first, pbr.frame_seeds(first, hi), px, cam, lo, step, hi, threshold)
    return dev.read_output(), dev.tile_stats()


def check_against(ref, dev, got, stats, want_frames, want_error, what):
    frames, error = stats
    print("%s: device %r reference %r" % (what, histogram(frames), histogram(want_frames)))
    assert np.array_equal(frames, want_frames), "%s: frames per tile differ at %r" % (what, np.argwhere(frames != want_frames)[:8].tolist())
    assert same_values(error, want_error), "%s: error estimates: %s" % (what, describe_mismatch(error, want_error))
    want = ref.compose(want_frames, ref.prefix)
    assert same_values(got, want), "%s: image: %s" % (what, describe_mismatch(got, want))
    want_debug = ref.compose(want_frames, {c: ref.debug[c - 1] for c in np.unique(want_frames)})
    assert same_values(dev.read_debug(), want_debug), "%s: debug image" % what
    counted, expected = dev.counters(), ref.counted(want_frames)
    assert {k: counted[k] for k in expected} == expected, what
    rounds, units, fold_ms = dev.last_adaptive()
    assert units == 64 * int(want_frames.astype(np.uint64).sum()), what
    return rounds


def check_mixed(pbr, oracle, dev, case, what="", knobs=(), **cfg_more):
    sc, cfg, cam, px, threshold = mixed_scene(pbr, case, **cfg_more)
    ref = Reference(pbr, oracle, sc.desc, cfg, cam, px, MAX)
    want_frames, want_error, want_rounds = ref.decide(MIN, ROUND, MAX, threshold)
    assert_mixed(want_frames, case + what)
    dev.upload_scene(sc.desc)
    dev.configure(cfg)
    for name, value in knobs:
        dev.set_knob(name, value)
    got, stats = render_adaptive(pbr, dev, px, cam, threshold)
    rounds = check_against(ref, dev, got, stats, want_frames, want_error, case + what)
    assert rounds == want_rounds
    return ref, got, stats, want_frames


# ---- 1, 2: nothing to decide ---------------------------------------------------------------------------------------

def test_one_round_is_pbr_render(pbr, device):
    """min_frames = max_frames: image, .w, debug image and counters of pbr_render( max_frames ) on a fresh context."""
    sc, cfg, cam, px, _ = mixed_scene(pbr, "cornell-sa", 64, 64)
    seeds = pbr.frame_seeds(0, 6)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.render_adaptive(0, seeds, px, cam, 6, 4, 6, 0.05)
    got, dbg, counted = device.read_output(), device.read_debug(), device.counters()
    frames, error = device.tile_stats()
    assert (frames == 6).all() and frames.shape == (8, 8)
    assert device.last_adaptive()[:2] == (1, 64 * 64 * 6)
    fresh = pbr.Device(0)
    try:
        fresh.upload_scene(sc.desc)
        fresh.configure(cfg)
        fresh.render(0, seeds, px, cam)
        want = fresh.read_output()
        assert same_values(got, want), describe_mismatch(got, want)
        assert same_values(dbg, fresh.read_debug())
        assert counted == fresh.counters()
    finally:
        fresh.close()


def test_threshold_zero_stops_only_constant_tiles(pbr, oracle, device):
    """threshold = 0 through five rounds: the restatement says which tiles' frames are exactly constant (error == 0: the
    Cornell box's black and sky tiles); all others reach max_frames and hold pbr_render( max_frames ) there."""
    sc, cfg, cam, px, _ = mixed_scene(pbr, "sky")
    ref = Reference(pbr, oracle, sc.desc, cfg, cam, px, MAX)
    want_frames, want_error, want_rounds = ref.decide(MIN, ROUND, MAX, 0.0)
    assert set(histogram(want_frames)) == {MIN, MAX}
    assert ((want_frames == MIN) == (want_error == 0)).all()
    device.upload_scene(sc.desc)
    device.configure(cfg)
    got, stats = render_adaptive(pbr, device, px, cam, 0.0)
    assert check_against(ref, device, got, stats, want_frames, want_error, "threshold 0") == want_rounds == 5


def test_threshold_infinity_stops_everything_after_min_frames(pbr, device):
    sc, cfg, cam, px, _ = mixed_scene(pbr, "cornell-sa", 64, 64)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    got, (frames, error) = render_adaptive(pbr, device, px, cam, float("inf"))
    assert (frames == MIN).all()
    assert device.last_adaptive()[:2] == (1, 64 * 64 * MIN)
    counted = device.counters()
    device.reset_accum()
    device.render(0, pbr.frame_seeds(0, MIN), px, cam)
    want = device.read_output()
    assert same_values(got, want), describe_mismatch(got, want)
    assert counted == device.counters()


# ---- 3: mixed, against the oracle -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(MIXED))
def test_mixed_against_the_oracle(pbr, oracle, device, case):
    ref, got, (frames, error), want_frames = check_mixed(pbr, oracle, device, case)
    if case == "sky":
        sky = np.array(list(mixed_scene(pbr, case)[1].sky_light)[:3], np.float32)
        only_sky = (ref.colours[..., :3] == sky).all(axis=(0, 2, 3)).reshape(frames.shape)
        assert only_sky.sum() * 2 >= only_sky.size                      # part of the frame is sky: here most of it
        assert (frames[only_sky] == MIN).all() and (error[only_sky] == 0).all()


# ---- 4: every plan ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plan", range(7))
def test_in_every_plan(pbr, oracle, device, plan):
    device.pin_plan(plan)
    check_mixed(pbr, oracle, device, "cornell-sa", " in " + PLANS[plan])
    assert device.last_plan()[0] == PLANS[plan]


def test_phong_tessellation(pbr, oracle, device, tmp_path):
    """Phong tessellation is one more plan of the same queue: against the oracle in that configuration."""
    from test_gpu_parity import smooth_scene
    sc = smooth_scene(pbr, tmp_path, **{"render.max_depth": 3, "render.brdf": 1, "render.phong_tessellation": 0.6})
    w, h = 64, 64
    cfg, cam, px = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h)
    ref = Reference(pbr, oracle, sc.desc, cfg, cam, px, 12)
    want_frames, want_error, want_rounds = ref.decide(3, 3, 12, 0.15)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    got, stats = render_adaptive(pbr, device, px, cam, 0.15, lo=3, step=3, hi=12)
    assert check_against(ref, device, got, stats, want_frames, want_error, "phong") == want_rounds
    assert device.last_plan()[0] == "refill-lean-phong"


# ---- 5: every mode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("traversal", [1, 2, 3])
def test_in_the_ray_ordered_walks(pbr, oracle, device, traversal):
    check_mixed(pbr, oracle, device, "cornell-sa", " traversal %d" % traversal, traversal=traversal)


@pytest.mark.parametrize("traversal", [0, 2])
def test_in_native_arithmetic(pbr, device, traversal):
    """arith = native has no oracle bits: the frames map against the restatement fed with the DEVICE's per-frame renders,
    the image against the same device's pbr_render( c ) per distinct count c."""
    sc, cfg, cam, px, threshold = mixed_scene(pbr, "cornell-sa", arith=1, traversal=traversal)
    seeds = pbr.frame_seeds(0, MAX)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    colours = []
    for seed in seeds:
        device.reset_accum()
        device.render_frame(float(seed), 0.0, px, cam)
        colours.append(pbr.tiles.to_tile_major(device.read_output()))
    want_frames, want_error, want_rounds = adaptive_ref.run(np.stack(colours), MIN, ROUND, MAX, threshold)
    want_frames, want_error = want_frames.reshape(H // 8, W // 8), want_error.reshape(H // 8, W // 8)
    assert_mixed(want_frames, "native")
    device.reset_accum()
    got, (frames, error) = render_adaptive(pbr, device, px, cam, threshold)
    assert np.array_equal(frames, want_frames)
    assert same_values(error, want_error), describe_mismatch(error, want_error)
    count = np.kron(frames, np.ones((8, 8), frames.dtype))
    for c in np.unique(frames):
        device.reset_accum()
        device.render(0, seeds[:int(c)], px, cam)
        want = device.read_output()
        assert same_values(got[count == c], want[count == c]), "%d frames: %s" % (c, describe_mismatch(got[count == c], want[count == c]))


# ---- 6: chunking -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [1, 3])
def test_chunked_rounds(pbr, oracle, device, chunk):
    """chunk_frames = 1 / 3: every round of 4 frames is 4 / 2 launch pairs, tested only behind its last."""
    check_mixed(pbr, oracle, device, "cornell-sa", " chunk %d" % chunk, knobs=(("chunk_frames", chunk),))
    per_round = (4 + chunk - 1) // chunk
    assert device.last_trace()[1] == 5 * per_round


# ---- 7: shards -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
def test_tile_shards(pbr, oracle, gpu_device, world):
    import torch
    sc, cfg, cam, px, threshold = mixed_scene(pbr, "cornell-sa")
    ref = Reference(pbr, oracle, sc.desc, cfg, cam, px, MAX)
    want_frames, want_error, _ = ref.decide(MIN, ROUND, MAX, threshold)
    want = ref.compose(want_frames, ref.prefix)
    gathered, ranks = None, []
    try:
        for rank in range(world):
            dev = pbr.Device(gpu_device)
            ranks.append(dev)
            c = pbr.Config.from_buffer_copy(cfg)
            c.tile_world, c.tile_rank = world, rank
            dev.upload_scene(sc.desc)
            dev.configure(c)
            part, (frames, error, ids) = render_adaptive(pbr, dev, px, cam, threshold)
            assert np.array_equal(ids, pbr.tiles.local_tile_ids(W, H, world, rank))
            assert np.array_equal(frames, want_frames.reshape(-1)[ids]), "rank %d" % rank
            assert same_values(error, want_error.reshape(-1)[ids]), "rank %d" % rank
            mask = pbr.tiles.rows_of_rank(W, H, world, rank)
            assert same_values(part[mask], want[mask]) and not part[~mask].any(), "rank %d" % rank
            assert dev.last_adaptive()[1] == 64 * int(frames.astype(np.uint64).sum())
            if gathered is None:
                gathered = torch.zeros(world * dev.tile_bytes() // 4, dtype=torch.float32, device="cuda")
            dev.export_tiles(gathered.data_ptr() + rank * dev.tile_bytes())
        torch.cuda.synchronize()
        ranks[0].import_tiles(gathered.data_ptr())
        full = ranks[0].read_full()
        assert same_values(full, want), describe_mismatch(full, want)
    finally:
        for dev in ranks:
            dev.close()


# ---- 8: the neighbours are untouched ---------------------------------------------------------------------------------

def test_the_renders_around_it_are_untouched(pbr, oracle, gpu_device):
    """pbr_render -> pbr_render_adaptive -> pbr_reset_accum -> pbr_render: the second render and what pbr_diag_last_plan /
    pbr_diag_last_deal report of it are those of a context that never rendered adaptively (tuner, tile costs and dealing
    tables as they were); a pbr_render_frame right behind an adaptive call deals all tiles."""
    sc, cfg, cam, px, threshold = mixed_scene(pbr, "cornell-sa")
    seeds = pbr.frame_seeds(0, 8)
    told = []
    for adaptive in (False, True):
        dev = pbr.Device(gpu_device)
        try:
            dev.upload_scene(sc.desc)
            dev.configure(cfg)
            dev.render(0, seeds, px, cam)
            first = dev.read_output()
            orders = [dev.tile_order(which=0)[0]]
            if adaptive:
                render_adaptive(pbr, dev, px, cam, threshold)
                assert np.array_equal(dev.tile_order(which=0)[0], orders[0])
            dev.reset_accum()
            dev.render(0, seeds, px, cam)
            second = dev.read_output()
            assert same_values(first, second)
            told.append((dev.last_plan(), dev.last_deal(), dev.counters()))
            if adaptive:
                render_adaptive(pbr, dev, px, cam, threshold)
                dev.reset_accum()
                dev.render_frame(float(seeds[0]), 0.0, px, cam)
                frame = dev.read_output()
                want = oracle.Renderer(sc.desc, cfg, threads=16).render_frame(float(seeds[0]), 0.0, px, cam)
                assert same_values(frame, want), describe_mismatch(frame, want)
        finally:
            dev.close()
    assert told[0] == told[1]


# ---- 9: refusals -----------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_rendering(pbr, device):
    sc, cfg, cam, px, _ = mixed_scene(pbr, "cornell-sa", 64, 64)
    seeds = pbr.frame_seeds(0, 8)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    device.render(0, seeds[:4], px, cam)
    want = device.read_output()
    focus = pbr.Camera.from_buffer_copy(cam)
    focus.focusPoint[0], focus.focusPoint[1] = 20, 30
    for why, args in (("pbr_render_dof", (focus, 4, 4, 8, 0.1)), ("min_frames 1 < 2", (cam, 1, 4, 8, 0.1)),
                      ("max_frames 8 < min_frames 9", (cam, 9, 4, 8, 0.1)), ("round_frames 0", (cam, 4, 0, 8, 0.1)),
                      ("negative or not a number", (cam, 4, 4, 8, -0.5)), ("negative or not a number", (cam, 4, 4, 8, float("nan")))):
        with pytest.raises(pbr.PbrError, match=why):
            device.render_adaptive(0, seeds, px, args[0], *args[1:])
        assert same_values(device.read_output(), want), why
    with pytest.raises(pbr.PbrError, match="before pbr_render_adaptive"):
        device.tile_stats()
    device.reset_accum()
    device.render(0, seeds[:4], px, cam)
    assert same_values(device.read_output(), want)


# ---- 10: the diagnostics and the host driver -------------------------------------------------------------------------

def test_last_adaptive_reports_the_schedule(pbr, oracle, device):
    """rounds = the rounds the call ran (it ends when nothing is active), units = 64 x the frames of every tile."""
    sc, cfg, cam, px, threshold = mixed_scene(pbr, "cornell-sa")
    ref = Reference(pbr, oracle, sc.desc, cfg, cam, px, MAX)
    device.upload_scene(sc.desc)
    device.configure(cfg)
    for thr in (threshold, 0.6):
        want_frames, _, want_rounds = ref.decide(MIN, ROUND, MAX, thr)
        device.reset_accum()
        _, (frames, _) = render_adaptive(pbr, device, px, cam, thr)
        rounds, units, fold_ms = device.last_adaptive()
        assert rounds == want_rounds and units == 64 * int(frames.astype(np.uint64).sum()) and fold_ms > 0.0
        assert np.array_equal(frames, want_frames)
    assert want_rounds < 5        # at 0.6 every tile has stopped before max_frames: the call ended early


def test_path_tracer_driver(pbr, device):
    """PathTracer.generateImagesAdaptive == Device.render_adaptive with the driver's seeds and camera."""
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4, "render.brdf": 1})
    sc = pbr.HostScene.generate("cornell", 1, 0)
    w, h = 64, 64
    pt = pbr.PathTracer(0, w, h)
    try:
        pt.initOpenCLBuffers(sc)
        got = pt.generateImagesAdaptive(4, 4, 12, 0.3)
        assert pt.sampleCount() == 0
        cam = pbr.Camera()
        pbr.host.pbrh_pt_camera(pt._h, ctypes.byref(cam))
    finally:
        pt.close()
    device.upload_scene(sc.desc)
    device.configure(sc.config(w, h))
    device.render_adaptive(0, pbr.frame_seeds(0, 12), pbr.pixel_dimension(w, h), cam, 4, 4, 12, 0.3)
    want = device.read_output()
    assert same_values(got, want), describe_mismatch(got, want)
    assert len(histogram(device.tile_stats()[0])) >= 2
