"""pbr_display on the device against the numpy restatement (tests/display_ref.py): the histogram exactly, the 8-bit image byte
for byte, the adaptation's doubles exactly.

Images are planted the way test_display_step_is_the_clamped_linear_image does — write_input, one render_frame with weight 1,
read_output — under a black sky with the eye far above the scene: every ray misses, the frame's colour is 0 and the fold
0 + ( planted - 0 ) * 1 leaves the planted words as they are (plant() asserts it), so the thresholds planted below really sit in
the accumulation.  Every comparison is against what read_output says the context holds.

Sizes: 8 x 8 — one tile, one wave, fewer pixels than a workgroup; 72 x 40 — 45 tiles, not a multiple of any workgroup's share
(4 groups per histogram workgroup, 64 x 4 pixels per map workgroup), top-row-first differs from bottom-first; 1024 x 520 — see
LARGE."""
import ctypes

import numpy as np
import pytest

import display_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
# The histogram kernel's launch shape (csrc/pt_display.hpp): at most kHistogramMaxBlocks = 2048 workgroups of four waves, a
# group of 64 pixels per wave and trip, so one trip of the stride loop covers 2048 * 4 = 8192 groups = 524288 pixels.
# 1024 x 520 = 532480 pixels = 8320 groups: workgroups 0 .. 31 make a second trip, the others one; the all-equal image puts
# 532480 > 65535 pixels into one bin.
LARGE = (1024, 520)
SIZES = {"tile": (8, 8), "odd": (72, 40), "large": LARGE}
assert LARGE[0] * LARGE[1] // 64 > 2048 * 4 and LARGE[0] * LARGE[1] > 65535


class Stage:
    """One context per size, shared by the tests of this module: a Cornell box that no ray of the planting frame reaches."""

    def __init__(self, pbr):
        self.pbr, self.devices = pbr, {}
        pbr.cfg_reset()
        pbr.cfg_set(**{"render.max_depth": 3})
        self.scene = pbr.HostScene.generate("cornell", 1, 0)
        self.cam = self.scene.camera()
        self.cam.eye.y = 1.0e4

    def config(self, w, h, world=1, rank=0):
        cfg = self.scene.config(w, h)
        for i in range(4):
            cfg.sky_light[i] = 0.0
        cfg.tile_world, cfg.tile_rank = world, rank
        return cfg

    def device(self, w, h, world=1, rank=0):
        key = (w, h, world, rank)
        if key not in self.devices:
            dev = self.pbr.Device(0)
            dev.upload_scene(self.scene.desc)
            dev.configure(self.config(w, h, world, rank))
            self.devices[key] = dev
        return self.devices[key]

    def plant(self, dev, image):
        """The image the context holds afterwards: the planted one, word for word, on the tiles the context owns."""
        w, h = dev.width, dev.height
        dev.write_input(image)
        dev.render_frame(0.0333, 1.0, self.pbr.pixel_dimension(w, h), self.cam)
        held = dev.read_output()
        return held

    def close(self):
        for dev in self.devices.values():
            dev.close()
        self.pbr.cfg_reset()


@pytest.fixture(scope="module")
def stage(pbr, gpu_device):
    s = Stage(pbr)
    yield s
    s.close()


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def same_values(a, b):
    return np.array_equal(a, b, equal_nan=True)


def log_uniform(w, h, seed):
    """Channels 2^u, u uniform over -20 .. 20; the special values and every sRGB threshold with both neighbours sprinkled in, as
    many as the image has room for."""
    rng = np.random.default_rng(seed)
    image = np.exp2(rng.uniform(-20.0, 20.0, (h, w, 4))).astype(F32)
    T = ref.TABLE[1:]
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-42, np.finfo(F32).max, 65504.0, 1.0, 2.0 ** -16, 2.0 ** 16, 1e-30, 0.5], F32)
    planted = np.concatenate([special, T, np.nextafter(T, F32(np.inf)), np.nextafter(T, F32(-np.inf))])
    flat = image.reshape(-1, 4)
    slots = rng.permutation(flat.shape[0] * 3)[:min(planted.size, flat.shape[0] * 3 // 2)]
    flat[slots // 3, slots % 3] = planted[:slots.size]
    if flat.shape[0] > 64:
        flat[5, :3], flat[6, :3], flat[7, :3] = 0.0, np.nan, (-1.0, -0.0, 0.0)      # whole pixels that are dark,
        flat[8, :3], flat[9, :3], flat[10, :3] = 1e-6, 2.0 ** -17, 1e-40              # below the first bin's lower edge,
        flat[11, :3], flat[12, :3] = 1e6, np.inf                                      # and beyond the last bin's upper edge
    return image


def images(w, h):
    equal = np.empty((h, w, 4), F32)
    equal[...] = (0.5, 0.4, 0.3, 1.0)
    return {"log-uniform": log_uniform(w, h, 7), "all-equal": equal, "black": np.zeros((h, w, 4), F32)}


def manual(pbr, exposure=1.0, curve=ref.CLAMP, transfer=ref.LINEAR, white=4.0):
    return pbr.DisplayParams(exposure_mode=ref.MANUAL, exposure=exposure, curve=curve, transfer=transfer, white=white)


def auto(pbr, curve=ref.ACES, transfer=ref.SRGB, adapt=1.0, low=0.05, high=0.05, key=0.18, white=4.0, lo2=-16.0, hi2=16.0):
    return pbr.DisplayParams(exposure_mode=ref.AUTO, key=key, low_fraction=low, high_fraction=high, min_log2=lo2, max_log2=hi2, adapt=adapt,
                             curve=curve, white=white, transfer=transfer)


def check_histogram(info, held):
    counts, counted, dark = ref.histogram(held[..., :3])
    assert np.array_equal(info["histogram"], counts) and info["counted"] == counted and info["dark"] == dark
    assert counted + dark == held.shape[0] * held.shape[1]
    return counts


@pytest.mark.parametrize("size", sorted(SIZES))
def test_histogram_equals_the_restatement_exactly(pbr, stage, size):
    w, h = SIZES[size]
    dev = stage.device(w, h)
    for name, image in images(w, h).items():
        held = stage.plant(dev, image)
        assert same_values(held[..., :3], image[..., :3]), name         # the plant is exact (the fold turns a planted -0 into +0)
        _, info = dev.display(manual(pbr), info=True)
        counts = check_histogram(info, held)
        assert (info["log2_target"], info["log2_used"], info["exposure"]) == (0.0, 0.0, 1.0)
        if name == "all-equal":
            assert counts.max() == w * h and info["dark"] == 0 and (size != "large" or counts.max() > 65535)
        if name == "black":
            assert info["counted"] == 0 and info["dark"] == w * h
        if name == "log-uniform" and size != "tile":
            assert (counts[1:255] > 0).sum() > 100 and counts[0] > 0 and counts[255] > 0 and info["dark"] >= 3


def test_histogram_does_not_depend_on_the_merge_rounds(pbr, stage):
    w, h = SIZES["odd"]
    dev = stage.device(w, h)
    try:
        for name, image in images(w, h).items():
            held = stage.plant(dev, image)
            for rounds in (0, 1, 2, 4, -1):
                dev.set_knob("display_merge", rounds)
                check_histogram(dev.display(manual(pbr), info=True)[1], held)
    finally:
        dev.set_knob("display_merge", -1)


@pytest.mark.parametrize("size", sorted(SIZES))
def test_image_equals_the_restatement_byte_for_byte(pbr, stage, size):
    """Every curve x transfer, manual (exposure 1 — every threshold planted is crossed as it stands — and 0.37) and auto."""
    w, h = SIZES[size]
    dev = stage.device(w, h)
    held = stage.plant(dev, log_uniform(w, h, 7))
    counts = ref.histogram(held[..., :3])[0]
    for curve in (ref.CLAMP, ref.REINHARD, ref.ACES):
        for transfer in (ref.LINEAR, ref.SRGB):
            for exposure in (1.0, 0.37):
                got, info = dev.display(manual(pbr, exposure, curve, transfer), info=True)
                assert info["exposure"] == F32(exposure)
                assert np.array_equal(got, ref.image(held, info["exposure"], curve, transfer, 4.0)), (curve, transfer, exposure)
            dev.display_reset()
            got, info = dev.display(auto(pbr, curve, transfer, low=0.1, high=0.02), info=True)
            want_target = ref.target(counts, 0.1, 0.02, -16.0, 16.0)
            assert info["log2_target"] == want_target and info["log2_used"] == want_target
            want_exposure = float(ref.exposure_of(0.18, want_target))
            assert abs(info["exposure"] - want_exposure) <= 2.0 ** -22 * want_exposure
            assert np.array_equal(got, ref.image(held, info["exposure"], curve, transfer, 4.0)), (curve, transfer, "auto")
    if size != "tile":
        codes = dev.display(manual(pbr, 1.0, ref.CLAMP, ref.SRGB))[..., :3]
        assert set(np.unique(codes).tolist()) == set(range(256))       # every code boundary was crossed
    top = dev.display(manual(pbr, 1.0, ref.ACES, ref.SRGB), top_row_first=True)
    assert np.array_equal(top, ref.image(held, 1.0, ref.ACES, ref.SRGB, 4.0, top_row_first=True)) and (top[..., 3] == 255).all()
    assert size == "tile" or not np.array_equal(top, top[::-1])


def test_linear_settings_equal_read_display(pbr, stage):
    """{ manual, exposure 1, curve 0, transfer 0 } against pbr_read_display in both row orders, on the image of
    test_display_step_is_the_clamped_linear_image: NaN, both infinities, values below 0 and above 1."""
    w, h = SIZES["odd"]
    dev = stage.device(w, h)
    rng = np.random.default_rng(5)
    img = rng.uniform(-0.5, 1.5, (h, w, 4)).astype(F32)
    img[3, 5, 0], img[4, 6, 1], img[0, 0, 2] = np.nan, np.inf, -np.inf
    lin = stage.plant(dev, img)
    assert np.isnan(lin[3, 5, 0]) and lin[4, 6, 1] == np.inf and lin[0, 0, 2] == -np.inf and (lin[..., :3] > 1.0).any() and (lin[..., :3] < 0.0).any()
    for top in (False, True):
        assert np.array_equal(dev.display(manual(pbr), top_row_first=top), dev.read_display(top_row_first=top))
    assert not np.array_equal(dev.read_display(), dev.read_display(top_row_first=True))


@pytest.mark.parametrize("size", ["tile", "odd"])
def test_host_image_equals_the_accumulated_one(pbr, stage, size):
    w, h = SIZES[size]
    dev = stage.device(w, h)
    held = stage.plant(dev, log_uniform(w, h, 9))
    for params in (auto(pbr, low=0.2, high=0.1), manual(pbr, 2.5, ref.REINHARD, ref.SRGB)):
        for top in (False, True):
            dev.display_reset()
            inner, inner_info = dev.display(params, top_row_first=top, info=True)
            dev.display_reset()
            outer, outer_info = dev.display(params, rgba=held, top_row_first=top, info=True)
            assert np.array_equal(inner, outer)
            assert np.array_equal(inner_info.pop("histogram"), outer_info.pop("histogram")) and inner_info == outer_info


def test_adaptation_moves_the_stated_share_and_is_forgotten_on_reset_and_configure(pbr, stage):
    w, h = SIZES["odd"]
    dev = stage.device(w, h)
    with np.errstate(over="ignore"):
        bright, dark = log_uniform(w, h, 21) * F32(64.0), log_uniform(w, h, 22) * F32(1.0 / 64.0)
    half = auto(pbr, adapt=0.5)
    dev.display_reset()
    held = stage.plant(dev, bright)
    _, first = dev.display(half, info=True)
    t1 = ref.target(ref.histogram(held[..., :3])[0], 0.05, 0.05, -16.0, 16.0)
    assert first["log2_target"] == t1 and first["log2_used"] == t1                    # nothing remembered: a jump
    held = stage.plant(dev, dark)
    t2 = ref.target(ref.histogram(held[..., :3])[0], 0.05, 0.05, -16.0, 16.0)
    assert t2 < t1 - 4
    dev.display(manual(pbr, 3.0), info=True)                                           # a manual call in between changes nothing
    got, second = dev.display(half, info=True)
    assert second["log2_target"] == t2 and second["log2_used"] == t1 + 0.5 * (t2 - t1)
    assert np.array_equal(got, ref.image(held, second["exposure"], ref.ACES, ref.SRGB, 4.0))
    _, third = dev.display(half, info=True)
    assert third["log2_used"] == second["log2_used"] + 0.5 * (t2 - second["log2_used"])
    _, jump = dev.display(auto(pbr, adapt=1.0), info=True)                              # adapt 1 jumps
    assert jump["log2_used"] == t2
    stage.plant(dev, bright)
    dev.display_reset()
    assert dev.display(half, info=True)[1]["log2_used"] == t1                          # forgotten: a jump
    dev.configure(stage.config(w, h))
    held = stage.plant(dev, dark)
    assert dev.display(half, info=True)[1]["log2_used"] == t2                          # pbr_configure forgets it too


def test_sharded_contexts(pbr, stage):
    import torch
    w, h = SIZES["odd"]
    world = 2
    image = log_uniform(w, h, 31)
    whole = stage.device(w, h)
    held = stage.plant(whole, image)
    params = manual(pbr, 0.8, ref.ACES, ref.SRGB)
    want, want_info = whole.display(params, info=True)
    ranks, gathered = [stage.device(w, h, world, r) for r in range(world)], None
    for rank, dev in enumerate(ranks):
        part = stage.plant(dev, image)
        mask = pbr.tiles.rows_of_rank(w, h, world, rank)
        assert same_words(part[mask], held[mask]) and not part[~mask].any()
        got, info = dev.display(params, info=True)
        assert np.array_equal(got[mask], want[mask]) and not got[~mask][..., :3].any() and (got[..., 3] == 255).all()
        counts, counted, dark = ref.histogram(part[..., :3])                        # other ranks' tiles read 0: dark
        assert np.array_equal(info["histogram"], counts) and (info["counted"], info["dark"]) == (counted, dark)
        with pytest.raises(pbr.PbrError, match=r"-3: pbr_display: auto exposure over a shard's tiles .* pass it as rgba"):
            dev.display(auto(pbr))
        if gathered is None:
            gathered = torch.zeros(world * dev.tile_bytes() // 4, dtype=torch.float32, device="cuda")
        dev.export_tiles(gathered.data_ptr() + rank * dev.tile_bytes())
    torch.cuda.synchronize()
    ranks[0].import_tiles(gathered.data_ptr())
    full = ranks[0].read_full()
    assert same_words(full[..., :3], held[..., :3])
    whole.display_reset()
    want, want_info = whole.display(auto(pbr), info=True)
    got, info = ranks[0].display(auto(pbr), rgba=full, info=True)
    assert np.array_equal(got, want) and info["log2_used"] == want_info["log2_used"] and info["exposure"] == want_info["exposure"]
    assert np.array_equal(info["histogram"], want_info["histogram"]) and info["dark"] == want_info["dark"]


def test_state_refusals_and_what_a_display_leaves_alone(pbr, stage):
    fresh = pbr.Device(0)
    try:
        fresh.width, fresh.height = 8, 8
        with pytest.raises(pbr.PbrError, match="-3: pbr_display before pbr_configure"):
            fresh.display(manual(pbr))
        fresh.upload_scene(stage.scene.desc)
        with pytest.raises(pbr.PbrError, match="-3: pbr_display before pbr_configure"):
            fresh.display(auto(pbr))
    finally:
        fresh.close()
    w, h = SIZES["odd"]
    dev = stage.device(w, h)
    with np.errstate(over="ignore"):
        bright, dark = log_uniform(w, h, 41) * F32(16.0), log_uniform(w, h, 42) * F32(1.0 / 16.0)
    held = stage.plant(dev, bright)
    dev.display_reset()
    remembered = dev.display(auto(pbr), info=True)[1]["log2_used"]
    before = dev.read_output()
    out = np.zeros((h, w, 4), np.uint8)
    refused = [(auto(pbr, key=0.0), "key"), (auto(pbr, adapt=0.0), "adapt"), (auto(pbr, low=0.6, high=0.5), "low_fraction"), (auto(pbr, lo2=3.0, hi2=2.0), "max_log2"),
               (auto(pbr, curve=ref.REINHARD, white=-1.0), "white"), (auto(pbr, curve=7), "curve"), (auto(pbr, transfer=2), "transfer"),
               (manual(pbr, exposure=float("nan")), "exposure"), (pbr.DisplayParams(exposure_mode=5), "exposure_mode")]
    for params, field in refused:
        with pytest.raises(pbr.PbrError, match=r"-1: pbr_display: .*%s" % field):
            dev.display(params)
    assert pbr.hip.pbr_display(dev._ctx, None, None, out.ctypes.data, 0, None) == -1
    assert pbr.hip.pbr_display(dev._ctx, ctypes.byref(auto(pbr)), None, None, 0, None) == -1
    assert (out == 0).all()
    for params in (auto(pbr), manual(pbr, 1.7, ref.REINHARD, ref.SRGB)):
        dev.display(params, info=True)
        hist_ms, map_ms = dev.display_info()
        assert dev.last_kernel_ms() > 0 and hist_ms > 0 and map_ms > 0 and abs(dev.last_kernel_ms() - (hist_ms + map_ms)) < 1e-9
    dev.display(manual(pbr))
    assert dev.display_info()[0] == 0.0 and dev.last_kernel_ms() > 0                 # manual without info launches no histogram
    assert same_words(dev.read_output(), before)                                     # the accumulation is not modified
    # every refusal left the remembered exposure as it was: the next auto call moves from it
    held = stage.plant(dev, dark)
    target = ref.target(ref.histogram(held[..., :3])[0], 0.05, 0.05, -16.0, 16.0)
    assert dev.display(auto(pbr, adapt=0.5), info=True)[1]["log2_used"] == remembered + 0.5 * (target - remembered)
