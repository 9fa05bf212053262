"""pbr_read_variance and pbr_denoise_guided (include/pbr_hip.h, csrc/pt_denoise_guided.hpp): the variance pbr_render_adaptive
estimates anyway, read back and handed to the a-trous filter.

The variance is a fixed binary32 algorithm and is compared with `same_values` (tolerance 0) against tests/guided_denoise_ref.py
fed with the device's own per-frame renders.  The filter goes through expf, whose last bit the device and numpy do not share:
it is compared with the restatement at rtol 2e-5, atol 1e-6 + 4 D, D = the largest colour difference between the restatement
with float32 exp and with float64 exp ON THE SAME INPUT — how one ulp of exp propagates through the passes there; measured on
the reference side, never on the device.  With sigma_luminance = 0 there is nothing to tolerate: the colour is pbr_denoise's
with sigma_color = 0, bit for bit.

Scenes as in test_gpu_adaptive.py: HostScene.generate( "cornell", 1, 0 ), render.max_depth 4."""
import numpy as np
import pytest

import adaptive_ref
import guided_denoise_ref as ref
from conftest import same_values, describe_mismatch

pytestmark = pytest.mark.gpu

W, H = 96, 64
FRAMES = 8
PARAMS = {
    "1-pass": dict(passes=1), "3-passes": dict(passes=3), "5-passes": dict(passes=5),
    "sigma-l-1": dict(passes=3, sigma_luminance=1.0),
    "no-features": dict(passes=3, sigma_normal=0.0, sigma_world=0.0, sigma_albedo=0.0),
}


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def cornell(pbr, dev, brdf, w=W, h=H, **more):
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.max_depth": 4, "render.brdf": brdf})
    sc = pbr.HostScene.generate("cornell", 1, 0)
    cfg, cam, px = sc.config(w, h), sc.camera(), pbr.pixel_dimension(w, h)
    for key, value in more.items():
        setattr(cfg, key, value)
    dev.upload_scene(sc.desc)
    dev.configure(cfg)
    return sc, cfg, cam, px


def uniform_round(pbr, dev, px, cam, frames=FRAMES):
    """One adaptive round that every tile renders: min = max = frames, threshold 0."""
    dev.reset_accum()
    dev.render_adaptive(0, pbr.frame_seeds(0, frames), px, cam, frames, frames, frames, 0.0)
    assert (dev.tile_stats()[0] == frames).all()
    return dev.read_output()


# ---- 1: the variance, bit for bit ------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [0, 3])
def test_variance_is_the_restatement_s_bit_for_bit(pbr, device, first):
    """64 x 48 = 48 tiles, tests after 4, 8 and 12 frames.  The per-frame colours are the device's own (a frame rendered onto a
    zero image with weight 0 is the frame's colour); the threshold — the restatement's median error after the first round —
    is chosen so that its frame map has several counts, which is asserted before the device is looked at."""
    w, h, lo, step, hi = 64, 48, 4, 4, 12
    sc, cfg, cam, px = cornell(pbr, device, 1, w, h)
    seeds = pbr.frame_seeds(first, hi)
    colours = []
    for seed in seeds:
        device.reset_accum()
        device.render(0, [seed], px, cam)
        colours.append(pbr.tiles.to_tile_major(device.read_output()))
    colours = np.stack(colours)
    early = adaptive_ref.Moments(colours.shape[1:3])
    for k in range(lo):
        early.add(colours[k])
    threshold = float(np.nanmedian(early.error()))
    want_frames, _, _ = adaptive_ref.run(colours, lo, step, hi, threshold)
    counts = {int(c): int(n) for c, n in zip(*np.unique(want_frames, return_counts=True))}
    print("first %d: threshold %.6g, frames per tile %r" % (first, threshold, counts))
    assert len(counts) >= 2, counts
    want = ref.variance_of_frames(colours, want_frames, adaptive_ref.round_ends(lo, step, hi), first)
    want = pbr.tiles.from_tile_major(want[..., None], w, h)[..., 0]

    device.reset_accum()
    if first:
        device.render(0, pbr.frame_seeds(0, first), px, cam)
    device.render_adaptive(first, seeds, px, cam, lo, step, hi, threshold)
    frames, _ = device.tile_stats()
    assert np.array_equal(frames, want_frames.reshape(h // 8, w // 8))
    got = device.read_variance()
    assert got.shape == (h, w) and got.dtype == np.float32
    assert same_values(got, want), describe_mismatch(got, want)
    assert np.isfinite(got).all() and (got >= 0).all() and got.max() > 0


# ---- 2: the filter against the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("brdf", [1, 0])
@pytest.mark.parametrize("case", sorted(PARAMS))
def test_filter_matches_the_numpy_restatement(pbr, device, brdf, case):
    sc, cfg, cam, px = cornell(pbr, device, brdf)
    before = uniform_round(pbr, device, px, cam)
    stats = device.tile_stats()
    var0 = device.read_variance()
    p = pbr.GuidedDenoiseParams(**PARAMS[case])
    got, var_out, feat = device.denoise_guided(px, cam, p, variance=True, features=True)
    assert same_values(device.read_output(), before)                       # the accumulation is not touched,
    assert same_values(device.read_variance(), var0)                       # nor are the moments
    assert all(same_values(a, b) for a, b in zip(device.tile_stats(), stats))
    assert same_values(got[..., 3], before[..., 3])                        # first-hit distance passes through

    want, want_var = ref.guided_numpy(before, var0, feat, p, px)
    want64, want_var64 = ref.guided_numpy(before, var0, feat, p, px, exp64=True)
    with np.errstate(invalid="ignore"):
        d = np.abs(want[..., :3] - want64[..., :3])
        spread = float(d[np.isfinite(d)].max())
        err = np.abs(got[..., :3].astype(np.float64) - want[..., :3])
        err = float(err[np.isfinite(err)].max())
        var_spread = np.abs(want_var - want_var64) / np.maximum(np.abs(want_var), 1e-30)
        var_err = np.abs(var_out.astype(np.float64) - want_var) / np.maximum(np.abs(want_var), 1e-30)
    print("brdf %d %s: D %.3g, colour max |device - restatement| %.3g (max |colour| %.3g); variance max relative: between the exp variants %.3g, device %.3g"
          % (brdf, case, spread, err, float(np.nanmax(np.abs(want[..., :3]))), float(np.nanmax(var_spread)), float(np.nanmax(var_err))))
    assert np.allclose(got[..., :3], want[..., :3], rtol=2e-5, atol=1e-6 + 4 * spread, equal_nan=True), (err, spread)
    assert np.abs(got[..., :3] - before[..., :3]).max() > 1e-3              # ... and it did something

    usable = np.isfinite(var0)
    if p.passes == 1:
        assert np.allclose(var_out, want_var, rtol=4e-5, atol=1e-12, equal_nan=True), float(np.nanmax(var_err))
    assert np.isfinite(var_out[usable]).all() and (var_out[usable] >= 0).all()
    assert var_out[usable].mean() < var0[usable].mean()


# ---- 3: without the luminance term it is pbr_denoise -----------------------------------------------------------------

@pytest.mark.parametrize("brdf", [1, 0])
@pytest.mark.parametrize("passes", [1, 3])
def test_sigma_luminance_zero_is_pbr_denoise_without_the_colour_term(pbr, device, brdf, passes):
    sc, cfg, cam, px = cornell(pbr, device, brdf)
    uniform_round(pbr, device, px, cam)
    got = device.denoise_guided(px, cam, pbr.GuidedDenoiseParams(passes=passes, sigma_luminance=0.0))
    want = device.denoise(px, cam, pbr.DenoiseParams(passes=passes, sigma_color=0.0))
    assert same_values(got, want), describe_mismatch(got, want)
    assert np.abs(got[..., :3] - device.read_output()[..., :3]).max() > 1e-3


# ---- 4: the sky ------------------------------------------------------------------------------------------------------

def test_open_sky_is_a_fixed_point_and_is_not_mixed_with_geometry(pbr, device):
    """test_gpu_denoise.py's scene: without the jitter every frame of a miss pixel is the sky colour — variance 0, and taps
    across the hit / miss divide are left out, so it still holds that colour afterwards."""
    w, h = 96, 64
    pbr.cfg_reset()
    pbr.cfg_set(**{"render.antialiasing": 0.0})
    sc = pbr.HostScene.generate("dragon", 2, 4000)
    cam, px = sc.camera(), pbr.pixel_dimension(w, h)
    device.upload_scene(sc.desc)
    device.configure(sc.config(w, h))
    noisy = uniform_round(pbr, device, px, cam, 2)
    out, feat = device.denoise_guided(px, cam, pbr.GuidedDenoiseParams(passes=2), features=True)   # taps reach 2 * (1 + 2) = 6 pixels
    miss = feat[1][..., 3] == 0
    assert 0.02 < miss.mean() < 0.98
    # (silhouette pixels that are miss-class by their centre ray but carry a surface's colour — see test_gpu_denoise.py —
    # and whatever they can reach are set aside)
    impure = miss & ~np.isinf(noisy[..., 3])
    assert impure.mean() < 0.01
    reach = np.zeros_like(impure)
    for y, x in zip(*np.nonzero(impure)):
        reach[max(0, y - 6): y + 7, max(0, x - 6): x + 7] = True
    pure = miss & ~reach
    assert pure.mean() > 0.02
    assert np.allclose(out[pure][:, :3], noisy[pure][:, :3], rtol=1e-6)
    hit = ~miss
    assert np.abs(out[hit][:, :3] - noisy[hit][:, :3]).max() > 1e-3          # while the surfaces were filtered


# ---- 5: it helps -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("brdf", [1, 0])
def test_guided_frame_is_closer_to_the_converged_one(pbr, device, brdf):
    """0.5 is the factor test_gpu_denoise.py asks of pbr_denoise; the restatement alone gives 0.13 (BRDF 1) and 0.065 (BRDF 0)
    on these inputs."""
    sc, cfg, cam, px = cornell(pbr, device, brdf)
    noisy = uniform_round(pbr, device, px, cam)
    out = device.denoise_guided(px, cam)
    device.reset_accum()
    device.render(0, pbr.frame_seeds(1000, 512), px, cam)
    converged = device.read_output()
    ok = np.isfinite(converged[..., :3]).all(-1) & np.isfinite(noisy[..., :3]).all(-1) & np.isfinite(out[..., :3]).all(-1)
    assert ok.mean() > 0.99
    mse = lambda a: float(((a[..., :3] - converged[..., :3])[ok] ** 2).mean())
    print("brdf %d: mse guided %.4g, unfiltered %.4g, ratio %.3g" % (brdf, mse(out), mse(noisy), mse(out) / mse(noisy)))
    assert mse(out) < 0.5 * mse(noisy), (mse(out), mse(noisy))


# ---- 6: state and arguments ------------------------------------------------------------------------------------------

def refused(pbr, dev, px, cam, why="pbr_render_adaptive"):
    for call in (dev.read_variance, lambda: dev.denoise_guided(px, cam)):
        with pytest.raises(pbr.PbrError, match=why):
            call()


def test_state_errors(pbr, device):
    sc, cfg, cam, px = cornell(pbr, device, 1, 64, 48)
    seeds = pbr.frame_seeds(0, 4)
    refused(pbr, device, px, cam)                                         # before any adaptive call
    spoilers = {
        "render": lambda: device.render(0, seeds[:2], px, cam),
        "render_frame": lambda: device.render_frame(float(seeds[0]), 0.0, px, cam),
        "accumulate": device.accumulate,
        "reset_accum": device.reset_accum,
        "write_input": lambda: device.write_input(np.zeros((48, 64, 4), np.float32)),
    }
    for name, spoil in spoilers.items():
        device.reset_accum()
        device.render_adaptive(0, seeds, px, cam, 4, 4, 4, 0.0)
        assert device.read_variance().shape == (48, 64)
        assert device.denoise_guided(px, cam).shape == (48, 64, 4)
        spoil()
        before = device.read_output()
        refused(pbr, device, px, cam)
        assert same_values(device.read_output(), before), name            # a refused call leaves the image as it was
        if name == "render":
            frames, error = device.tile_stats()                           # another flag: still the adaptive call's
            assert (frames == 4).all()


def test_tile_sharding_is_refused(pbr, device):
    sc, cfg, cam, px = cornell(pbr, device, 1, 64, 48, tile_world=2, tile_rank=0)
    device.render_adaptive(0, pbr.frame_seeds(0, 4), px, cam, 4, 4, 4, 0.0)
    refused(pbr, device, px, cam, "tile sharding")
    assert len(device.tile_stats()) == 3


def test_argument_errors(pbr, device):
    sc, cfg, cam, px = cornell(pbr, device, 1, 64, 48)
    device.render_adaptive(0, pbr.frame_seeds(0, 4), px, cam, 4, 4, 4, 0.0)
    before = device.read_output()
    for bad in (dict(passes=0), dict(passes=9), dict(sigma_luminance=-1.0), dict(sigma_world=float("nan"))):
        with pytest.raises(pbr.PbrError):
            device.denoise_guided(px, cam, pbr.GuidedDenoiseParams(**bad))
        assert same_values(device.read_output(), before), bad
    assert pbr.hip.pbr_denoise_guided(device._ctx, px, None, None, None, None, None) == -1      # PBR_EINVAL
    assert pbr.hip.pbr_read_variance(device._ctx, None) == -1
    out, var = device.denoise_guided(px, cam, variance=True)                # ... and the context still answers
    assert out.shape == (48, 64, 4) and var.shape == (48, 64) and device.last_kernel_ms() > 0.0
