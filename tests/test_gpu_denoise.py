"""pbr_denoise (csrc/pt_denoise.hpp).  The reference's noise filter is an unfinished
sketch (source/opencl/noise_filtering.cl:386-401 are TODOs), so there is nothing to be bit-identical WITH: this is a
floating-point pass checked against an fp32 numpy restatement of its definition in include/pbr_hip.h — tolerance
2e-5 relative + 1e-6 absolute (expf on the device vs numpy's float32 exp: an ulp or two per tap, 25 taps) — against
traced rays for the feature buffers, and through properties on rendered frames.  The oracle is not involved."""
import numpy as np
import pytest

from denoise_ref import atrous_numpy

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 1e-6


@pytest.fixture()
def device(pbr, gpu_device):
    dev = pbr.Device(gpu_device)
    yield dev
    dev.close()


def rendered(pbr, dev, kind="cornell", triangles=0, w=96, h=64, frames=4, **cfg):
    pbr.cfg_reset()
    pbr.cfg_set(**cfg)
    sc = pbr.HostScene.generate(kind, 2, triangles)
    cam, px = sc.camera(), pbr.pixel_dimension(w, h)
    dev.upload_scene(sc.desc)
    dev.configure(sc.config(w, h))
    dev.render(0, pbr.frame_seeds(0, frames), px, cam)
    return sc, cam, px


def test_features_are_the_first_hits_of_the_pixel_centre_rays(pbr, device):
    """position | t, normal | hit, Kd | material against pbr_diag_trace over rays built here from the camera basis
    (pathtracing.cl:25-48 without the jitter)."""
    w, h = 96, 64
    sc, cam, px = rendered(pbr, device, "sponza", 6000, w, h, 1)
    _, feat = device.denoise(px, cam, features=True)
    position, normal, albedo = feat
    f32 = np.float32
    eye, cw, cu, cv = (np.array([v.x, v.y, v.z], f32) for v in (cam.eye, cam.w, cam.u, cam.v))
    ys, xs = np.mgrid[0:h, 0:w].astype(f32)
    inner = (cu - cu * f32(w)) + cu * (f32(2) * xs[..., None])
    inner = inner + cv
    inner = inner - cv * f32(h)
    inner = inner + cv * (f32(2) * ys[..., None])
    initial = cw + inner * (f32(px) * f32(0.5))
    dirs = (initial / np.linalg.norm(initial, axis=-1, keepdims=True)).astype(f32)
    rays = np.concatenate([np.broadcast_to(eye, dirs.shape), dirs], axis=-1).reshape(-1, 6).astype(f32)
    t, face, n, _ = device.diag_trace(rays)
    t, n = t.reshape(h, w), n.reshape(h, w, 3)
    hit = np.isfinite(t)
    agree = hit == (normal[..., 3] == 1)
    assert agree.mean() > 0.995                                          # silhouettes: the rays differ in the last bit
    both = hit & agree
    assert both.mean() > 0.5
    assert np.allclose(position[..., 3][both], t[both], rtol=1e-4)
    flipped = np.where((n * dirs).sum(-1, keepdims=True) > 0, -n, n)
    close = np.abs(normal[..., :3][both] - flipped[both]).max(-1) < 1e-4
    assert close.mean() > 0.995                                          # edges between faces
    assert np.allclose(position[..., :3][both], (eye + dirs * t[..., None])[both], rtol=1e-4, atol=1e-4)
    miss = ~hit & agree
    assert np.isinf(position[..., 3][miss]).all() and (albedo[..., 3][miss] == -1).all() and not normal[miss].any()
    arr = sc.arrays()
    material = albedo[..., 3][both].astype(np.int64)
    assert material.min() >= 0 and material.max() < arr["materials"].shape[0]


@pytest.mark.parametrize("params", [
    dict(passes=1), dict(passes=3), dict(passes=5),
    dict(passes=3, sigma_color=0.0), dict(passes=2, sigma_normal=0.0, sigma_world=0.0, sigma_albedo=0.0),
    dict(passes=3, sigma_color=0.2, sigma_normal=0.1, sigma_world=1.0, sigma_albedo=0.05),
])
def test_filter_matches_the_numpy_restatement(pbr, device, params):
    w, h = 96, 64
    sc, cam, px = rendered(pbr, device, "cornell", 0, w, h, 4)
    p = pbr.DenoiseParams(**params)
    before = device.read_output()
    got, feat = device.denoise(px, cam, p, features=True)
    assert np.array_equal(device.read_output(), before, equal_nan=True)   # the accumulation is not touched
    want = atrous_numpy(before, feat, p, px)
    assert np.array_equal(got[..., 3], before[..., 3], equal_nan=True)    # first-hit distance passes through
    assert np.allclose(got[..., :3], want[..., :3], rtol=RTOL, atol=ATOL), float(np.abs(got[..., :3] - want[..., :3]).max())
    assert np.abs(got[..., :3] - before[..., :3]).max() > 1e-3            # ... and it did something


def test_open_sky_is_a_fixed_point_and_is_not_mixed_with_geometry(pbr, device):
    """Without the jitter every sample of a pixel is its centre ray: miss pixels hold the sky colour exactly
    (pathtracing.cl:263-266); taps across the hit / miss divide are left out, so they still do afterwards — next to
    surfaces of any colour."""
    w, h = 96, 64
    sc, cam, px = rendered(pbr, device, "dragon", 4000, w, h, 2, **{"render.antialiasing": 0.0})
    noisy = device.read_output()
    out, feat = device.denoise(px, cam, pbr.DenoiseParams(passes=2), features=True)      # taps reach 2 * (1 + 2) = 6 pixels
    miss = feat[1][..., 3] == 0
    assert 0.02 < miss.mean() < 0.98
    # (a handful of silhouette pixels are miss-class by their centre ray and carry a surface's colour: the renderer
    # normalises the direction once more, pt_utils.cl:327-340, and lands on the other side of an edge; whatever they
    # can reach is set aside)
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


def test_denoised_low_sample_frame_is_closer_to_the_converged_one(pbr, device):
    w, h = 128, 96
    sc, cam, px = rendered(pbr, device, "cornell", 0, w, h, 4)
    out = device.denoise(px, cam)
    noisy = device.read_output()
    device.reset_accum()
    device.render(0, pbr.frame_seeds(100, 512), px, cam)
    converged = device.read_output()
    ok = np.isfinite(converged[..., :3]).all(-1) & np.isfinite(noisy[..., :3]).all(-1)
    mse = lambda a: float(((a[..., :3] - converged[..., :3])[ok] ** 2).mean())
    assert mse(out) < 0.5 * mse(noisy), (mse(out), mse(noisy))


def test_denoise_of_the_gathered_frame_equals_the_unsharded_one(pbr, device):
    import torch
    w, h = 72, 40
    sc, cam, px = rendered(pbr, device, "cornell", 0, w, h, 3)
    want = device.denoise(px, cam)
    world, devs, gathered = 2, [], None
    for rank in range(world):
        d = pbr.Device(0)
        devs.append(d)
        cfg = sc.config(w, h)
        cfg.tile_world, cfg.tile_rank = world, rank
        d.upload_scene(sc.desc)
        d.configure(cfg)
        d.render(0, pbr.frame_seeds(0, 3), px, cam)
        if gathered is None:
            gathered = torch.zeros(world * d.tile_bytes() // 4, dtype=torch.float32, device="cuda")
        d.export_tiles(gathered.data_ptr() + rank * d.tile_bytes())
    torch.cuda.synchronize()
    with pytest.raises(pbr.PbrError, match="pbr_import_tiles"):
        devs[0].denoise(px, cam)
    devs[0].import_tiles(gathered.data_ptr())
    assert np.array_equal(devs[0].denoise(px, cam), want, equal_nan=True)
    for d in devs:
        d.close()


def test_denoise_argument_errors(pbr, device):
    pbr.cfg_reset()
    sc = pbr.HostScene.generate("cornell", 1, 0)
    cam, px = sc.camera(), pbr.pixel_dimension(64, 40)
    with pytest.raises(pbr.PbrError, match="before"):
        device.denoise(px, cam)
    device.upload_scene(sc.desc)
    device.configure(sc.config(64, 40))
    for bad in (dict(passes=0), dict(passes=9), dict(sigma_color=-1.0), dict(sigma_world=float("nan"))):
        with pytest.raises(pbr.PbrError):
            device.denoise(px, cam, pbr.DenoiseParams(**bad))
    out = device.denoise(px, cam)                                         # nothing rendered yet: zeros in, zeros out
    assert out.shape == (40, 64, 4) and not out[..., :3].any()
